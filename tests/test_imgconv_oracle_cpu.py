"""The exact oracle of tests/test_imgconv_paths_gpu.py, checked without a GPU.

Data conditions: every case's reference meets its regime's conditions (imgconv_cases' docstring): the
``unit`` cap of 256, for ``wide`` ties of both kinds and every sum below 2^24, every operand a non-zero
integer.

Honesty: for every case the project's fp32 CPU reference path (conv2d / conv2d_weight) passes ``check``
against the oracle (a tap loop of float64 tensordots): two independent implementations agree bit for bit.

Sensitivity: for every case and every mutation that applies to it (imgconv_cases.mutations states
which), ``check`` of the mutated oracle's output against the true oracle fails.

Coverage: the expected-path names over all cases are the full lists CONV_PATHS / WGRAD_PATHS, every shape
is one a ``*_supported`` predicate accepts, and the hand-derived geometry figures of the path table in
test_imgconv_paths_gpu.py hold.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgconv_cases as ic  # noqa: E402


@pytest.fixture(autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("group", list(ic.GROUPS))
def test_oracle_conditions_reference_path_and_sensitivity(group):
    """One pass per case (the oracle's sums are computed once and shared): data conditions, the CPU
    reference path against the oracle, and every applicable mutation caught."""
    cases = ic.GROUPS[group]()
    caught = 0
    for c in cases:
        b = ic.build(c)
        ic.conditions(b)
        ref, info = ic.oracle(b)
        ic.check(b, ic.run(b, "cpu"), ref)
        ic.check(b, ic.as_buffers(b, ref), ref)   # the packing used below is itself clean
        for m in ic.mutations(b, info):
            wrong = ic.oracle(b, mutate=m)[0]
            with pytest.raises(AssertionError):
                ic.check(b, ic.as_buffers(b, wrong), ref)
            caught += 1
    print("%s: %d cases, %d mutations caught" % (group, len(cases), caught))


def test_check_sees_guards_nan_and_unwritten_argmax():
    c = ic.per_image_cases()[0]
    b = ic.build(c)
    ref = ic.oracle(b)[0]
    good = ic.as_buffers(b, ref)
    for name, at, val in (("y", ic.GUARD - 1, 0.0), ("y", -ic.GUARD, 0.0), ("y", ic.GUARD, float("nan")),
                          ("argmax", ic.GUARD - 1, 0), ("argmax", -1, 0), ("argmax", ic.GUARD + 5, 0xFF)):
        got = {k: v.clone() for k, v in good.items()}
        got[name][at] = val
        with pytest.raises(AssertionError):
            ic.check(b, got, ref)


def test_cases_cover_every_path_and_are_supported():
    seen = {"conv": set(), "wgrad": set()}
    for group in ic.GROUPS.values():
        for c in group():
            assert (ic.conv_supported if c.kind == "conv" else ic.wgrad_supported)(c), c
            seen[c.kind].add(ic.path(c))
            if c.kind == "conv":
                # the few-channel path is forward-only; dilated sources need the persistent kernel
                assert c.CS > 4 or (c.src == "plain" and not c.flip and c.dil == 1), c
                assert c.dil == 1 or ic.path(c).startswith("cfg"), c
    assert seen["conv"] == set(ic.CONV_PATHS), seen["conv"] ^ set(ic.CONV_PATHS)
    assert seen["wgrad"] == set(ic.WGRAD_PATHS), seen["wgrad"] ^ set(ic.WGRAD_PATHS)


def test_path_table_of_the_gpu_test():
    """The rows of the module docstring of test_imgconv_paths_gpu.py (CONV_TABLE / WGRAD_TABLE there) against
    imgconv_cases' mirror of the dispatch conditions."""
    import test_imgconv_paths_gpu as paths

    for c, want_path, want_npf, want_epi in paths.CONV_TABLE:
        assert ic.conv_path(c) == want_path, (c, ic.conv_path(c))
        if want_path.startswith("cfg"):
            wm, wn = (int(x) for x in want_path[4:want_path.index(">")].split(",")[2:])
            assert ic.persist_npf(c, 64 * wm * wn) == want_npf, c
            assert ic.conv_epilogue(c) == want_epi, c
            nt = int(want_path[4])
            key = (c.O, c.CS, c.stride, c.K, wn * nt * 16)
            assert ic.persist_layout(c, wn * nt * 16) == paths.LAYOUTS[key], (c, ic.persist_layout(c, wn * nt * 16))
            # stage_out as launch_cfg decides it, from the table's own figures
            fits = paths.LAYOUTS[key][2] + c.O * c.O * c.N * 2 <= 160 * 1024
            assert (want_epi == "staged") == (not c.pool and c.N % 8 == 0 and c.O & (c.O - 1) == 0 and fits), c
    for c, want_path, want_npf in paths.WGRAD_TABLE:
        assert ic.wgrad_path(c) == want_path, (c, ic.wgrad_path(c))
        if want_path.startswith("wp"):
            assert ic.wgrad_npf(c) == want_npf, c
    # every persistent case of the groups is a row of a table
    rows = {c for c, *_ in paths.CONV_TABLE} | {c for c, *_ in paths.WGRAD_TABLE}
    for group in ic.GROUPS.values():
        for c in group():
            if ic.path(c).startswith(("cfg", "wp")):
                assert ic.dataclasses.replace(c, regime="unit") in rows, c
