"""The exact oracle of tests/test_igemm_paths_gpu.py, checked without a GPU.

Data conditions: every case's reference meets its regime's conditions (igemm_cases' docstring): non-zero
integer operands, every partial sum below 2^24, the ``unit`` cap of 256, ties of both kinds for
``rounded``, and the statistics' bounds by sums of absolute values.

Honesty: for every case the project's fp32 CPU reference path (ops.conv_fwd / conv_dgrad / conv_wgrad on
CPU tensors: conv2d / conv2d_input / conv2d_weight, bn_stats, bn_bwd_stats) passes ``check`` against the
oracle, a float64 tap loop: two independent implementations agree bit for bit.  The CPU path accumulates
as the unsplit epilogue does - it stores bf16(S) and then adds the old value - so it is compared with
the oracle's unsplit rounding, RNE(RNE(S) + old), in every case.  That is also the oracle's expectation
for the GPU except in the accumulating split-K cases; among those the two roundings differ only in the
``rounded`` ones (asserted below), which the CPU path therefore does not vouch for: there the
expectation RNE(S + old) rests on the oracle alone.

Sensitivity: for every case and every mutation that applies to it (igemm_cases.mutations states which),
``check`` of the mutated oracle's output against the true oracle fails.

Coverage: the path names over all cases are the declared list PATHS of test_igemm_paths_gpu.py, the kernel
instantiations they run are the full list igemm_cases.INSTANTIATIONS, and every row of the hand-derived
table there agrees with the mirror.
"""
import collections
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import igemm_cases as gc  # noqa: E402


@pytest.fixture(autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _pass(group):
    """One pass per case of the group (run once, shared by the tests below): data conditions, the CPU
    reference path against the oracle, and every applicable mutation caught.  Returns (number of cases,
    mutations caught by name, (ties up, ties down) of the ``rounded`` cases, the cases whose split-K
    accumulation rounding differs from the unsplit one)."""
    cases = gc.GROUPS[group]()
    assert len(set(cases)) == len(cases), "duplicate cases"
    caught, ties, differs = collections.Counter(), [], []
    for c in cases:
        b = gc.build(c)
        gc.conditions(b)
        ref, inf = gc.oracle(b)
        unsplit = gc.oracle(b, split_rounding=False)[0]
        gc.check(b, gc.run(b, "cpu"), unsplit)
        if c.kind == "dgrad" and not np.array_equal(ref["dx"], unsplit["dx"]):
            assert c.accumulate and c.regime == "rounded" and gc.gemm_info(c)["splits"] > 1, c
            differs.append(c)
            with pytest.raises(AssertionError):   # ... and ``check`` tells the two roundings apart
                gc.check(b, gc.as_buffers(b, unsplit), ref)
        gc.check(b, gc.as_buffers(b, ref), ref)   # the packing used below is itself clean
        for m in gc.mutations(b):
            wrong = gc.oracle(b, mutate=m)[0]
            with pytest.raises(AssertionError):
                gc.check(b, gc.as_buffers(b, wrong), ref)
            caught[m] += 1
        if c.regime == "rounded":
            ties.append((inf["ties_up"], inf["ties_down"]))
    return len(cases), caught, ties, differs


@pytest.mark.parametrize("group", list(gc.GROUPS))
def test_oracle_conditions_reference_path_and_sensitivity(group):
    n, caught, _, _ = _pass(group)
    print("%s: %d cases, %d mutations caught (%s)" % (group, n, sum(caught.values()),
                                                      ", ".join("%s %d" % kv for kv in sorted(caught.items()))))


def test_every_mutation_is_caught_and_ties_of_both_kinds_exist():
    """Over all groups: each of the twelve mutations applied to (and was caught in) some case, a ``rounded``
    case held ties of both kinds, and some case separates the split-K accumulation rounding from the unsplit."""
    caught, ties, differs = collections.Counter(), [], []
    for group in gc.GROUPS:
        _, k, t, d = _pass(group)
        caught.update(k)
        ties += t
        differs += d
    assert set(caught) == set(gc.MUTATIONS), set(gc.MUTATIONS) - set(caught)
    assert any(u > 0 and d > 0 for u, d in ties), ties
    assert differs, "no case separates RNE(S + old) from RNE(RNE(S) + old)"


def test_check_sees_guards_nan_and_unwritten_elements():
    c = next(c for c in gc.fwd_cases() if c.stats)
    b = gc.build(c)
    ref = gc.oracle(b)[0]
    good = gc.as_buffers(b, ref)
    gc.check(b, good, ref)
    for name, at, val in (("y", gc.GUARD - 1, 0.0), ("y", -gc.GUARD, 0.0), ("y", -1, float("nan")),
                          ("y", gc.GUARD, float("nan")), ("stats", gc.GUARD - 1, 0.0), ("stats", -1, 1.0),
                          ("stats", gc.GUARD + 3, float("nan"))):
        got = {k: v.clone() for k, v in good.items()}
        got[name][at] = val
        with pytest.raises(AssertionError):
            gc.check(b, got, ref)
    got = {k: v.clone() for k, v in good.items()}
    got["y"] = b.bufs["y"].clone()          # nothing written: the NaN pre-fill is still there
    with pytest.raises(AssertionError):
        gc.check(b, got, ref)
    for c in (gc.dgrad_cases()[0], gc.wgrad_tap_cases()[0]):
        b = gc.build(c)
        ref = gc.oracle(b)[0]
        name = b.outputs[0]
        for at in (0, gc.GUARD - 1, -gc.GUARD, -1):
            got = gc.as_buffers(b, ref)
            got[name][at] = 1.0
            with pytest.raises(AssertionError):
                gc.check(b, got, ref)


def test_cases_cover_every_path_and_instantiation():
    import test_igemm_paths_gpu as paths

    seen, inst = collections.defaultdict(set), set()
    for name, group in gc.GROUPS.items():
        for c in group():
            # shapes the implicit-GEMM launchers accept (launch_igemm_fwd / dgrad / wgrad)
            assert c.C % 64 == 0 and c.Cout % 64 == 0 and c.KH * c.KW <= 9 and c.stride <= 2, c
            seen[name].add(gc.path(c))
            inst |= gc.instantiations(c)
    for name in gc.GROUPS:
        assert seen[name] == set(paths.PATHS[name]), (name, sorted(seen[name] ^ set(paths.PATHS[name])))
    assert inst == set(gc.INSTANTIATIONS), inst ^ set(gc.INSTANTIATIONS)


def test_path_table_of_the_gpu_test():
    """The rows of the module docstring of test_igemm_paths_gpu.py (TABLE there) against the mirror, and the
    figures the issue names: reduce S = 1, 2, 4, 8, 16 and the unrolled loop, 2 / 33 fold chunks, absent tiles."""
    import test_igemm_paths_gpu as paths

    every = {c for group in gc.GROUPS.values() for c in group()}
    for c, want in paths.TABLE:
        assert c in every, c
        assert gc.path(c) == want, (c, gc.path(c))
    tap = [gc.wgrad_info(c) for c in gc.wgrad_tap_cases()]
    assert {i["S"] for i in tap} == {0, 1, 2, 4, 8, 16} and any(i["unrolled"] for i in tap)
    stats = {(c.H, c.W): gc.gemm_info(c) for c in gc.fwd_cases() if c.stats and c.tile == "64x64"}
    assert (stats[(48, 48)]["tiles"], stats[(48, 48)]["chunks"]) == (72, 2)
    assert (stats[(257, 256)]["tiles"], stats[(257, 256)]["chunks"]) == (2056, 33)
    fused = [gc.gemm_info(c) for c in gc.dgrad_stats_cases() if gc.gemm_info(c)["stat"] == "fused"]
    assert any(i["absent"] > 0 and i["bm"] == 128 for i in fused) and any(i["absent"] > 0 and i["bm"] == 64 for i in fused)
    assert any(i["zero"] == 3 for i in fused)
