"""The float64 oracle of tests/test_gemm_dense_paths_gpu.py, checked without a GPU.

Honesty: for every case ``ops.gemm``'s CPU reference path (fp32, the oracle of the other kernel
tests) lands within the oracle's bound, so the two references cannot drift apart.

Sensitivity: for every case three wrong kernels, expressed as mutated oracles, must break the
bound - the last k-term dropped, the first k-term counted twice, the output shifted by one column.
The two k-term mutations must break it at every element they touch (every element whose mutated
value differs from the reference at all, act'(aux) = 0 hides the term from any test; under a ReLU
the elements neither value of which is clamped, a clamp passes on only what lies above 0).  A shifted output puts the neighbouring column's sum in each place, and two
random sums can land within one rounding of each other, so for it the condition is: every output
row and every output column it touches holds an element that breaks the bound, and at least 9 in 10 of the
touched elements do.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_dense_cases as gd  # noqa: E402


@pytest.fixture(autouse=True)
def _one_thread():
    """Hundreds of tiny matrix products: a thread pool per product only costs time."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("group", list(gd.GROUPS))
def test_oracle_agrees_with_cpu_reference(group):
    worst = 0.0
    for c in gd.GROUPS[group]():
        b = gd.build(c)
        worst = max(worst, gd.check(b, gd.run(b, "cpu")))
    print("%s: CPU reference max err / bound = %.3g" % (group, worst))


def _mutants(b, ref):
    for how in ("drop_last", "dup_first"):
        yield how, gd.oracle(b, mutate=how)
    shifted = {k: (np.roll(v[0], 1, axis=1), None) for k, v in ref.items() if k != "bias_out"}
    yield "shift", shifted


@pytest.mark.parametrize("group", list(gd.GROUPS))
def test_bound_catches_wrong_kernels(group):
    margin = np.inf
    for c in gd.GROUPS[group]():
        b = gd.build(c)
        ref = gd.oracle(b)
        for how, mut in _mutants(b, ref):
            for name, (m, _) in mut.items():
                r, bound = ref[name]
                touched = m != r
                if c.act == gd.ops.ACT_RELU:   # a clamped value shows only the part of the term above 0, or none
                    touched &= (m != 0) & (r != 0)
                if how == "shift" and r.shape[1] == 1:
                    continue  # one column: nowhere to shift to
                assert touched.any(), (c, how, name)
                broke = np.abs(m - r) > bound
                if how == "shift":
                    hit = broke & touched
                    for ax in (0, 1):   # (a row or column the shift leaves as it was, K = 1 with equal neighbours, has nothing to find)
                        assert (hit.any(axis=ax) | ~touched.any(axis=ax)).all(), (c, how, name, ax)
                    assert hit.sum() >= 0.9 * touched.sum(), (c, how, name, int(hit.sum()), int(touched.sum()))
                else:
                    assert broke[touched].all(), "%s: %s misses %s at %d of %d touched elements" % (
                        c, how, name, int((~broke & touched).sum()), int(touched.sum()))
                    margin = min(margin, float((np.abs(m - r)[touched] / bound[touched]).min()))
    print("%s: smallest mutation / bound = %.3g" % (group, margin))


def test_expected_loop_table_matches_prefetch_depth():
    """The k-loop table in test_gemm_dense_paths_gpu.py, against the host mirror of PrefetchDepth."""
    import test_gemm_dense_paths_gpu as paths

    for (tile, dtype), depth in paths.RING_DEPTH.items():
        assert gd.prefetch_depth(tile, dtype) == depth, (tile, dtype)
        for nk in (1, 2, 3, 4, 5, 7, 9):
            want = "fast" if depth == 1 or nk <= 2 else "deep%d" % depth
            assert gd.expected_loop(tile, dtype, nk) == want == paths.interior_loop(tile, dtype, nk)
    assert set(paths.RING_DEPTH) == {(t, d) for t in range(5) for d in ("bf16", "f32")}


def test_guarded_buffers_hold_every_access():
    """The dense tiles' binding does not bounds-check operands: every case's logical extent
    (rows - 1) * ld + width fits its buffer with a guard on either side, and every GEMM stays small
    (at most 3 x 3 tiles, K <= 640)."""
    for group in gd.GROUPS.values():
        for c in group():
            b = gd.build(c)
            ra, rb = c.M - (c.ones == "a"), c.N - (c.ones == "b")
            for buf, start, ld, rows, mode in ((b.A, b.a_start, b.lda, ra, c.amode), (b.B, b.b_start, b.ldb, rb, c.bmode)):
                ext = (rows - 1) * ld + c.K if mode == gd.ops.KMAJ else (c.K - 1) * ld + rows
                assert start >= gd.GUARD and start + ext + gd.GUARD <= buf.numel(), c
            assert b.out_start + (c.M - 1) * c.ldc_ + c.N + gd.GUARD <= b.out.numel(), c
            assert c.M <= 3 * gd.TILE_DIMS[c.tile][0] and c.N <= 3 * gd.TILE_DIMS[c.tile][1] and c.K <= 640, c
