"""gemm_dense_kernel (tiles 0-4 of ops.gemm): every k-loop, loader branch, tail and epilogue path
against a float64 oracle, inside NaN-guarded buffers, with a derived per-element bound.

Cases, oracle, guards and the bound live in tests/gemm_dense_cases.py (its docstring states the
bound); tests/test_gemm_dense_oracle_cpu.py proves on the CPU that the bound catches a dropped or
doubled k-term and a shifted output in every case.

Which k-loop the interior workgroup of a launch takes (gemm_core.h gemm_mainloop; the edge
workgroups of the same launch always take gemm_kloop<false>).  all_fast holds for it when its rows
are whole, the strides are multiples of 8, the bases 16-B aligned and K (or the split's chunk) a
multiple of 64; then D = PrefetchDepth picks

    D = SLOT_REGS <= 24 ? 4 : SLOT_REGS <= 32 ? 3 : 1,   SLOT_REGS = 4 * ((BM + BN) * 64 * sizeof(T) / 16 / 256)

    tile (BM x BN)   dtype  SLOT_REGS  D   nk = 1, 2          nk = 3, 4, 5, 7, 9
    0 (64 x 64)      bf16   16         4   gemm_kloop<true>   gemm_kloop_deep<4>   (nk = 4: D, 5: D + 1, 9: 2D + 1)
    0 (64 x 64)      f32    32         3   gemm_kloop<true>   gemm_kloop_deep<3>   (nk = 3: D, 4: D + 1, 5: D + 2, 7: 2D + 1)
    1 (128 x 128)    bf16   32         3   gemm_kloop<true>   gemm_kloop_deep<3>
    1 (128 x 128)    f32    64         1   gemm_kloop<true>   gemm_kloop<true>
    2 (128 x 64)     bf16   24         4   gemm_kloop<true>   gemm_kloop_deep<4>
    2 (128 x 64)     f32    48         1   gemm_kloop<true>   gemm_kloop<true>
    3 (64 x 128)     bf16   24         4   gemm_kloop<true>   gemm_kloop_deep<4>
    3 (64 x 128)     f32    48         1   gemm_kloop<true>   gemm_kloop<true>
    4 (32 x 32)      bf16   8          4   gemm_kloop<true>   gemm_kloop_deep<4>
    4 (32 x 32)      f32    16         4   gemm_kloop<true>   gemm_kloop_deep<4>

RING_DEPTH below is the D column; the CPU test checks it against the formula.

Measured on an MI355X at commit b7007eb (the parent of the commit that added this file):

    activation allowance (test_activation_error_within_allowance: the activated output against the
    float64 activation of the kernel's own fp32 z, relative, the fp32 store's rounding included)
        sigmoid (1 / (1 + __expf(-z)))   4.58e-7 = 2^-21.06   ->  ACT_ALLOW = 4 x = 1.83e-6
        tanh (tanhf)                     1.32e-7 = 2^-22.85   ->  ACT_ALLOW = 4 x = 5.28e-7
      both below 2^-20, so both are adopted.

    largest err / bound per test (every tile of a parametrised test)
        test_kloop_selection                  0.040   (fp32 operands, K = 64)
        test_kloop_split_k                    0.0048
        test_k_tails_and_unaligned_operands   0.148   (K = 7 and 9: the bound is smallest there)
        test_m_n_edges                        0.037
        test_store_paths                      0.988   (bf16 out: a value just above a power of two rounds by almost
        test_epilogues                        0.990    the whole 2^-8 * |ref|; the fp32 CPU reference reaches the same)
        test_ones_row_bias_out                0.037
        test_combined_epilogue_split_k        0.981   (bf16 out)
"""
import dataclasses
import os
import sys

import numpy as np
import pytest

from dtfe import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_dense_cases as gd  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ring depth D of gemm_kloop_deep per (tile, operand dtype): the table in the module docstring
RING_DEPTH = {(0, "bf16"): 4, (0, "f32"): 3, (1, "bf16"): 3, (1, "f32"): 1, (2, "bf16"): 4, (2, "f32"): 1,
              (3, "bf16"): 4, (3, "f32"): 1, (4, "bf16"): 4, (4, "f32"): 4}


def interior_loop(tile, dtype, nk):
    """The loop an all_fast workgroup takes at nk k-tiles: "fast" = gemm_kloop<true>, "deepD" = gemm_kloop_deep<D>."""
    d = RING_DEPTH[(tile, dtype)]
    return "deep%d" % d if d > 1 and nk > 2 else "fast"


def _run_all(name, cases):
    worst, at = 0.0, None
    for c in cases:
        b = gd.build(c)
        ref = gd.oracle(b)
        ws = None
        if c.splits > 1 and not c.atomic:
            ws = ops.split_workspace(DEV, c.splits, c.M, c.N, c.tile, private=True)
        # a ticketed split-K launch runs twice on the same workspace: the kernel must have reset its counters
        for _ in range(2 if ws is not None else 1):
            r = gd.check(b, gd.run(b, DEV, workspace=ws), ref)
            if r > worst:
                worst, at = r, c
    print("%s: %d cases, max err / bound = %.3g at %s" % (name, len(cases), worst, at))


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
def test_kloop_selection(tile):
    """nk = 1..9 whole k-tiles on a 2 x 2 grid: the interior workgroup takes gemm_kloop<true> or the deep
    ring (table above: nk = D, D + 1, D + 2, 2D + 1 for D = 3 and 4), the three edge workgroups of the
    same launch gemm_kloop<false>; both dtypes, four layouts."""
    cases = gd.kloop_cases([tile])
    loops = {interior_loop(c.tile, c.dtype, c.K // gd.KT) for c in cases}
    assert loops == {"fast"} | {"deep%d" % RING_DEPTH[(tile, d)] for d in ("bf16", "f32") if RING_DEPTH[(tile, d)] > 1}
    _run_all("kloop tile %d" % tile, cases)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
def test_kloop_split_k(tile):
    """6 and 7 k-tiles split 2 and 3 ways (chunks of 3, 2 and 4 + 3, 3 + 3 + 1 k-tiles), ticketed
    (private workspace, launched twice) and atomic."""
    _run_all("split-K tile %d" % tile, gd.splitk_cases([tile]))


@pytest.mark.parametrize("tile", [0, 1, 4])
def test_k_tails_and_unaligned_operands(tile):
    """K in {1, 7, 8, 9, 63, 65, 127, 129, 201} with tight strides, strides padded to 8 (vector loads, the
    last chunk crossing K), strides padded by 3 (scalar loads) and a base one element off 16-B alignment."""
    _run_all("K tails tile %d" % tile, gd.ktail_cases([tile]))


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
def test_m_n_edges(tile):
    """M in {1, 15, 17, BM - 1, BM + 1} x N in {1, 7, 9, BN - 1, BN + 1} (tiles 1-3: the diagonal)."""
    _run_all("M/N edges tile %d" % tile, gd.edge_cases([tile]))


def test_store_paths():
    """8-wide vector store (ldc = 72), per-element (ldc = 77), misaligned base (ldc = 80, out one element
    in), partial last chunk (N = 70, ldc = 72); fp32 and bf16 out."""
    _run_all("store paths", gd.store_cases())


def test_epilogues():
    """bias on either axis, act 0-3, alpha = -0.5, beta over fp32 and bf16, out2 (fp32 / bf16, plain /
    transposed), aux (fp32, bf16 with ld_aux % 8 == 0 and != 0) with aux_act 1-3; each with the vector
    store open (ldc = 72) and closed (ldc = 77)."""
    _run_all("epilogues", gd.epilogue_cases())


def test_ones_row_bias_out():
    """a_ones_row = M - 1 and b_ones_row = N - 1 routed to bias_out, stored and atomic, inside an edge
    tile and first of a tile."""
    _run_all("ones rows", gd.ones_cases())


def test_combined_epilogue_split_k():
    _run_all("combined", gd.combined_cases())


def test_activation_error_within_allowance():
    """The device sigmoid / tanh on the kernel's own fp32 pre-activation z (the same GEMM with act = NONE)
    against the float64 activation of that z: the relative error stays inside ACT_ALLOW."""
    for c in gd.epilogue_cases():
        if c.act not in (ops.ACT_SIGMOID, ops.ACT_TANH):
            continue
        b = gd.build(c)
        got = gd.logical_outputs(b, gd.run(b, DEV))["out"][0]
        b.case = dataclasses.replace(c, act=ops.ACT_NONE)
        z = gd.logical_outputs(b, gd.run(b, DEV))["out"][0]
        want = gd._act(z, c.act)
        rel = float((np.abs(got - want) / np.abs(want)).max())
        print("act %d %s ldc %d: max relative error %.3g = 2^%.2f" % (c.act, c.dtype, c.ldc, rel, np.log2(max(rel, 1e-30))))
        assert rel <= gd.ACT_ALLOW[c.act], (c, rel)
