"""The implicit-GEMM convolutions of csrc/kernels/igemm.hip (ops.conv_fwd / conv_dgrad / conv_wgrad with C and
Cout multiples of 64) bit for bit against an exact float64 oracle, inside NaN-guarded buffers.

Cases, guards, oracle, dispatch mirror and ``check`` live in tests/igemm_cases.py (its docstring states the
two data regimes, ``unit`` and ``rounded``, on which the kernels have to be exact, how accumulation
rounds on the unsplit and the split-K path, and why the statistics are exact); tests/test_igemm_oracle_cpu.py
proves on the CPU that the data conditions hold, that the project's fp32 reference path agrees with the
oracle, and that ``check`` catches twelve kinds of wrong kernel.  Every comparison below is
``torch.equal``; there is no tolerance to tune.

Which kernels a case reaches
----------------------------
Forward and data gradient, run_igemm (M = rows of the largest phase, N = output channels, k-tiles of 64):

  tile     DTFE_IG_TILE=BMxBN when N % BN == 0; else the first of 128x128, 128x64, 64x64 with
           ceil(M / BM) * (N / BN) * phases >= 240 workgroups, else 64x64.  Every case here has fewer
           than 240, so auto = 64x64; 64x128 is reached through the knob only.
  phases   forward 1.  Data gradient stride^2, phase (py, px) visits the taps with (py + pad - kh) and
           (px + pad - kw) divisible by the stride: 3x3 s2 pad 1 -> 1, 2, 2, 4 taps; 2x2 s2 -> 1 each; 1x1 s2 ->
           1, 0, 0, 0.  ``accumulate`` without BN statistics drops the zero-tap phases (p1z0 for the 1x1 s2);
           otherwise they are launched and write zeros (p4z3).
  splits   only one phase and stride 1: DTFE_IG_SPLIT, or on auto doubled while workgroups * splits < 200 and
           k-tiles / (2 * splits) >= 6; clipped to the k-tile count.  The partials are combined by
           splitk_to_bf16_kernel.  A masked accumulation source (acc_src) does not split.
  stats    forward: fused epilogue partials + bn_part_fold when unsplit ("fused"), else the bn_stats pass
           ("pass").  Data gradient (BN-backward): fused (igemm_kernel<.., BB>) with more than one phase,
           the bn_bwd_stats pass with one.

  case (B = 2 unless stated)                                   k-tiles  workgroups  path
  fwd 1x1 64->64 5x7 (70 rows)                                     1        2       fwd:64x64:s1:p1z0:none
  fwd 3x3 64->128 6x10 pad 1 (120 rows)                            9        4       fwd:64x64:s1:p1z0:none  (9 / 2 < 6)
  fwd 3x3 512->128 7x7 pad 1, rounded                             72        4       fwd:64x64:s8:p1z0:none  (72 / 16 < 6)
  fwd 1x1 640->64 5x7, DTFE_IG_SPLIT=3 (+ stats)                  10        2       fwd:64x64:s3:p1z0:none / :pass
  fwd 1x1 128->64 5x7, DTFE_IG_SPLIT=5                             2        2       fwd:64x64:s2:p1z0:none  (clipped)
  fwd 1x1 64->64 48x48 stats, tile 64x64                           1       72       fwd:64x64:s1:p1z0:fused (72 tiles, 2 chunks)
  fwd 1x1 64->64 257x256 stats, tile 64x64                         1     2056       fwd:64x64:s1:p1z0:fused (33 chunks)
  dgrad 1x1 s2 256->128 9x6                                        -        -       dgrad:64x64:s1:p4z3:none
  dgrad 1x1 s2 256->128 9x6 accumulate                             -        -       dgrad:64x64:s1:p1z0:none (stride 2: no split)
  dgrad 3x3 s2 64->128 7x12, tile 128x128                          -        -       dgrad:128x128:s1:p4z0:none
  dgrad 3x3 128->64 7x7 pad 1 accumulate                          18        2       dgrad:64x64:s2:p1z0:none (18 / 4 < 6)
  dgrad 3x3 512->128 7x7 pad 1 rounded (+ accumulate)             72        4       dgrad:64x64:s8:p1z0:none
  dgrad 1x1 128->512 7x7 acc_src, DTFE_IG_SPLIT=2                  2       16       dgrad:64x64:s1:p1z0:none (acc_src: unsplit)
  dgrad 3x3 128->64 7x7 pad 1 acc_src                             18        2       dgrad:64x64:s1:p1z0:none (acc_src: unsplit)
  dgrad 3x3 s2 64->128 7x12 B=6 bn, tile 128x128 (rows 144, 144, 108, 108: 2 absent tiles)   dgrad:128x128:s1:p4z0:fused
  dgrad 3x3 s2 64->128 9x9 B=6 bn, tile 64x64 (rows 150, 120, 120, 96: 3 absent tiles)       dgrad:64x64:s1:p4z0:fused
  dgrad 1x1 s2 256->128 9x6 bn                                     -        -       dgrad:64x64:s1:p4z3:fused
  dgrad 3x3 128->64 6x10 pad 1 bn                                 18        4       dgrad:64x64:s2:p1z0:pass

Weight gradient, launch_igemm_wgrad (M = B * OH * OW):

  all taps  igemm_wgrad3_kernel: 3x3, stride 1, pad 1, W <= 62, (64 / W + 2) * (W + 2) <= 192 patch pixels and
            DTFE_IG_W3 = 1 (or unset / 2 with C, Cout <= 64).  k-tiles of R = 64 / W rows, T = B * ceil(H / R) of them;
            splits = DTFE_IG_WSPLIT, or min(ceil(192 / tiles), T / 4), clipped to T.
  per tap   igemm_wgrad_kernel<BM, BN>, BM = 128 if Cout % 128 == 0 else 64, BN likewise from C; splits =
            DTFE_IG_WSPLIT, or min(ceil(192 / tiles), ceil(M / 256)); mchunk = ceil(M / splits) rounded up to 64,
            splits = ceil(M / mchunk).
  reduce    splits > 1: wgrad_splits_reduce_kernel<S>, S doubled from 1 while S < 16, 2 S <= splits and
            (len / 4) * S / 256 < 512; its 8-way unrolled trip runs when splits > 7 S ("u").

  case                                                            splits -> after mchunk   path
  tap 3x3 64->64 B=10 16x16 (M 2560, len 36864), WSPLIT=2              2 (mchunk 1280)     wgrad:tap64x64:s2:r2
    WSPLIT=3                                                           3 (896)             wgrad:tap64x64:s3:r2
    WSPLIT=5                                                           5 (512)             wgrad:tap64x64:s5:r4
    WSPLIT=9                                                           8 (320)             wgrad:tap64x64:s8:r8
    WSPLIT=17                                                         14 (192)             wgrad:tap64x64:s14:r8
    WSPLIT=40                                                         40 (64)              wgrad:tap64x64:s40:r16
    auto: min(ceil(192 / 9), 10)                                      10 (256)             wgrad:tap64x64:s10:r8
  tap 3x3 512->128 7x7 (len 589824: 576 position groups), WSPLIT=2     2 (64)              wgrad:tap128x128:s2:r1
  tap 3x3 512->128 B=10 8x8 (M 640), WSPLIT=10                        10 (64)              wgrad:tap128x128:s10:r1u
  w3 64->64 5x62 (R 1, T 10), auto min(192, 10 / 4)                    2                   wgrad:w3:s2:r2
  w3 64->64 5x2 (R 32, T 2), auto                                      1                   wgrad:w3:s1:r0
  w3 64->128 5x62, WSPLIT=50 (clipped to T)                           10                   wgrad:w3:s10:r8
  w3 knob on, 5x63 (W > 62)                                            3 (256)             wgrad:tap64x64:s3:r2
  w3 knob on, 6x62 pad 0                                               2 (256)             wgrad:tap64x64:s2:r2

TABLE below holds these rows and PATHS every path name each group reaches; the CPU test checks both against
igemm_cases' mirror of the host code.

Measured on an MI355X
---------------------
At commit da7a72a (the parent of the commit that added this file), split-K was taken with a masked
accumulation source (acc_src), and its combine kernel, splitk_to_bf16_kernel, adds dx's old contents and knows
nothing of the source.  The three acc_src cases that reached split-K there - DTFE_IG_SPLIT=2 on the 1x1 128->512
at 7x7 (2 splits), the automatic split of the 3x3 128->64 at 7x7 (2 splits) and of the ``rounded`` 3x3 512->64
at 7x7 (8 splits) - failed with NaN in every element of dx: the NaN pre-fill, read back as the old value.  The
four unsplit acc_src cases and the other 142 cases were bit-equal with untouched guards the first time they
ran.  With run_igemm keeping an acc_src launch unsplit all 149 cases pass.  Wall time of each test's call (the
host's float64 oracle and the copies included; the launches are microseconds):

    test_forward        45 cases   0.79 s
    test_dgrad          41         0.12 s
    test_dgrad_stats    21         0.06 s
    test_wgrad_tap      22         0.14 s
    test_wgrad_w3       20         0.08 s
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import igemm_cases as gc  # noqa: E402
from igemm_cases import Case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

_K3 = dict(KH=3, KW=3, pad=1)
_S2 = dict(C=128, Cout=64, KH=3, KW=3, stride=2, pad=1)
_SWEEP = dict(kind="wgrad", w3=0, B=10, H=16, W=16, C=64, Cout=64, scale=0.25, **_K3)
_BIG = dict(kind="wgrad", w3=0, C=512, Cout=128, scale=0.5, **_K3)
_W3 = dict(kind="wgrad", w3=1, **_K3)

# (case, path): the rows of the tables above
TABLE = [
    (Case("fwd", H=5, W=7, C=64, Cout=64), "fwd:64x64:s1:p1z0:none"),
    (Case("fwd", H=6, W=10, C=64, Cout=128, **_K3), "fwd:64x64:s1:p1z0:none"),
    (Case("fwd", H=7, W=7, C=512, Cout=128, regime="rounded", **_K3), "fwd:64x64:s8:p1z0:none"),
    (Case("fwd", H=5, W=7, C=640, Cout=64, split=3), "fwd:64x64:s3:p1z0:none"),
    (Case("fwd", H=5, W=7, C=640, Cout=64, split=3, stats=True), "fwd:64x64:s3:p1z0:pass"),
    (Case("fwd", H=5, W=7, C=128, Cout=64, split=5), "fwd:64x64:s2:p1z0:none"),
    (Case("fwd", H=48, W=48, C=64, Cout=64, tile="64x64", stats=True), "fwd:64x64:s1:p1z0:fused"),
    (Case("fwd", H=257, W=256, C=64, Cout=64, tile="64x64", stats=True, free=4), "fwd:64x64:s1:p1z0:fused"),
    (Case("dgrad", H=9, W=6, C=128, Cout=256, stride=2), "dgrad:64x64:s1:p4z3:none"),
    (Case("dgrad", H=9, W=6, C=128, Cout=256, stride=2, accumulate=True), "dgrad:64x64:s1:p1z0:none"),
    (Case("dgrad", H=7, W=12, tile="128x128", **_S2), "dgrad:128x128:s1:p4z0:none"),
    (Case("dgrad", H=7, W=7, C=64, Cout=128, accumulate=True, **_K3), "dgrad:64x64:s2:p1z0:none"),
    (Case("dgrad", H=7, W=7, C=128, Cout=512, regime="rounded", **_K3), "dgrad:64x64:s8:p1z0:none"),
    (Case("dgrad", H=7, W=7, C=128, Cout=512, regime="rounded", accumulate=True, **_K3), "dgrad:64x64:s8:p1z0:none"),
    (Case("dgrad", H=7, W=7, C=512, Cout=128, split=2, accumulate=True, acc_src=True), "dgrad:64x64:s1:p1z0:none"),
    (Case("dgrad", H=7, W=7, C=64, Cout=128, accumulate=True, acc_src=True, **_K3), "dgrad:64x64:s1:p1z0:none"),
    (Case("dgrad", H=7, W=12, B=6, bn="relu_x", tile="128x128", **_S2), "dgrad:128x128:s1:p4z0:fused"),
    (Case("dgrad", H=9, W=9, B=6, bn="relu_x", tile="64x64", **_S2), "dgrad:64x64:s1:p4z0:fused"),
    (Case("dgrad", H=9, W=6, C=128, Cout=256, stride=2, bn="relu_x"), "dgrad:64x64:s1:p4z3:fused"),
    (Case("dgrad", H=6, W=10, C=64, Cout=128, bn="relu_x", **_K3), "dgrad:64x64:s2:p1z0:pass"),
    (Case(wsplit=2, **_SWEEP), "wgrad:tap64x64:s2:r2"),
    (Case(wsplit=3, **_SWEEP), "wgrad:tap64x64:s3:r2"),
    (Case(wsplit=5, **_SWEEP), "wgrad:tap64x64:s5:r4"),
    (Case(wsplit=9, **_SWEEP), "wgrad:tap64x64:s8:r8"),
    (Case(wsplit=17, **_SWEEP), "wgrad:tap64x64:s14:r8"),
    (Case(wsplit=40, **_SWEEP), "wgrad:tap64x64:s40:r16"),
    (Case(**_SWEEP), "wgrad:tap64x64:s10:r8"),
    (Case(H=7, W=7, wsplit=2, **_BIG), "wgrad:tap128x128:s2:r1"),
    (Case(B=10, H=8, W=8, wsplit=10, **_BIG), "wgrad:tap128x128:s10:r1u"),
    (Case(H=5, W=62, C=64, Cout=64, scale=0.25, **_W3), "wgrad:w3:s2:r2"),
    (Case(H=5, W=2, C=64, Cout=64, scale=0.25, **_W3), "wgrad:w3:s1:r0"),
    (Case(H=5, W=62, C=64, Cout=128, wsplit=50, scale=0.5, **_W3), "wgrad:w3:s10:r8"),
    (Case(H=5, W=63, C=64, Cout=64, **_W3), "wgrad:tap64x64:s3:r2"),
    (Case(H=6, W=62, C=64, Cout=64, **{**_W3, "pad": 0}), "wgrad:tap64x64:s2:r2"),
]

# every path name the cases of a group reach (igemm_cases.path), by the test below that runs the group
PATHS = {
    "fwd": (
        "fwd:64x64:s1:p1z0:none", "fwd:128x64:s1:p1z0:none", "fwd:64x128:s1:p1z0:none", "fwd:128x128:s1:p1z0:none",
        "fwd:64x64:s1:p1z0:fused", "fwd:128x128:s1:p1z0:fused",
        "fwd:64x64:s2:p1z0:none", "fwd:128x64:s2:p1z0:none", "fwd:64x64:s3:p1z0:none", "fwd:64x64:s8:p1z0:none",
        "fwd:64x64:s2:p1z0:pass", "fwd:64x64:s3:p1z0:pass"),
    "dgrad": (
        "dgrad:64x64:s1:p1z0:none", "dgrad:128x128:s1:p1z0:none",
        "dgrad:64x64:s1:p4z0:none", "dgrad:128x64:s1:p4z0:none", "dgrad:64x128:s1:p4z0:none", "dgrad:128x128:s1:p4z0:none",
        "dgrad:64x64:s1:p4z3:none",
        "dgrad:64x64:s2:p1z0:none", "dgrad:128x64:s2:p1z0:none",
        "dgrad:64x64:s8:p1z0:none"),
    "dgrad_stats": (
        "dgrad:64x64:s1:p4z0:fused", "dgrad:128x64:s1:p4z0:fused", "dgrad:64x128:s1:p4z0:fused",
        "dgrad:128x128:s1:p4z0:fused", "dgrad:64x64:s1:p4z3:fused",
        "dgrad:64x64:s1:p1z0:pass", "dgrad:64x64:s2:p1z0:pass"),
    "wgrad_tap": (
        "wgrad:tap64x64:s1:r0", "wgrad:tap64x128:s1:r0", "wgrad:tap128x64:s1:r0", "wgrad:tap128x128:s1:r0",
        "wgrad:tap64x64:s2:r2", "wgrad:tap64x64:s3:r2", "wgrad:tap64x64:s5:r4", "wgrad:tap64x64:s8:r8",
        "wgrad:tap64x64:s10:r8", "wgrad:tap64x64:s14:r8", "wgrad:tap64x64:s40:r16",
        "wgrad:tap128x128:s2:r1", "wgrad:tap128x128:s10:r1u"),
    "wgrad_w3": (
        "wgrad:w3:s1:r0", "wgrad:w3:s2:r2", "wgrad:w3:s4:r4", "wgrad:w3:s10:r8",
        "wgrad:tap64x64:s2:r2", "wgrad:tap64x64:s3:r2"),     # the last two: the fall-through to the per-tap kernel
}


def _run_group(name, monkeypatch):
    """Every case of the group on the guarded buffers under its own DTFE_IG_* knobs (monkeypatch restores the
    environment), then ``check``: guards intact, nothing unwritten, bit equality with the oracle."""
    import torch

    cases = gc.GROUPS[name]()
    seen = set()
    for c in cases:
        b = gc.build(c)
        ref = gc.oracle(b)[0]
        seen.add(gc.path(c))
        gc.apply_env(monkeypatch, c)
        got = gc.run(b, DEV)
        torch.cuda.synchronize()
        gc.check(b, got, ref)
    assert seen == set(PATHS[name]), (name, seen ^ set(PATHS[name]))
    print("%s: %d cases bit-equal" % (name, len(cases)))


def test_forward(monkeypatch):
    """The geometry set on auto and on every tile, BatchNorm statistics fused and (split-K) by the separate pass,
    split-K on auto (8), forced uneven (3 over 10 k-tiles) and clipped, ``rounded`` split and unsplit, and the
    statistics fold with 2 and with 33 chunks."""
    _run_group("fwd", monkeypatch)


def test_dgrad(monkeypatch):
    """The geometry set with and without ``accumulate`` (stride-2 phases: zero-tap phases write zeros over NaN,
    or are dropped and leave the old values), the four tiles, split-K accumulation (forced and auto, ``rounded``:
    RNE(S + old) against the unsplit RNE(RNE(S) + old)) and the masked accumulation source unsplit, under
    DTFE_IG_SPLIT=2 and at shapes the automatic split would take."""
    _run_group("dgrad", monkeypatch)


def test_dgrad_stats(monkeypatch):
    """BN-backward statistics: fused on unequal stride-2 phase grids (absent tiles) on every tile, with
    ``accumulate``, act none / ReLU from x / ReLU from y, with zero-tap phases; the separate pass for one phase."""
    _run_group("dgrad_stats", monkeypatch)


def test_wgrad_tap(monkeypatch):
    """The per-tap kernel's four instantiations, M no multiple of 32 or 64, stride 2 / pad 0 / non-square kernels,
    and the m-split sweep through reduce S = 1, 2, 4, 8, 16 and its unrolled loop."""
    _run_group("wgrad_tap", monkeypatch)


def test_wgrad_w3(monkeypatch):
    """The all-taps kernel at W = 2 .. 62 (W = 62 fills the 192-pixel patch), splits 1 / auto / clipped, and the
    fall-through to the per-tap kernel at W = 63 and at pad 0."""
    _run_group("wgrad_w3", monkeypatch)
