"""The whole-image LDS convolution kernels (ops.imgconv, ops.imgconv_shortcut, ops.imgwgrad) bit for bit
against an exact float64 oracle, inside NaN-guarded buffers.

Cases, guards, oracle and ``check`` live in tests/imgconv_cases.py (its docstring states the two data
regimes, ``unit`` and ``wide``, on which the kernels have to be exact); tests/test_imgconv_oracle_cpu.py
proves on the CPU that the data conditions hold, that the project's fp32 reference path agrees with the
oracle, and that ``check`` catches nine kinds of wrong kernel in every case.  Every comparison below is
``torch.equal``; there is no tolerance to tune.

Which kernel a case reaches
---------------------------
Forward / data gradient, launch_imgconv (imgconv.hip):

  CS <= 4  B >= 256, 28x28x1 -> 32, 5x5 pad 2, pool, act none / ReLU   conv1c_fwd_kernel (launch_conv1_copies_fwd,
                                                                        grid min(B, 1024): B = 1030 is the smallest
                                                                        batch with a second image per workgroup)
           otherwise: launch_nt<NT>, NT = 1, 2, 4 for N <= 16, 32, 64   imgconv1_kernel<NT, 4, STAGE>; STAGE (16-B
                                                                        stores from LDS) = no pool, no mask, N % 8 == 0
  CS > 4   B < 64, or a pooled source with odd S                       imgconv_kernel<NT, 4> (launch_nt)
           B >= 256, O = 14, 5x5, stride 1 (launch_imgconv_persistent -> launch_fixed):
             CS 32, N 64, ReLU, plain source, pool                      imgconv_fixed_kernel<32,5,5,20,48,...> "fixed:fwd"
             CS 64, N 32, act none, pooled source, no pool              imgconv_fixed_kernel<64,5,5,20,80,...> "fixed:dgrad"
           B >= 64: launch_cfg<NT,RT,WM,WN> = N <= 16: <1,2,16,1>; N <= 32: <1,2,8,2>; else O*O <= 64 and a plain
             source: <2,1,4,2>; else <2,2,8,2>.  Threads = 64 * WM * WN; npf = ceil(source 16-B chunks / threads)
             (chunks = S*S*CS/8, a pooled source (S/2)^2*CS/8) picks the prefetch instance NPF = 1..4.  The k walk is
             closed-form (":csc") for a plain source, 3x3, CS in {16, 32, 64} and npf <= 2, else the runtime walk
             (":rt"); a pooled source takes the POOLED instance (":unpool").  The epilogue is "pool" (blocked rows),
             "staged" (stage_out: no pool, N % 8 == 0, OW a power of two; it applies relu_mask from 16-B loads at
             store time and is the only one that adds the shortcut gradient) or "direct".  stage_out also needs
             persist_lds + O*O*N*2 <= 160 KB, where persist_lds = (NTOT * KP weights + LH * LWP * PS image + slack) * 2
             follows the (PS, LWP) layout that persist_geom's conflict search picks (mirrored step for step in
             imgconv_cases._persist_layout; it reproduces launch_fixed's constants (20, 48) and (20, 80)): the
             last two columns.  slack = the image's zero tail, K*K*CS % 32 != 0.
           B >= 64 but persist_lds > 160 KB (28x28x32 5x5 N 64: 64 * 816 weights + 32*32*32 image = 170 KB)
                                                                        launch_cfg returns false -> imgconv_kernel<4, 4>

  case (B: S x S x CS -> N, K, features)                 kernel                  npf  epilogue  slack  (PS, LWP)  lds + stage B
  64, 259: 32x32x16 -> 16 3x3 (+bias, ReLU)              cfg<1,2,16,1>:csc       2    staged    yes    (16, 36)    46080 + 32768
  64: 16x16x16 -> 16 3x3                                 cfg<1,2,16,1>:csc       1    staged    yes    (16, 20)    17920 +  8192
  64: 14x14x8 -> 16 5x5 (+bias, ReLU)                    cfg<1,2,16,1>:rt        1    direct    yes    (16, 20)    OW = 14
  259: 14x14x32 -> 16 5x5 pool                           cfg<1,2,16,1>:rt        1    pool      no     (48, 20)
  64, 259: 16x16x32 -> 32 3x3                            cfg<1,2,8,2>:csc        1    staged    no     (48, 20)    54016 + 16384
  64: 16x16x24 -> 32 3x3                                 cfg<1,2,8,2>:rt         1    staged    yes    (48, 20)    52224 + 16384
  64: 28x28x32 -> 32 3x3 (fwd ReLU; dgrad + mask)        cfg<1,2,8,2>:rt         4    direct    no     (48, 36)    OW = 28
  259: 24x24x32 -> 32 3x3                                cfg<1,2,8,2>:rt         3    direct    no     (48, 28)    OW = 24
  64: 14x14x32 -> 32 5x5 pool                            cfg<1,2,8,2>:rt         1    pool      no     (48, 20)
  64: 32x32x16 -> 32 3x3 stride 2                        cfg<1,2,8,2>:csc        2    staged    yes    (24, 36)    70208 + 16384
  64, 259: 8x8x64 -> 64 3x3                              cfg<2,1,4,2>:csc        1    staged    no     (80, 12)    94976 +  8192
  64: 8x8x8 -> 64 3x3                                    cfg<2,1,4,2>:rt         1    staged    yes    (16, 12)    18688 +  8192
  259: 16x16x32 -> 64 3x3 stride 2 (O = 8)               cfg<2,1,4,2>:csc        2    staged    no     (40, 20)    66112 +  8192
  64, 259: 16x16x64 -> 64 3x3                            cfg<2,2,8,2>:csc        2    direct    no     (80, 20)   133376 + 32768 > 163840
  64, 259: 16x16x32 -> 64 3x3                            cfg<2,2,8,2>:csc        1    staged    no     (48, 20)    73472 + 32768
  259: 16x16x32 -> 64 5x5                                cfg<2,2,8,2>:rt         1    direct    no     (48, 20)   142848 + 32768 > 163840
  64: 14x14x32 -> 64 5x5 pool                            cfg<2,2,8,2>:rt         1    pool      no     (48, 20)
  dgrad 64: 32x32x16 -> 16 3x3 mask / shortcut s 1       cfg<1,2,16,1>:csc       2    staged    yes    (16, 36)    46080 + 32768
  dgrad 259: 16x16x32 -> 32 3x3 mask / shortcut s 1      cfg<1,2,8,2>:csc        1    staged    no     (48, 20)    54016 + 16384
  dgrad 64: 8x8x64 -> 64 3x3 mask                        cfg<2,1,4,2>:csc        1    staged    no     (80, 12)    94976 +  8192
  dgrad 64: pooled 7x7x64 -> 14x14x32 5x5 mask           cfg<1,2,8,2>:unpool     1    direct    no     (80, 20)    OW = 14
  dgrad 259: pooled 7x7x16 -> 14x14x16 5x5               cfg<1,2,16,1>:unpool    1    direct    yes    (16, 20)    OW = 14
  dgrad 64: pooled 8x8x32 -> 16x16x64 3x3 mask           cfg<2,2,8,2>:unpool     1    staged    no     (48, 20)    73472 + 32768
  dgrad 96, 64: 16x16x32 dil 2 -> 32x32x16 (/ sc s 2)    cfg<1,2,16,1>:csc       1    staged    no     (48, 36)   127232 + 32768
  dgrad 259: 8x8x64 dil 2 -> 16x16x32 (mask / sc s 2)    cfg<1,2,8,2>:csc        1    staged    no     (80, 20)    95488 + 16384

  So <2,2,8,2> runs its staged epilogue only with the csc npf 1 instance (B = 64 and 259) and the un-pool
  instance; its csc npf 2 and runtime-walk instances exceed the LDS limit with every shape used here.

Weight gradient, launch_imgwgrad (imgconv.hip, imgwgrad_persist.hip):

  CS <= 4  B >= 256, 28x28x1 -> 32 5x5 pad 2, dy_pooled                 conv1c_wgrad_kernel + partials_reduce_kernel (grid
                                                                        min(B, 320): B = 330 gives ten workgroups two images)
           otherwise                                                    imgwgrad1_kernel<NC>, NC = 1, 2, 4 (N <= 16, 32, 64)
  CS > 4   CS % 16 == 0, N % 8 == 0, B >= 128 (launch_imgwgrad_persistent), ctiles = K*K*CS/16 column tiles:
             no db, plain dY: ctiles <= 9 and N <= 16: wp<1,9,KG8>; ctiles <= 9, N <= 32: wp<2,9,KG8>;
               ctiles <= 18, N <= 32: wp<2,9,KG4>; N > 32, ctiles <= 40: wp<4,5>
             otherwise (db, or dY pooled = ":unpool"): N > 32 and ceil(ctiles/8) <= 7: wp<4,7>; N <= 32 and <= 8: wp<2,8>
             each imgwgrad_persist_kernel<MT,CTW,NPFS,NPFD,..>: NPFS / NPFD = 1, 2, 4 from npfs = ceil(S*S*CS/8 / 512),
             npfd = ceil(dY chunks / 512) rounded up to 1, 2, 4; grid = min(B, max_blocks or 256, ceil(B / ipw)),
             ipw = ceil(256 (KG > 1: 512) / (O*O)); + wp_reduce_kernel over the workspace
           otherwise (B < 128, CS = 8, 24)                              imgwgrad_kernel<1,8>, <2,6>, <4,4> (N <= 16, 32, 64),
                                                                        4 images per block at these B: B = 5 is 4 + 1

  case (B: S x S x CS -> N, features)                    kernel                  (npfs, npfd)
  128, 130: 16x16x16 -> 16                               wp<1,9,KG8>             (1, 1)    ipw 2: grid 64 / 65
  128: 32x32x16 -> 16                                    wp<1,9,KG8>             (4, 4)    ipw 1
  128, 130 (+ own workspace): 16x16x16 -> 32             wp<2,9,KG8>             (1, 2)
  130: 32x32x16 -> 32 stride 2                           wp<2,9,KG8>             (4, 2)
  128, 130 (+ max_blocks 64): 16x16x32 -> 32             wp<2,9,KG4>             (2, 2)
  128, 130, 300: 8x8x64 -> 64                            wp<4,5>                 (1, 1)    ipw 4: grid 32 / 33 / 75
  128, 130: 16x16x32 -> 64                               wp<4,5>                 (2, 4)
  130: 16x16x16 -> 32 + db                               wp<2,8>                 (1, 2)
  130: 32x32x16 -> 16 + db, own workspace                wp<2,8>                 (4, 4)
  130: 16x16x32 -> 32 + db, own workspace, deferred      wp<2,8>                 (2, 2)
  128: 16x16x16 -> 32 + db, dy_pooled                    wp<2,8>:unpool          (1, 1)
  130: 8x8x64 -> 64 + db                                 wp<4,7>                 (1, 1)
  259: 14x14x32 -> 64 5x5 + db, dy_pooled (MNIST conv2)  wp<4,7>:unpool          (2, 1)

CONV_TABLE / WGRAD_TABLE below are these rows; the CPU test checks them against imgconv_cases' mirror of
the dispatch conditions and that every persistent case is a row.

Measured on an MI355X
---------------------
At commit 7d0a60a (the parent of the commit that added this file), cases (both regimes counted) and wall
time of each test's call; the time is the host's float64 oracle and the copies, the launches are microseconds.
Every case was bit-equal, with untouched guards, the first time it ran: no kernel had to be fixed.

    test_per_image_kernel                    22 cases   0.29 s
    test_persistent_cfg[fwd-1]               10         0.80 s
    test_persistent_cfg[fwd-2]               14         0.98 s
    test_persistent_cfg[fwd-4]               20         1.77 s
    test_persistent_cfg[dgrad-None]          26         1.60 s
    test_lds_fall_through_to_per_image        2         0.41 s
    test_fixed_geometry[fwd]                  4         0.90 s
    test_fixed_geometry[dgrad]                4         0.56 s
    test_few_channel_forward[img1-None]      14         0.12 s
    test_few_channel_forward[conv1c-unit]     3         1.16 s
    test_few_channel_forward[conv1c-wide]     3         1.17 s
    test_wgrad_per_image                      8         0.05 s
    test_wgrad_few_channel                    7         0.14 s
    test_wgrad_persistent[kgroups]           15         0.44 s   (each launch twice)
    test_wgrad_persistent[db]                 5         0.20 s   (each launch twice)
    test_wgrad_deferred_grouped_flush         3         0.05 s
"""
import os
import sys

import pytest
import torch

from dtfe import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgconv_cases as ic  # noqa: E402
from imgconv_cases import ConvCase as C, WgradCase as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = ops.ACT_RELU

# (case in the ``unit`` regime, kernel, npf, epilogue): the forward / data-gradient table above; LAYOUTS
# below holds its (PS, LWP) and LDS columns
CONV_TABLE = [
    (C(B=B, S=32, CS=16, N=16, K=3, pad=1, bias=True, act=R), "cfg<1,2,16,1>:csc", 2, "staged") for B in (64, 259)] + [
    (C(B=64, S=16, CS=16, N=16, K=3, pad=1), "cfg<1,2,16,1>:csc", 1, "staged"),
    (C(B=64, S=14, CS=8, N=16, K=5, pad=2, bias=True, act=R), "cfg<1,2,16,1>:rt", 1, "direct"),
    (C(B=259, S=14, CS=32, N=16, K=5, pad=2, pool=True, act=R, bias=True), "cfg<1,2,16,1>:rt", 1, "pool"),
    (C(B=64, S=16, CS=32, N=32, K=3, pad=1), "cfg<1,2,8,2>:csc", 1, "staged"),
    (C(B=259, S=16, CS=32, N=32, K=3, pad=1), "cfg<1,2,8,2>:csc", 1, "staged"),
    (C(B=64, S=16, CS=24, N=32, K=3, pad=1), "cfg<1,2,8,2>:rt", 1, "staged"),
    (C(B=64, S=28, CS=32, N=32, K=3, pad=1, act=R), "cfg<1,2,8,2>:rt", 4, "direct"),
    (C(B=259, S=24, CS=32, N=32, K=3, pad=1, bias=True), "cfg<1,2,8,2>:rt", 3, "direct"),
    (C(B=64, S=14, CS=32, N=32, K=5, pad=2, pool=True, act=R, bias=True), "cfg<1,2,8,2>:rt", 1, "pool"),
    (C(B=64, S=32, CS=16, N=32, K=3, stride=2, pad=1), "cfg<1,2,8,2>:csc", 2, "staged"),
    (C(B=64, S=8, CS=64, N=64, K=3, pad=1, bias=True), "cfg<2,1,4,2>:csc", 1, "staged"),
    (C(B=259, S=8, CS=64, N=64, K=3, pad=1, bias=True), "cfg<2,1,4,2>:csc", 1, "staged"),
    (C(B=64, S=8, CS=8, N=64, K=3, pad=1), "cfg<2,1,4,2>:rt", 1, "staged"),
    (C(B=259, S=16, CS=32, N=64, K=3, stride=2, pad=1, bias=True), "cfg<2,1,4,2>:csc", 2, "staged"),
    (C(B=64, S=16, CS=64, N=64, K=3, pad=1, act=R), "cfg<2,2,8,2>:csc", 2, "direct"),
    (C(B=259, S=16, CS=64, N=64, K=3, pad=1, act=R), "cfg<2,2,8,2>:csc", 2, "direct"),
    (C(B=64, S=16, CS=32, N=64, K=3, pad=1), "cfg<2,2,8,2>:csc", 1, "staged"),
    (C(B=259, S=16, CS=32, N=64, K=3, pad=1), "cfg<2,2,8,2>:csc", 1, "staged"),
    (C(B=259, S=16, CS=32, N=64, K=5, pad=2, bias=True, act=R), "cfg<2,2,8,2>:rt", 1, "direct"),
    (C(B=64, S=14, CS=32, N=64, K=5, pad=2, pool=True, act=R, bias=True), "cfg<2,2,8,2>:rt", 1, "pool"),
    (C(B=64, S=32, CS=16, N=16, K=3, pad=1, flip=True, mask=True), "cfg<1,2,16,1>:csc", 2, "staged"),
    (C(B=259, S=16, CS=32, N=32, K=3, pad=1, flip=True, mask=True), "cfg<1,2,8,2>:csc", 1, "staged"),
    (C(B=64, S=8, CS=64, N=64, K=3, pad=1, flip=True, mask=True), "cfg<2,1,4,2>:csc", 1, "staged"),
    (C(B=64, S=28, CS=32, N=32, K=3, pad=1, flip=True, mask=True), "cfg<1,2,8,2>:rt", 4, "direct"),
    (C(B=64, S=14, CS=64, N=32, K=5, pad=2, flip=True, mask=True, src="pooled"), "cfg<1,2,8,2>:unpool", 1, "direct"),
    (C(B=259, S=14, CS=16, N=16, K=5, pad=2, flip=True, src="pooled"), "cfg<1,2,16,1>:unpool", 1, "direct"),
    (C(B=64, S=16, CS=32, N=64, K=3, pad=1, flip=True, mask=True, src="pooled"), "cfg<2,2,8,2>:unpool", 1, "staged"),
    (C(B=96, S=16, CS=32, N=16, K=3, pad=1, flip=True, dil=2), "cfg<1,2,16,1>:csc", 1, "staged"),
    (C(B=259, S=8, CS=64, N=32, K=3, pad=1, flip=True, dil=2, mask=True), "cfg<1,2,8,2>:csc", 1, "staged"),
    (C(B=64, S=32, CS=16, N=16, K=3, pad=1, flip=True, sc=1, sc_C=16), "cfg<1,2,16,1>:csc", 2, "staged"),
    (C(B=259, S=16, CS=32, N=32, K=3, pad=1, flip=True, sc=1, sc_C=32), "cfg<1,2,8,2>:csc", 1, "staged"),
    (C(B=64, S=16, CS=32, N=16, K=3, pad=1, flip=True, dil=2, sc=2, sc_C=32), "cfg<1,2,16,1>:csc", 1, "staged"),
    (C(B=259, S=8, CS=64, N=32, K=3, pad=1, flip=True, dil=2, sc=2, sc_C=64), "cfg<1,2,8,2>:csc", 1, "staged"),
    (C(B=64, S=28, CS=32, N=64, K=5, pad=2, pool=True, act=R, bias=True), "img<4>:lds", 0, ""),
    (C(B=256, S=14, CS=32, N=64, K=5, pad=2, pool=True, act=R, bias=True), "fixed:fwd", 0, ""),
    (C(B=259, S=14, CS=64, N=32, K=5, pad=2, flip=True, mask=True, src="pooled"), "fixed:dgrad", 0, ""),
]

# (O, CS, stride, K, NTOT = WN * NT * 16) -> (PS, LWP, persist_lds bytes): the layout columns of the table above
LAYOUTS = {
    (32, 16, 1, 3, 16): (16, 36, 46080), (16, 16, 1, 3, 16): (16, 20, 17920), (14, 8, 1, 5, 16): (16, 20, 19968),
    (14, 32, 1, 5, 16): (48, 20, 60672), (16, 32, 1, 3, 32): (48, 20, 54016), (16, 24, 1, 3, 32): (48, 20, 52224),
    (28, 32, 1, 3, 32): (48, 36, 123136), (24, 32, 1, 3, 32): (48, 28, 89344), (14, 32, 1, 5, 32): (48, 20, 86784),
    (16, 16, 2, 3, 32): (24, 36, 70208), (8, 64, 1, 3, 64): (80, 12, 94976), (8, 8, 1, 3, 64): (16, 12, 18688),
    (8, 32, 2, 3, 64): (40, 20, 66112), (16, 64, 1, 3, 64): (80, 20, 133376), (16, 32, 1, 3, 64): (48, 20, 73472),
    (16, 32, 1, 5, 64): (48, 20, 142848), (14, 32, 1, 5, 64): (48, 20, 139008), (14, 64, 1, 5, 32): (80, 20, 161024),
    (14, 16, 1, 5, 16): (16, 20, 26112), (32, 32, 1, 3, 16): (48, 36, 127232), (16, 64, 1, 3, 32): (80, 20, 95488),
}

# (case, kernel, (npfs, npfd)): the weight-gradient table above
_W3 = dict(K=3, pad=1)
WGRAD_TABLE = [
    (W(B=B, S=16, CS=16, N=16, db=False, **_W3), "wp<1,9,KG8>", (1, 1)) for B in (128, 130)] + [
    (W(B=B, S=16, CS=16, N=32, db=False, **_W3), "wp<2,9,KG8>", (1, 2)) for B in (128, 130)] + [
    (W(B=B, S=16, CS=32, N=32, db=False, **_W3), "wp<2,9,KG4>", (2, 2)) for B in (128, 130)] + [
    (W(B=B, S=8, CS=64, N=64, db=False, **_W3), "wp<4,5>", (1, 1)) for B in (128, 130, 300)] + [
    (W(B=B, S=16, CS=32, N=64, db=False, **_W3), "wp<4,5>", (2, 4)) for B in (128, 130)] + [
    (W(B=128, S=32, CS=16, N=16, db=False, **_W3), "wp<1,9,KG8>", (4, 4)),
    (W(B=130, S=32, CS=16, N=32, stride=2, db=False, **_W3), "wp<2,9,KG8>", (4, 2)),
    (W(B=130, S=16, CS=32, N=32, db=False, max_blocks=64, **_W3), "wp<2,9,KG4>", (2, 2)),
    (W(B=130, S=16, CS=16, N=32, db=False, ws="own", **_W3), "wp<2,9,KG8>", (1, 2)),
    (W(B=130, S=16, CS=16, N=32, **_W3), "wp<2,8>", (1, 2)),
    (W(B=128, S=16, CS=16, N=32, pooled=True, **_W3), "wp<2,8>:unpool", (1, 1)),
    (W(B=130, S=8, CS=64, N=64, **_W3), "wp<4,7>", (1, 1)),
    (W(B=259, S=14, CS=32, N=64, K=5, pad=2, pooled=True), "wp<4,7>:unpool", (2, 1)),
    (W(B=130, S=32, CS=16, N=16, ws="own", **_W3), "wp<2,8>", (4, 4)),
    (W(B=130, S=16, CS=16, N=16, db=False, ws="own", **_W3), "wp<1,9,KG8>", (1, 1)),
    (W(B=128, S=8, CS=64, N=64, db=False, ws="own", **_W3), "wp<4,5>", (1, 1)),
    (W(B=130, S=16, CS=32, N=32, ws="own", **_W3), "wp<2,8>", (2, 2)),
]


def _own_workspace(c):
    """A NaN-filled workspace of the case's own: a partial read before it is written poisons dW."""
    return torch.full((ops.wgrad_ws_floats(c.N, c.K * c.K * c.CS),), float("nan"), device=DEV)


def _run_all(name, cases, want_paths):
    """Every case through run(case, "cuda") and check.  A persistent weight gradient runs twice on the same
    workspace: the second launch meets the first one's partials."""
    seen = set()
    for c in cases:
        b = ic.build(c)
        ref = ic.oracle(b)[0]
        p = ic.path(c)
        seen.add(p)
        ws = _own_workspace(c) if c.kind == "wgrad" and c.ws == "own" else None
        for _ in range(2 if p.startswith("wp") else 1):
            got = ic.run(b, DEV, workspace=ws)
            ic.check(b, got, ref)
            if c.kind == "conv" and c.sc:   # staged epilogue: the launch itself adds the shortcut gradient
                assert got["sc_done"] is True, c
    assert seen == set(want_paths), (name, seen ^ set(want_paths))
    print("%s: %d cases bit-equal" % (name, len(cases)))


def test_per_image_kernel():
    """B in {1, 3}: imgconv_kernel<NT> for N = 16, 24, 32, 64; pool + argmax + bias + ReLU, stride 2, valid
    padding, an odd map, the data-gradient form with relu_mask and with an un-pooled source."""
    _run_all("per-image", ic.per_image_cases(), ("img<1>", "img<2>", "img<4>"))


@pytest.mark.parametrize("half,nt", [("fwd", 1), ("fwd", 2), ("fwd", 4), ("dgrad", None)])
def test_persistent_cfg(half, nt):
    """launch_cfg at B = 64 and 259 (forward by N class: 1, 2, 4 n-tiles): the four wave grids, closed-form
    and runtime k walks, npf 1-4, staged / direct / pooled epilogues; data gradient: relu_mask with the
    special values, un-pool on load, dil = 2, the fused shortcut gradient (stride 1 and 2, wider than N)."""
    want = {p for c, p, _, _ in CONV_TABLE if p.startswith("cfg") and c.flip == (half == "dgrad") and
            nt in (None, ic._nt(c.N))}
    _run_all("persistent %s %s" % (half, nt or ""), ic.persistent_cases(half, nt), want)


def test_lds_fall_through_to_per_image():
    _run_all("LDS fall-through", ic.lds_fallthrough_cases(), ("img<4>:lds",))


@pytest.mark.parametrize("half", ["fwd", "dgrad"])
def test_fixed_geometry(half):
    """MNIST conv2 forward / data gradient at B = 256 and 259 (imgconv_fixed_kernel)."""
    _run_all("fixed %s" % half, ic.fixed_cases(half), ("fixed:%s" % half,))


@pytest.mark.parametrize("which,regime", [("img1", None), ("conv1c", "unit"), ("conv1c", "wide")])
def test_few_channel_forward(which, regime):
    """CS = 1, 2, 3: imgconv1_kernel staged and direct, stride 2, B in {2, 70}; conv1c_fwd at B = 256, 1030
    (26 M pre-pool values at B = 1030: one regime per test)."""
    _run_all("few-channel %s %s" % (which, regime or ""), ic.few_channel_cases(which, regime),
             [p for p in ic.CONV_PATHS if p.startswith(which)])


def test_wgrad_per_image():
    _run_all("wgrad per-image", ic.wgrad_per_image_cases(), ("wg<1,8>", "wg<2,6>", "wg<4,4>"))


def test_wgrad_few_channel():
    _run_all("wgrad few-channel", ic.wgrad_few_channel_cases(), ("wg1<1>", "wg1<2>", "wg1<4>", "conv1c_wgrad"))


@pytest.mark.parametrize("kind", ["kgroups", "db"])
def test_wgrad_persistent(kind):
    """B = 128, 130 (and 300: the ipw cap): the k-group configs without db, <2,8> / <4,7> with db (plain and
    dy_pooled); max_blocks = 64; an own NaN-filled workspace; every launch twice on the same workspace."""
    want = ("wp<1,9,KG8>", "wp<2,9,KG8>", "wp<2,9,KG4>", "wp<4,5>") if kind == "kgroups" else (
        "wp<2,8>", "wp<2,8>:unpool", "wp<4,7>", "wp<4,7>:unpool")
    _run_all("wgrad persistent %s" % kind, ic.wgrad_persistent_cases(kind), want)


def test_wgrad_deferred_grouped_flush():
    """Three launches with own NaN-filled workspaces leave their reduces to a collector; dW / db hold their
    old values until ONE grouped flush sums them; then each equals the oracle."""
    cases = ic.wgrad_deferred_cases()
    reduces = ops.WgradReduces()
    pending = []
    for c in cases:
        b = ic.build(c)
        ws = _own_workspace(c)
        pending.append((b, ic.launch(b, DEV, workspace=ws, defer=reduces), ws))
    assert len(reduces) == len(cases)
    for b, t, _ in pending:   # nothing summed yet
        for name in b.outputs:
            assert torch.equal(t[name].cpu(), b.bufs[name]), (b.case, name)
    assert reduces.flush() == len(cases)
    torch.cuda.synchronize()
    for b, t, _ in pending:
        ic.check(b, ic.fetch(t))
    assert reduces.flush() == 0
    print("wgrad deferred: %d cases bit-equal" % len(cases))
