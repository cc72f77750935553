"""Cases, guarded buffers and an exact float64 oracle for the whole-image LDS convolution family
(``ops.imgconv``, ``ops.imgconv_shortcut``, ``ops.imgwgrad``).

Shared by tests/test_imgconv_paths_gpu.py (the kernels) and tests/test_imgconv_oracle_cpu.py (the
oracle itself: its data conditions, agreement with the project's fp32 CPU reference path, sensitivity
to wrong kernels, and coverage of the dispatch paths).

Data: every operand is a small non-zero signed integer.  The kernels multiply bf16 operands and
accumulate in fp32, so every product and every partial sum, in any order, is an integer far below
2^24: the accumulation is exact whatever the tiling, split or atomic order, the expected output is
one bit pattern, and ``check`` compares with ``torch.equal``.  No tolerance appears anywhere.

  unit   magnitudes from the first rung of ((x 1..2, w 1..2), (x 1..2, w 1), (x 1, w 1)) at which every
         reference value - pre-activation, after the bias, after the shortcut add - is an integer of
         magnitude <= 256, hence exact in bf16.  Every term is non-zero: a dropped, doubled or misplaced
         term changes some output.  Weight gradients (fp32 outputs) have no cap: they use (1..2, 1..2).
  wide   (bf16 outputs only) magnitudes 1..h, h the first of 7, 15, 31 at which the values the kernel
         has to round contain exact ties that round-to-nearest-even rounds up in magnitude and ties it
         rounds down; the expected output is RNE_bf16 of the exact value.  This regime sees a
         truncating or round-half-away conversion, or an accumulation held in bf16.

  In both, (number of terms) * max|x| * max|w| + max|bias| < 2^24 bounds every partial sum.

Guards: every input is a view into a larger flat buffer with GUARD elements of NaN (0xFF for argmax
bytes) on both sides; every output a view into a buffer whose guards hold SENT (0xFF).  y is pre-filled
with NaN, the argmax with 0xFF, dw / db with non-zero integers that the oracle adds (the op is +=).
GUARD elements are a multiple of 16 bytes in every dtype, so the views keep the kernels' alignment.

The oracle is a loop over taps, one tensordot per (kh, kw) over the padded source, written from the
definitions in the docstrings of ops.imgconv / ops.imgwgrad; it shares no code with the project's CPU
reference path (conv2d / conv2d_weight).
"""
import dataclasses
import functools
import zlib

import numpy as np
import torch

from dtfe import ops

GUARD = 64              # elements around every buffer: 64 B of uint8, 128 B of bf16, 256 B of fp32
SENT = -512.0           # exact in bf16 and fp32, far outside every result that is compared
UNIT_CAP = 256
UNIT_LADDER = ((2, 2), (2, 1), (1, 1))   # (max|x|, max|w|)
WIDE_LADDER = (7, 15, 31)
MASK_SPECIALS = (0.0, -0.0, -3.0, float("nan"), float("inf"), float("-inf"))   # only +inf keeps


# --------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class ConvCase:
    """ops.imgconv / ops.imgconv_shortcut over a square S x S x CS source (``src`` "pooled": S is the
    un-pooled side, the source arrives as (src_pooled, src_argmax))."""
    B: int
    S: int
    CS: int
    N: int
    K: int
    stride: int = 1
    pad: int = 0
    flip: bool = False
    pool: bool = False
    act: int = 0
    bias: bool = False
    src: str = "plain"         # "plain" | "pooled"
    mask: bool = False         # relu_mask, the special values included
    dil: int = 1
    sc: int = 0                # 0: ops.imgconv; s > 0: ops.imgconv_shortcut with sc_stride = s
    sc_C: int = 0              # channels of the shortcut gradient (>= N)
    regime: str = "unit"

    kind = "conv"

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())

    @property
    def O(self):               # output side before the pool
        return (self.S * self.dil + 2 * self.pad - self.K) // self.stride + 1

    @property
    def terms(self):
        return self.K * self.K * self.CS


@dataclasses.dataclass(frozen=True)
class WgradCase:
    """ops.imgwgrad: dW [N][K][K][CS] and db [N] of a conv over a square S x S x CS source."""
    B: int
    S: int
    CS: int
    N: int
    K: int
    stride: int = 1
    pad: int = 0
    pooled: bool = False       # dY un-pooled from (dy_pooled, dy_argmax)
    db: bool = True
    ws: str = "default"        # "default" | "own": the test passes a NaN-filled workspace of its own
    max_blocks: int = 0
    scale: float = 0.5
    regime: str = "unit"

    kind = "wgrad"

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())

    @property
    def O(self):
        return (self.S + 2 * self.pad - self.K) // self.stride + 1

    @property
    def terms(self):
        return self.B * self.O * self.O


# ------------------------------------------------------------ dispatch, mirrored (top level only)
def _nt(N):
    return 1 if N <= 16 else (2 if N <= 32 else 4)


def _mnist_conv1(c):
    return c.B >= 256 and c.S == 28 and c.CS == 1 and c.N == 32 and c.K == 5 and c.stride == 1 and c.pad == 2


def conv_supported(c):
    """imgconv_supported (csrc/kernels/imgconv.hip)."""
    OH = (c.S + 2 * c.pad - c.K) // c.stride + 1
    L = (OH - 1) * c.stride + c.K
    if c.CS <= 4:
        return c.K * c.K * c.CS <= 32 and c.N <= 64 and L * L * c.CS * 2 <= 150 * 1024
    return c.CS % 8 == 0 and c.N <= 64 and L * L * c.CS * 2 <= 150 * 1024


def persist_npf(c, threads):
    """persist_geom's npf: 16-B source chunks per thread."""
    px = (c.S // 2) ** 2 if c.src == "pooled" else c.S * c.S
    return (px * (c.CS // 8) + threads - 1) // threads


_LANE_GROUPS = ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27),
                (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31),
                (32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59),
                (36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63))


def _row_pixel(m, O, blocked):
    """row_pixel (imgconv_persist.hip): output row m of an image -> (oy, ox); (0, 0) for a padding row."""
    if blocked:
        t, quad, q = m >> 4, (m >> 2) & 3, m & 3
        w = t * 4 + (0, 2, 3, 1)[quad]
        if w >= (O >> 1) * (O >> 1):
            return 0, 0
        return 2 * (w // (O >> 1)) + (q >> 1), 2 * (w % (O >> 1)) + (q & 1)
    return (m // O, m % O) if m < O * O else (0, 0)


@functools.lru_cache(maxsize=None)
def _persist_layout(O, CS, stride, K, ntot):
    """persist_geom's image layout search (imgconv_persist.hip), step for step: the (PS, LWP) with the
    fewest modelled A-read conflicts (a_read_conflicts) within 160 KB, ties to the smaller layout, and
    persist_lds of it in bytes.  No layout fits: (CS, LW) and an LDS need above the limit."""
    L = (O - 1) * stride + K
    terms = K * K * CS
    img_off = ntot * ((terms + 31) // 32 * 32 + 16)
    blocked = O & 1 == 0
    tiles = (O * O + 15) // 16
    pix = [[_row_pixel(t * 16 + (lane & 15), O, blocked) for lane in range(64)] for t in range(tiles)]
    best, pick = 1e30, (CS, L)
    for pss in range(CS // 8, CS // 8 + 8):
        for lwp in range(L, L + 12):
            slack = (lwp + 4) * pss * 8 if terms % 32 else 0
            nbytes = (img_off + L * lwp * pss * 8 + slack) * 2
            if nbytes > 160 * 1024:
                continue
            total = 0
            for t in range(tiles):
                slot = [((oy * stride * lwp + ox * stride) * pss + (lane >> 4)) % 16
                        for lane, (oy, ox) in enumerate(pix[t])]
                for group in _LANE_GROUPS:
                    cnt = [0] * 16
                    for lane in group:
                        cnt[slot[lane]] += 1
                    total += max(cnt) - 1
            cost = total / tiles + 1e-7 * nbytes
            if cost < best:
                best, pick = cost, (pss * 8, lwp)
    ps, lwp = pick
    slack = (lwp + 4) * ps if terms % 32 else 0
    return ps, lwp, (img_off + L * lwp * ps + slack) * 2


def persist_layout(c, ntot):
    """(PS, LWP, LDS bytes) of the case under a wave grid of ntot = WN * NT * 16 output channels."""
    return _persist_layout(c.O, c.CS, c.stride, c.K, ntot)


_CFG = {"cfg<1,2,16,1>": (1, 2, 16, 1), "cfg<1,2,8,2>": (1, 2, 8, 2), "cfg<2,1,4,2>": (2, 1, 4, 2),
        "cfg<2,2,8,2>": (2, 2, 8, 2)}


def conv_path(c):
    """The kernel launch_imgconv reaches for the case: conv1c_fwd (imgconv1_copies.hip), img1<NT>
    (imgconv1_kernel, ":staged" = LDS-staged 16-B stores), fixed (imgconv_fixed_kernel), cfg<NT,RT,WM,WN>
    (imgconv_persist_kernel; ":csc" closed-form k walk, ":rt" runtime walk, ":unpool" source un-pooled on
    load) or img<NT> (imgconv_kernel; ":lds" = the persistent kernel's LDS need sent it there).

    The names are derived from the host code's conditions, mirrored here (the layout search included);
    nothing observes which kernel really ran, so a dispatch change that sends a case elsewhere keeps the
    case passing under its old name until this mirror is updated with it.  DTFE_DIAG is taken as unset."""
    O = c.O
    if c.CS <= 4:
        if _mnist_conv1(c) and c.pool and c.act in (ops.ACT_NONE, ops.ACT_RELU) and not c.mask:
            return "conv1c_fwd"
        L = (O - 1) * c.stride + c.K
        staged = (not c.pool and not c.mask and c.N % 8 == 0 and
                  (L * L * c.CS * 2 + 15) // 16 * 16 + O * O * c.N * 2 <= 150 * 1024)
        return "img1<%d>:%s" % (_nt(c.N), "staged" if staged else "direct")
    pooled = c.src == "pooled"
    L = (O - 1) * c.stride + c.K
    if c.B < 64 or (pooled and (c.S & 1 or c.dil > 1 or c.S + c.pad > L)):
        return "img<%d>" % _nt(c.N)
    if O == 14 and c.B >= 256 and c.K == 5 and c.stride == 1 and c.dil == 1:
        # launch_fixed: compile-time layouts (LWP, PS) = (20, 48) / (20, 80), 13 waves of one 16-row tile
        for name, cs, n, act, layout in (("fwd", 32, 64, ops.ACT_RELU, (48, 20)), ("dgrad", 64, 32, ops.ACT_NONE, (80, 20))):
            if (c.CS, c.N, c.act, pooled, c.pool) == (cs, n, act, name == "dgrad", name == "fwd"):
                ps, lwp, lds = persist_layout(c, n)
                stage = 0 if pooled else O * O // 4 * n * 3
                if ((ps, lwp) == layout and c.terms % 32 == 0 and (O * O + 15) // 16 <= 13 and
                        lds + stage <= 160 * 1024 and persist_npf(c, 64 * 13) <= 2):
                    return "fixed:" + name
    if c.N <= 16:
        cfg = (1, 2, 16, 1)
    elif c.N <= 32:
        cfg = (1, 2, 8, 2)
    elif O * O <= 64 and not pooled:
        cfg = (2, 1, 4, 2)
    else:
        cfg = (2, 2, 8, 2)
    NT, _, WM, WN = cfg
    if persist_layout(c, WN * NT * 16)[2] > 160 * 1024:
        return "img<%d>:lds" % _nt(c.N)
    npf = persist_npf(c, 64 * WM * WN)
    assert 1 <= npf <= 4 and not (c.pool and O & 1), c
    if pooled:
        walk = "unpool"
    else:
        walk = "csc" if c.K == 3 and c.CS in (16, 32, 64) and npf <= 2 else "rt"
    return "cfg<%d,%d,%d,%d>:%s" % (cfg + (walk,))


def conv_epilogue(c):
    """How a persistent (launch_cfg) launch of the case stores: "pool" (blocked rows, pooled + argmax),
    "staged" (stage_out: the whole image through LDS, 16-B stores - no pool, N % 8 == 0, OW a power of
    two, and the staging area fits beside the chosen layout: persist_lds + O*O*N*2 <= 160 KB) or "direct"."""
    NT, _, _, WN = _CFG[conv_path(c).split(":")[0]]
    if c.pool:
        return "pool"
    lds = persist_layout(c, WN * NT * 16)[2]
    fits = lds + c.O * c.O * c.N * 2 <= 160 * 1024
    return "staged" if c.N % 8 == 0 and c.O & (c.O - 1) == 0 and fits else "direct"


def wgrad_supported(c):
    """imgwgrad_supported (csrc/kernels/imgconv.hip: wg_geom / wg_lds)."""
    O = c.O
    if c.N > 64 or O > 32:
        return False
    if c.CS <= 4:
        if c.K * c.K * c.CS > 32:
            return False
    elif c.CS % 8:
        return False
    L = (O - 1) * c.stride + c.K
    owp = 8 if c.CS <= 4 else 4
    while owp < O:
        owp <<= 1
    kpad = (O * owp + 31) // 32 * 32
    slack = (((kpad // owp - O + 1) * c.stride + 1) * L + owp * c.stride) * c.CS
    slack = (slack + 7) // 8 * 8
    mt = _nt(c.N)
    if c.CS <= 4:
        lds = ((L * L * c.CS + slack + 7) // 8 * 8 + kpad * mt * 16) * 2 + 33 * mt * 16 * 4
    else:
        lds = (L * L * c.CS + slack + kpad * mt * 16) * 2
    return lds <= 150 * 1024


def _wp_fits(c, MT, CTW, KG):
    """wp_launch's own limits (imgwgrad_persist.hip: wp_geom / wp_lds, the column-tile and LDS checks)."""
    O = c.O
    odd16 = lambda e: 16 * ((e + 15) // 16 | 1)  # noqa: E731
    L = (O - 1) * c.stride + c.K
    ps, nps = odd16(c.CS), odd16(c.N)
    owp = 8 if O <= 8 else (16 if O <= 16 else 32)
    per = 32 // owp
    rows = (O + per - 1) // per * per
    slack = ((rows - O + 1) * c.stride * L + owp * c.stride + 8) * ps
    lds = ((L * L * ps + slack + 7) // 8 * 8 + rows * owp * nps) * 2
    ctiles = c.K * c.K * c.CS // 16
    red = (KG - 1) * (8 // KG) * CTW * MT * 64 * 16
    return lds <= 150 * 1024 and (ctiles + CTW - 1) // CTW <= 8 // KG and max(lds, red) <= 160 * 1024


def wgrad_path(c):
    """The kernel launch_imgwgrad reaches: conv1c_wgrad (imgconv1_copies.hip), wg1<NC> (imgwgrad1_kernel),
    wp<MT,CTW[,KGn]> (imgwgrad_persist_kernel, ":unpool" = dY un-pooled on load) or wg<MT,CT>
    (imgwgrad_kernel).  Derived from the host code's conditions, not observed (see conv_path)."""
    O = c.O
    if c.CS <= 4:
        return "conv1c_wgrad" if _mnist_conv1(c) and c.pooled else "wg1<%d>" % _nt(c.N)
    if c.CS % 16 == 0 and c.N % 8 == 0 and O <= 32 and c.B >= 128 and not (c.pooled and O & 1):
        ctiles = c.K * c.K * c.CS // 16
        ctw = (ctiles + 7) // 8
        pick = None
        if not c.db and not c.pooled:
            if ctiles <= 9 and c.N <= 16:
                pick = (1, 9, 8)
            elif ctiles <= 9 and c.N <= 32:
                pick = (2, 9, 8)
            elif ctiles <= 18 and c.N <= 32:
                pick = (2, 9, 4)
            elif c.N > 32 and ctiles <= 40:
                pick = (4, 5, 1)
        if pick is None and c.N > 32 and ctw <= 7:
            pick = (4, 7, 1)
        if pick is None and c.N <= 32 and ctw <= 8:
            pick = (2, 8, 1)
        if pick is not None and _wp_fits(c, *pick):
            MT, CTW, KG = pick
            return "wp<%d,%d%s>%s" % (MT, CTW, ",KG%d" % KG if KG > 1 else "", ":unpool" if c.pooled else "")
    return "wg<%d,%d>" % {1: (1, 8), 2: (2, 6), 4: (4, 4)}[_nt(c.N)]


def wgrad_npf(c):
    """(npfs, npfd) of wp_launch: 16-B chunks per thread (512 threads) of the source and of dY."""
    sch = c.S * c.S * c.CS // 8
    dch = ((c.O // 2) ** 2 if c.pooled else c.O * c.O) * c.N // 8
    return (sch + 511) // 512, (dch + 511) // 512


CONV_PATHS = ("img<1>", "img<2>", "img<4>", "img<4>:lds",
              "cfg<1,2,16,1>:csc", "cfg<1,2,16,1>:rt", "cfg<1,2,16,1>:unpool",
              "cfg<1,2,8,2>:csc", "cfg<1,2,8,2>:rt", "cfg<1,2,8,2>:unpool",
              "cfg<2,1,4,2>:csc", "cfg<2,1,4,2>:rt",
              "cfg<2,2,8,2>:csc", "cfg<2,2,8,2>:rt", "cfg<2,2,8,2>:unpool",
              "fixed:fwd", "fixed:dgrad",
              "img1<1>:staged", "img1<2>:staged", "img1<4>:staged",
              "img1<1>:direct", "img1<2>:direct", "img1<4>:direct", "conv1c_fwd")
WGRAD_PATHS = ("wg<1,8>", "wg<2,6>", "wg<4,4>", "wg1<1>", "wg1<2>", "wg1<4>", "conv1c_wgrad",
               "wp<1,9,KG8>", "wp<2,9,KG8>", "wp<2,9,KG4>", "wp<4,5>",
               "wp<2,8>", "wp<2,8>:unpool", "wp<4,7>", "wp<4,7>:unpool")


def path(c):
    return conv_path(c) if c.kind == "conv" else wgrad_path(c)


# --------------------------------------------------------------------------- buffers
_DT = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}


class Built:
    """The CPU buffers of one case: ``bufs[name]`` flat, guards included; ``shape[name]`` of the logical
    view at [GUARD, GUARD + numel); ``log[name]`` the logical values as stored (float64 / uint8)."""

    def __init__(self, case):
        self.case = case
        self.bufs, self.shape, self.log, self.outputs = {}, {}, {}, []
        self.rung = None
        self._z = self._ref = None

    def put(self, name, values, dtype, guard_fill, output=False):
        dt = _DT[dtype]
        v = torch.from_numpy(np.ascontiguousarray(values)).to(dt)
        assert (GUARD * v.element_size()) % 16 == 0
        buf = torch.full((v.numel() + 2 * GUARD,), guard_fill, dtype=dt)
        buf[GUARD:GUARD + v.numel()] = v.reshape(-1)
        self.bufs[name], self.shape[name] = buf, tuple(values.shape)
        self.log[name] = v.numpy() if dtype == "u8" else v.double().numpy()
        if output:
            self.outputs.append(name)


def view(bufs, b, name):
    """The logical view of buffer ``name`` (None if the case has none)."""
    if name not in bufs:
        return None
    n = int(np.prod(b.shape[name]))
    return bufs[name][GUARD:GUARD + n].view(b.shape[name])


def _ints(rng, shape, h):
    return rng.integers(1, h + 1, size=shape).astype(np.float64) * rng.choice([-1.0, 1.0], size=shape)


def _fill_conv(b, hx, hw):
    c = b.case
    rng = np.random.default_rng(c.seed)
    nan = float("nan")
    O = c.O
    if c.src == "pooled":
        b.put("src_pooled", _ints(rng, (c.B, c.S // 2, c.S // 2, c.CS), hx), "bf16", nan)
        b.put("src_argmax", rng.integers(0, 4, size=(c.B, c.S // 2, c.S // 2, c.CS)).astype(np.uint8), "u8", 0xFF)
    else:
        b.put("src", _ints(rng, (c.B, c.S, c.S, c.CS), hx), "bf16", nan)
    b.put("w", _ints(rng, (c.N, c.K, c.K, c.CS), hw), "bf16", nan)
    if c.bias:
        b.put("bias", _ints(rng, (c.N,), 2 if c.regime == "unit" else hx), "f32", nan)
    if c.mask:
        m = rng.choice([-1.0, 1.0], size=(c.B, O, O, c.N))
        m.reshape(-1)[:len(MASK_SPECIALS)] = MASK_SPECIALS    # image 0, pixel 0, channels 0-5
        m[-1, -1, -1, -len(MASK_SPECIALS):] = MASK_SPECIALS       # last image, last pixel, channels N-6.. (>= 10)
        b.put("mask", m, "bf16", nan)
    if c.sc:
        b.put("g", _ints(rng, (c.B, O // c.sc, O // c.sc, c.sc_C), 2 if c.regime == "unit" else hx), "bf16", nan)
    oshape = (c.B, O // 2, O // 2, c.N) if c.pool else (c.B, O, O, c.N)
    b.put("y", np.full(oshape, nan), "bf16", SENT, output=True)
    if c.pool:
        b.put("argmax", np.full(oshape, 0xFF, dtype=np.uint8), "u8", 0xFF, output=True)


def _fill_wgrad(b):
    c = b.case
    rng = np.random.default_rng(c.seed)
    nan = float("nan")
    O = c.O
    b.put("src", _ints(rng, (c.B, c.S, c.S, c.CS), 2), "bf16", nan)
    if c.pooled:
        b.put("dy_pooled", _ints(rng, (c.B, O // 2, O // 2, c.N), 2), "bf16", nan)
        b.put("dy_argmax", rng.integers(0, 4, size=(c.B, O // 2, O // 2, c.N)).astype(np.uint8), "u8", 0xFF)
    else:
        b.put("dy", _ints(rng, (c.B, O, O, c.N), 2), "bf16", nan)
    b.put("dw", _ints(rng, (c.N, c.K, c.K, c.CS), 3), "f32", SENT, output=True)
    if c.db:
        b.put("db", _ints(rng, (c.N,), 3), "f32", SENT, output=True)


def build(c):
    """CPU buffers of one case (deterministic in the case), on the rung of its regime's ladder that
    meets the regime's condition (the last rung if none does: ``conditions`` then fails)."""
    if c.kind == "wgrad":
        b = Built(c)
        _fill_wgrad(b)
        b.rung = (2, 2)
        return b
    ladder = UNIT_LADDER if c.regime == "unit" else tuple((h, h) for h in WIDE_LADDER)
    for rung in ladder:
        b = Built(c)
        b.rung = rung
        _fill_conv(b, *rung)
        info = oracle(b)[1]
        if (info["max_abs"] <= UNIT_CAP) if c.regime == "unit" else (info["ties_up"] and info["ties_down"]):
            break
    return b


def conditions(b):
    """Assert the data conditions of the case's regime on its reference."""
    c = b.case
    info = oracle(b)[1]
    hx, hw = b.rung
    for name in ("src", "src_pooled", "w", "bias", "g", "dy", "dy_pooled"):
        if name in b.log:
            assert (b.log[name] != 0).all() and (b.log[name] == np.round(b.log[name])).all(), (c, name)
    hb = max([np.abs(b.log[k]).max() for k in ("bias", "g") if k in b.log] + [0.0])
    assert c.terms * hx * hw + hb < 2 ** 24 and info["max_sum"] < 2 ** 24, (c, info)
    if c.kind == "wgrad":
        assert 2 * info["max_sum"] < 2 ** 24, (c, info)   # scale = 0.5 and the old value: still exact in fp32
    elif c.regime == "unit":
        assert info["max_abs"] <= UNIT_CAP, (c, info)
    else:
        assert info["ties_up"] > 0 and info["ties_down"] > 0, (c, info)


# --------------------------------------------------------------------------- oracle
def rne_bf16(v, trunc=False):
    """float64 -> the nearest bf16 value, ties to even (``trunc``: toward zero), as float64.  The inputs
    are integers below 2^24, so the step through fp32 is exact."""
    f = np.ascontiguousarray(v, dtype=np.float32)
    assert (f.astype(np.float64) == v).all()
    u = f.view(np.uint32).astype(np.uint64)
    if not trunc:
        u = u + 0x7FFF + ((u >> 16) & 1)
    u = (u & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def _ties(v):
    """(ties rounded up in magnitude, ties rounded down) among the values RNE has to round."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    tie = (u & 0xFFFF) == 0x8000
    up = ((u >> 16) & 1) == 1
    return int((tie & up).sum()), int((tie & ~up).sum())


def _max_abs(v):
    return float(max(v.max(), -v.min()))


def _unpool(p, am):
    """[B][PH][PW][C] pooled values -> [B][2PH][2PW][C]: each value at position (dy, dx) = (am >> 1, am & 1)
    of its 2 x 2 window, zeros elsewhere."""
    B, PH, PW, C = p.shape
    full = np.zeros((B, 2 * PH, 2 * PW, C))
    bi, yi, xi, ci = np.indices(p.shape)
    full[bi, 2 * yi + (am >> 1), 2 * xi + (am & 1), ci] = p
    return full


def _conv_source(b):
    c = b.case
    s = _unpool(b.log["src_pooled"], b.log["src_argmax"]) if c.src == "pooled" else b.log["src"]
    if c.dil > 1:
        d = np.zeros((c.B, c.S * c.dil, c.S * c.dil, c.CS))
        d[:, ::c.dil, ::c.dil, :] = s
        s = d
    return np.pad(s, ((0, 0), (c.pad, c.pad), (c.pad, c.pad), (0, 0)))


def _tap_weight(b, kh, kw):
    """[N][CS] weights that multiply the padded source at offset (kh, kw)."""
    c = b.case
    w = b.log["w"]
    return w[:, c.K - 1 - kh, c.K - 1 - kw, :] if c.flip else w[:, kh, kw, :]


def _tap_patch(c, sp, kh, kw, O):
    e = (O - 1) * c.stride + 1
    return sp[:, kh:kh + e:c.stride, kw:kw + e:c.stride, :]


def _conv_sums(b):
    """Exact pre-bias sums [B][O][O][N], one tensordot per tap (cached on the case's buffers)."""
    if b._z is None:
        c = b.case
        sp = _conv_source(b)
        z = np.zeros((c.B, c.O, c.O, c.N))
        step = max(1, 2 ** 18 // (c.O * c.O * c.N))   # images per pass: the running sums stay in cache
        for b0 in range(0, c.B, step):
            zc, spc = z[b0:b0 + step], sp[b0:b0 + step]
            for kh in range(c.K):
                for kw in range(c.K):
                    zc += np.tensordot(_tap_patch(c, spc, kh, kw, c.O), _tap_weight(b, kh, kw), axes=([3], [1]))
        b._z = (sp, z)
    return b._z


CONV_MUTATIONS = ("tap_at_border", "channel_of_tap", "last_image_from_first", "last_max", "truncate")
WGRAD_MUTATIONS = ("last_row", "last_image", "overwrite", "db_unscaled")


def _oracle_conv(b, mutate):
    c = b.case
    O = c.O
    sp, z = _conv_sums(b)
    t = min(c.pad, c.K - 1)   # tap (t, t) reads source pixel (oy * stride, ox * stride): never padding
    if mutate == "tap_at_border":      # (a) a padding off-by-one: that tap missing at output row 0 and the last column
        term = np.tensordot(_tap_patch(c, sp, t, t, O), _tap_weight(b, t, t), axes=([3], [1]))
        z = z.copy()
        z[:, 0, :, :] -= term[:, 0, :, :]
        z[:, 1:, O - 1, :] -= term[:, 1:, O - 1, :]
    elif mutate == "channel_of_tap":   # (b) source channel 0 of that tap missing for the last output channel
        z = z.copy()
        z[..., c.N - 1] -= _tap_patch(c, sp, t, t, O)[..., 0] * _tap_weight(b, t, t)[c.N - 1, 0]
    elif mutate == "last_image_from_first":   # (c)
        z = z.copy()
        z[c.B - 1] = z[0]
    info = {"max_sum": _max_abs(z)}
    if c.bias:
        z = z + b.log["bias"]
    cap = max(info["max_sum"], _max_abs(z))
    if c.act == ops.ACT_RELU:
        z = np.maximum(z, 0.0)
    else:
        assert c.act == ops.ACT_NONE
    ref = {}
    if c.pool:
        win = z.reshape(c.B, O // 2, 2, O // 2, 2, c.N).transpose(0, 1, 3, 5, 2, 4).reshape(c.B, O // 2, O // 2, c.N, 4)
        first = np.argmax(win, axis=-1)               # the first maximum, index dy * 2 + dx
        last = 3 - np.argmax(win[..., ::-1], axis=-1)
        z = win.max(axis=-1)
        ref["argmax"] = (last if mutate == "last_max" else first).astype(np.uint8)   # (d)
        info["pos_ties"] = int(((first != last) & (z > 0)).sum())
    if c.mask:
        z = np.where(b.log["mask"] > 0, z, 0.0)
    info["ties_up"], info["ties_down"] = _ties(z)
    y = rne_bf16(z, trunc=mutate == "truncate")   # (e)
    if c.sc:
        s = c.sc
        v = y[:, ::s, ::s, :] + b.log["g"][..., :c.N]
        cap = max(cap, _max_abs(v))
        u, d = _ties(v)
        info["ties_up"] += u
        info["ties_down"] += d
        y[:, ::s, ::s, :] = rne_bf16(v, trunc=mutate == "truncate")
    info["max_abs"] = cap
    ref["y"] = y
    return ref, info


def _oracle_wgrad(b, mutate):
    c = b.case
    O = c.O
    d = _unpool(b.log["dy_pooled"], b.log["dy_argmax"]) if c.pooled else b.log["dy"]
    if mutate == "last_row":           # (f)
        d = d.copy()
        d[:, O - 1] = 0
    elif mutate == "last_image":       # (g)
        d = d.copy()
        d[c.B - 1] = 0
    sp = np.pad(b.log["src"], ((0, 0), (c.pad, c.pad), (c.pad, c.pad), (0, 0)))
    s = np.zeros((c.N, c.K, c.K, c.CS))
    for kh in range(c.K):
        for kw in range(c.K):
            s[:, kh, kw, :] = np.tensordot(d, _tap_patch(c, sp, kh, kw, O), axes=([0, 1, 2], [0, 1, 2]))
    sb = d.sum(axis=(0, 1, 2))
    info = {"max_sum": float(max(np.abs(s).max(), np.abs(sb).max()))}
    ref = {"dw": (0.0 if mutate == "overwrite" else b.log["dw"]) + c.scale * s}     # (h)
    if c.db:
        ref["db"] = b.log["db"] + (1.0 if mutate == "db_unscaled" else c.scale) * sb   # (i)
    return ref, info


def oracle(b, mutate=None):
    """({output name: exact expected logical values}, info) of the case.  ``mutate``: one of CONV_MUTATIONS /
    WGRAD_MUTATIONS - what a wrong kernel would give (letters (a)-(i) in the code)."""
    if mutate is None and b._ref is not None:
        return b._ref
    out = (_oracle_conv if b.case.kind == "conv" else _oracle_wgrad)(b, mutate)
    if mutate is None:
        b._ref = out   # (callers leave the arrays as they are)
    return out


def mutations(b, info):
    """The mutations that apply to the case:
    tap_at_border, channel_of_tap: every conv case; last_image_from_first: B >= 2; last_max: a pooled
    case whose reference has a tie among positive values in some window (every pooled ``unit`` case has
    to have one: asserted); truncate: ``wide`` (``unit`` values are exact, there is nothing to round).
    last_row, overwrite: every wgrad case; last_image: B >= 2; db_unscaled: cases with db."""
    c = b.case
    if c.kind == "wgrad":
        return [m for m in WGRAD_MUTATIONS if (m != "last_image" or c.B >= 2) and (m != "db_unscaled" or c.db)]
    out = ["tap_at_border", "channel_of_tap"]
    if c.B >= 2:
        out.append("last_image_from_first")
    if c.pool:
        if c.regime == "unit":
            assert info["pos_ties"] > 0, (c, "no tie among positive values: first-maximum-wins is not exercised")
        if info["pos_ties"] > 0:
            out.append("last_max")
    if c.regime == "wide":
        out.append("truncate")
    return out


# --------------------------------------------------------------------------- run and check
def launch(b, dev, workspace=None, defer=None):
    """Launch the case of ``b`` = build(case) on ``dev`` ("cuda": the HIP kernels, "cpu": the project's fp32
    reference path); returns the whole buffers on ``dev`` (and "sc_done": what ops.imgconv_shortcut
    answered).  It takes the built buffers, not the case, so that one build serves the oracle, several
    launches and the check."""
    c = b.case
    t = {k: v.clone().to(dev) for k, v in b.bufs.items()}
    v = lambda name: view(t, b, name)  # noqa: E731
    O = c.O
    if c.kind == "conv":
        geom = dict(B=c.B, SH=c.S, SW=c.S, CS=c.CS, OH=O, OW=O, N=c.N, KH=c.K, KW=c.K, stride=c.stride, pad=c.pad,
                    dil=c.dil)
        if c.sc:
            assert c.flip and not (c.pool or c.bias or c.mask or c.act) and c.src == "plain"
            done = ops.imgconv_shortcut(v("w"), v("y"), v("g"), c.sc, src=v("src"), **geom)
            if not done:   # only dx was written: the caller adds the shortcut gradient
                ops.shortcut_grad_add(v("g"), v("y"), c.sc)
            t["sc_done"] = bool(done)
        else:
            ops.imgconv(v("w"), v("y"), src=v("src"), src_pooled=v("src_pooled"), src_argmax=v("src_argmax"),
                        bias=v("bias"), argmax=v("argmax"), relu_mask=v("mask"), flip_taps=c.flip, act=c.act,
                        pool=c.pool, **geom)
    else:
        ops.imgwgrad(v("src"), v("dw"), v("db"), B=c.B, SH=c.S, SW=c.S, CS=c.CS, OH=O, OW=O, N=c.N, KH=c.K, KW=c.K,
                     stride=c.stride, pad=c.pad, dy=v("dy"), dy_pooled=v("dy_pooled"), dy_argmax=v("dy_argmax"),
                     scale=c.scale, workspace=workspace, max_blocks=c.max_blocks, defer=defer)
    return t


def fetch(t):
    return {k: (x.cpu() if isinstance(x, torch.Tensor) else x) for k, x in t.items()}


def run(b, dev, workspace=None):
    """launch + fetch: the whole buffers of ``b`` = build(case), guards included, on the CPU."""
    return fetch(launch(b, dev, workspace=workspace))


def as_buffers(b, ref):
    """Logical outputs (an oracle's) laid into sentinel-guarded buffers, as ``run`` returns them."""
    got = {}
    for name in b.outputs:
        buf = b.bufs[name].clone()
        n = buf.numel() - 2 * GUARD
        buf[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(ref[name])).to(buf.dtype).reshape(-1)
        got[name] = buf
    return got


def _first_diff(c, name, a, r, where=None):
    diff = a != r
    if where is not None:
        diff &= where
    i = tuple(int(k) for k in np.argwhere(diff)[0])
    return "%s: %s%s = %r, expected %r (%d of %d elements differ)" % (c, name, list(i), a[i].item(), r[i].item(),
                                                                      int(diff.sum()), diff.size)


def check(b, got, ref=None):
    """Assert the sentinels untouched, no NaN in the logical outputs, and every value bit-equal to the
    oracle's (the argmax wherever the pooled reference is > 0: elsewhere the ReLU discarded the window,
    the consumers mask it, and the kernel picks its maximum before the activation)."""
    c = b.case
    ref = ref or oracle(b)[0]
    for name in b.outputs:
        buf = got[name]
        n = buf.numel() - 2 * GUARD
        guards = torch.cat([buf[:GUARD], buf[GUARD + n:]])
        logical = buf[GUARD:GUARD + n].view(b.shape[name])
        r = ref[name]
        assert tuple(r.shape) == b.shape[name], (c, name, r.shape)
        if name == "argmax":
            assert (guards == 0xFF).all(), "%s: argmax written outside its logical elements" % (c,)
            assert (logical < 4).all(), "%s: %d argmax bytes unwritten or out of range" % (c, int((logical >= 4).sum()))
            where = ref["y"] > 0
            a = logical.numpy()
            assert (a[where] == r[where]).all(), _first_diff(c, name, a, r, where)
            continue
        assert (guards == SENT).all(), "%s: %s written outside its logical elements" % (c, name)
        assert not torch.isnan(logical).any(), "%s: NaN in %s (%d elements: unwritten, or poisoned by a stray read)" % (
            c, name, int(torch.isnan(logical).sum()))
        want = torch.from_numpy(np.ascontiguousarray(r)).to(logical.dtype)
        assert (want.double().numpy() == r).all(), "%s: the reference of %s is not exact in %s" % (
            c, name, logical.dtype)
        if not torch.equal(logical, want):
            raise AssertionError(_first_diff(c, name, logical.double().numpy(), r))


# --------------------------------------------------------------------------- case groups
R, NONE = ops.ACT_RELU, ops.ACT_NONE


def _both(cases):
    """conv cases in both regimes."""
    return [dataclasses.replace(c, regime=r) for c in cases for r in ("unit", "wide")]


def per_image_cases():
    """B in {1, 3}: imgconv_kernel<NT>, NT = 1, 2, 4 via N = 16, 32, 64, and one partial n-tile (N = 24)."""
    C = ConvCase
    conv2 = dict(S=14, CS=32, K=5, pad=2, pool=True, act=R, bias=True)
    return _both([
        C(B=3, N=64, **conv2), C(B=1, N=16, **conv2), C(B=3, N=32, **conv2), C(B=3, N=24, **conv2),
        C(B=3, S=32, CS=16, N=16, K=3, pad=1),
        C(B=3, S=8, CS=64, N=64, K=3, pad=1, act=R, bias=True),
        C(B=1, S=32, CS=16, N=32, K=3, stride=2, pad=1),                       # 32 -> 16
        C(B=3, S=12, CS=8, N=16, K=5, pool=True, act=R),                       # valid padding, 12 -> 8 -> 4
        C(B=3, S=7, CS=16, N=32, K=3, pad=1, bias=True),                       # odd map, no pool
        C(B=3, S=14, CS=64, N=32, K=5, pad=2, flip=True, mask=True),           # data gradient, ReLU' mask
        C(B=3, S=14, CS=64, N=32, K=5, pad=2, flip=True, mask=True, src="pooled"),
    ])


def persistent_cases(half, nt=None):
    """launch_cfg at B = 64 (one image per workgroup) and B = 259 (three workgroups take a second image).
    half: "fwd" | "dgrad"; nt: only the cases of that N class (1, 2, 4 n-tiles: N <= 16, 32, 64)."""
    C = ConvCase
    out = []
    if half == "fwd":
        for B in (64, 259):
            out += [
                C(B=B, S=32, CS=16, N=16, K=3, pad=1, bias=True, act=R),        # <1,2,16,1> csc npf 2, staged OW 32
                C(B=B, S=16, CS=32, N=32, K=3, pad=1),                          # <1,2,8,2> csc npf 1, staged OW 16
                C(B=B, S=8, CS=64, N=64, K=3, pad=1, bias=True),                # <2,1,4,2> csc npf 1, staged OW 8
                C(B=B, S=16, CS=64, N=64, K=3, pad=1, act=R),                   # <2,2,8,2> csc npf 2, direct (LDS)
                C(B=B, S=16, CS=32, N=64, K=3, pad=1),                          # <2,2,8,2> csc npf 1, staged OW 16
            ]
        out += [
            C(B=64, S=16, CS=16, N=16, K=3, pad=1),                             # <1,2,16,1> csc npf 1
            C(B=64, S=14, CS=8, N=16, K=5, pad=2, bias=True, act=R),            # <1,2,16,1> rt, CS 8, direct OW 14
            C(B=64, S=16, CS=24, N=32, K=3, pad=1),                             # <1,2,8,2> rt, CS 24
            C(B=64, S=28, CS=32, N=32, K=3, pad=1, act=R),                      # <1,2,8,2> rt npf 4, direct OW 28
            C(B=259, S=24, CS=32, N=32, K=3, pad=1, bias=True),                 # <1,2,8,2> rt npf 3, direct OW 24
            C(B=64, S=8, CS=8, N=64, K=3, pad=1),                               # <2,1,4,2> rt
            C(B=259, S=16, CS=32, N=64, K=5, pad=2, bias=True, act=R),          # <2,2,8,2> rt 5x5, direct (LDS)
            C(B=64, S=14, CS=32, N=32, K=5, pad=2, pool=True, act=R, bias=True),   # pooled forward, <1,2,8,2>
            C(B=259, S=14, CS=32, N=16, K=5, pad=2, pool=True, act=R, bias=True),  # pooled forward, <1,2,16,1>
            C(B=64, S=14, CS=32, N=64, K=5, pad=2, pool=True, act=R, bias=True),   # pooled forward, <2,2,8,2>
            C(B=64, S=32, CS=16, N=32, K=3, stride=2, pad=1),                   # stride 2, <1,2,8,2> csc npf 2
            C(B=259, S=16, CS=32, N=64, K=3, stride=2, pad=1, bias=True),       # stride 2, 16 -> 8: <2,1,4,2>
        ]
    else:
        out += [
            C(B=64, S=32, CS=16, N=16, K=3, pad=1, flip=True, mask=True),       # staged epilogue applies the mask
            C(B=259, S=16, CS=32, N=32, K=3, pad=1, flip=True, mask=True),
            C(B=64, S=8, CS=64, N=64, K=3, pad=1, flip=True, mask=True),
            C(B=64, S=28, CS=32, N=32, K=3, pad=1, flip=True, mask=True),       # direct epilogue applies the mask
            C(B=64, S=14, CS=64, N=32, K=5, pad=2, flip=True, mask=True, src="pooled"),   # <1,2,8,2> unpool
            C(B=259, S=14, CS=16, N=16, K=5, pad=2, flip=True, src="pooled"),             # <1,2,16,1> unpool
            C(B=64, S=16, CS=32, N=64, K=3, pad=1, flip=True, mask=True, src="pooled"),   # <2,2,8,2> unpool
            C(B=96, S=16, CS=32, N=16, K=3, pad=1, flip=True, dil=2),           # dX of a stride-2 conv, O = 32
            C(B=259, S=8, CS=64, N=32, K=3, pad=1, flip=True, dil=2, mask=True),
            C(B=64, S=32, CS=16, N=16, K=3, pad=1, flip=True, sc=1, sc_C=16),   # shortcut gradient, stride 1
            C(B=259, S=16, CS=32, N=32, K=3, pad=1, flip=True, sc=1, sc_C=32),
            C(B=64, S=16, CS=32, N=16, K=3, pad=1, flip=True, dil=2, sc=2, sc_C=32),   # stride 2, wider than N
            C(B=259, S=8, CS=64, N=32, K=3, pad=1, flip=True, dil=2, sc=2, sc_C=64),
        ]
    return _both([c for c in out if nt is None or _nt(c.N) == nt])


def lds_fallthrough_cases():
    """28x28x32 5x5 N = 64: the persistent kernel needs more than 160 KB of LDS, the per-image kernel runs."""
    return _both([ConvCase(B=64, S=28, CS=32, N=64, K=5, pad=2, pool=True, act=R, bias=True)])


def fixed_cases(half):
    """imgconv_fixed_kernel: MNIST conv2 forward / data gradient at B = 256 and 259."""
    if half == "fwd":
        return _both([ConvCase(B=B, S=14, CS=32, N=64, K=5, pad=2, pool=True, act=R, bias=True) for B in (256, 259)])
    return _both([ConvCase(B=B, S=14, CS=64, N=32, K=5, pad=2, flip=True, mask=True, src="pooled") for B in (256, 259)])


def few_channel_cases(which=None, regime=None):
    """CS <= 4 forward: imgconv1_kernel<NT> staged (no pool, N % 8 == 0) and direct (pool) ("img1"), and the
    MNIST conv1 shifted-copy kernel at B = 256 and 1030 (grid min(B, 1024): a second image in six
    workgroups) ("conv1c")."""
    return [c for c in _both(_few_channel()) if (which is None or conv_path(c).startswith(which)) and
            regime in (None, c.regime)]


def _few_channel():
    C = ConvCase
    return [
        C(B=70, S=32, CS=3, N=16, K=3, pad=1, bias=True, act=R),                # staged <1>
        C(B=2, S=32, CS=2, N=32, K=3, pad=1),                                   # staged <2>
        C(B=2, S=28, CS=1, N=64, K=3, stride=2, pad=1, bias=True),              # staged <4>, stride 2
        C(B=70, S=28, CS=1, N=16, K=3, stride=2, pad=1, pool=True, act=R),      # direct <1>, stride 2, 14 -> 7
        C(B=2, S=28, CS=1, N=32, K=5, pad=2, pool=True, act=R, bias=True),      # direct <2>: conv1 below B = 256
        C(B=2, S=32, CS=3, N=64, K=3, pad=1, pool=True, bias=True),             # direct <4>, act none
        C(B=70, S=16, CS=2, N=32, K=3, pad=1, pool=True, act=R, bias=True),
        C(B=256, S=28, CS=1, N=32, K=5, pad=2, pool=True, act=R, bias=True),    # conv1c_fwd
        C(B=1030, S=28, CS=1, N=32, K=5, pad=2, pool=True, act=R, bias=True),
        C(B=256, S=28, CS=1, N=32, K=5, pad=2, pool=True, bias=True),           # act none
    ]


def wgrad_per_image_cases():
    """imgwgrad_kernel<1,8>, <2,6>, <4,4>: B = 5 (4 images per block + 1 ragged) and 3; OW = 14, 7, 8, 32."""
    W = WgradCase
    return [
        W(B=5, S=14, CS=32, N=64, K=5, pad=2, pooled=True),                     # OW 14 (padded to 16), pooled dY
        W(B=3, S=14, CS=32, N=64, K=5, pad=2, db=False),
        W(B=5, S=7, CS=16, N=32, K=3, pad=1),                                   # OW 7 (to 8)
        W(B=3, S=8, CS=64, N=64, K=3, pad=1),                                   # OW 8
        W(B=5, S=32, CS=16, N=16, K=3, pad=1, db=False),                        # OW 32
        W(B=3, S=32, CS=16, N=32, K=3, stride=2, pad=1),
        W(B=130, S=14, CS=8, N=16, K=5, pad=2),                                 # CS % 16 != 0: not persistent
        W(B=130, S=16, CS=24, N=32, K=3, pad=1, db=False),
    ]


def wgrad_few_channel_cases():
    """imgwgrad1_kernel<NC>, NC = 1, 2, 4, and the MNIST conv1 shifted-copy weight gradient at B = 256 and
    330 (grid min(B, 320): ten workgroups take a second image)."""
    W = WgradCase
    return [
        W(B=5, S=28, CS=1, N=32, K=5, pad=2, pooled=True),
        W(B=3, S=28, CS=1, N=64, K=3, stride=2, pad=1),
        W(B=7, S=12, CS=1, N=16, K=5),                                          # valid padding, OW 8
        W(B=70, S=32, CS=3, N=16, K=3, pad=1, db=False),
        W(B=5, S=16, CS=2, N=32, K=3, pad=1),
        W(B=256, S=28, CS=1, N=32, K=5, pad=2, pooled=True),
        W(B=330, S=28, CS=1, N=32, K=5, pad=2, pooled=True),
    ]


def wgrad_persistent_cases(kind):
    """imgwgrad_persist_kernel at B = 128 and 130.  kind: "kgroups" (3x3, no db) | "db"."""
    W = WgradCase
    out = []
    if kind == "kgroups":
        for B in (128, 130):
            out += [
                W(B=B, S=16, CS=16, N=16, K=3, pad=1, db=False),                # <1,9,KG8>
                W(B=B, S=16, CS=16, N=32, K=3, pad=1, db=False),                # <2,9,KG8>
                W(B=B, S=16, CS=32, N=32, K=3, pad=1, db=False),                # <2,9,KG4>, npfs 2
                W(B=B, S=8, CS=64, N=64, K=3, pad=1, db=False),                 # <4,5>, npfs 1
                W(B=B, S=16, CS=32, N=64, K=3, pad=1, db=False),                # <4,5>
            ]
        out += [
            W(B=300, S=8, CS=64, N=64, K=3, pad=1, db=False),                   # ipw = 4: several images per workgroup
            W(B=128, S=32, CS=16, N=16, K=3, pad=1, db=False),                  # npfs 4, npfd 4
            W(B=130, S=32, CS=16, N=32, K=3, stride=2, pad=1, db=False),        # stride 2
            W(B=130, S=16, CS=32, N=32, K=3, pad=1, db=False, max_blocks=64),
            W(B=130, S=16, CS=16, N=32, K=3, pad=1, db=False, ws="own"),
        ]
    else:
        out += [
            W(B=130, S=16, CS=16, N=32, K=3, pad=1),                            # <2,8>
            W(B=128, S=16, CS=16, N=32, K=3, pad=1, pooled=True),               # <2,8> unpool
            W(B=130, S=8, CS=64, N=64, K=3, pad=1),                             # <4,7>
            W(B=259, S=14, CS=32, N=64, K=5, pad=2, pooled=True),               # <4,7> unpool: MNIST conv2
            W(B=130, S=32, CS=16, N=16, K=3, pad=1, ws="own"),                  # <2,8>, N = 16
        ]
    return out


def wgrad_deferred_cases():
    """Three launches with own workspaces whose reduces one grouped flush sums."""
    W = WgradCase
    return [W(B=130, S=16, CS=16, N=16, K=3, pad=1, db=False, ws="own"),
            W(B=128, S=8, CS=64, N=64, K=3, pad=1, db=False, ws="own"),
            W(B=130, S=16, CS=32, N=32, K=3, pad=1, ws="own")]


GROUPS = {
    "per_image": per_image_cases,
    "persistent_fwd_n16": lambda: persistent_cases("fwd", 1),
    "persistent_fwd_n32": lambda: persistent_cases("fwd", 2),
    "persistent_fwd_n64": lambda: persistent_cases("fwd", 4),
    "persistent_dgrad": lambda: persistent_cases("dgrad"),
    "lds_fallthrough": lds_fallthrough_cases,
    "fixed_fwd": lambda: fixed_cases("fwd"),
    "fixed_dgrad": lambda: fixed_cases("dgrad"),
    "few_channel_img1": lambda: few_channel_cases("img1"),
    "few_channel_conv1c_unit": lambda: few_channel_cases("conv1c", "unit"),
    "few_channel_conv1c_wide": lambda: few_channel_cases("conv1c", "wide"),
    "wgrad_per_image": wgrad_per_image_cases,
    "wgrad_few_channel": wgrad_few_channel_cases,
    "wgrad_kgroups": lambda: wgrad_persistent_cases("kgroups"),
    "wgrad_db": lambda: wgrad_persistent_cases("db"),
    "wgrad_deferred": wgrad_deferred_cases,
}
