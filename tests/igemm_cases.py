"""Cases, guarded buffers, an exact float64 oracle and a dispatch mirror for the implicit-GEMM
convolutions of csrc/kernels/igemm.hip (``ops.conv_fwd`` / ``ops.conv_dgrad`` / ``ops.conv_wgrad`` with
C and Cout multiples of 64).

Shared by tests/test_igemm_paths_gpu.py (the kernels) and tests/test_igemm_oracle_cpu.py (the oracle
itself: its data conditions, agreement with the project's fp32 CPU reference path, sensitivity to
twelve kinds of wrong kernel, and coverage of the dispatch paths).

Data: every operand is a small non-zero signed integer held in bf16.  The kernels multiply bf16 operands
and accumulate in fp32, so every product and every partial sum - of any tile, k-split, m-split or
stride phase, in any order - is an integer below 2^24: the accumulation is exact, the expected output
is one bit pattern and ``check`` compares with ``torch.equal``.  No tolerance appears anywhere.

  unit     magnitudes from the first rung of UNIT_LADDER at which every value the kernel stores (the
           sum, and the sum plus the accumulated old value) is an integer of magnitude <= 256, hence
           exact in bf16.  Every term is non-zero: a dropped, doubled or misplaced term changes an output.
  rounded  (bf16 outputs, deep k) magnitudes 1..h, h the first of ROUNDED_LADDER at which the values the
           kernel has to round hold exact ties that round-to-nearest-even moves up in magnitude and
           ties it moves down; the expected output is RNE_bf16 of the exact integer.
  Weight gradients have fp32 outputs and no cap: operands 1..2, ``scale`` in {0.25, 0.5, 1}, dw
  pre-filled with non-zero integers that the oracle adds (the op is +=).

Accumulation (``accumulate``) rounds differently by path, and the oracle takes the path from the
mirrored dispatch: the unsplit epilogue stores RNE(RNE(S) + old) (the tile is rounded to bf16 in LDS
before the old value is added), the split-K combine RNE(S + old) (fp32 partials).  With ``acc_src``
old is src * bit, never dx's contents: dx is pre-filled with NaN.  The project's CPU path rounds as
the unsplit epilogue does (it stores bf16(S), then adds), so test_igemm_oracle_cpu.py compares it
with the oracle's unsplit rounding in every case; the two coincide in every ``unit`` case (nothing is
rounded) and differ only in the ``rounded`` split-K accumulating cases.

Statistics are exact as well.  Forward ``stats`` has bn_stats semantics: (sum (y - K), sum (y - K)^2)
per channel around the shift K = y[row 0] of the STORED bf16 output (norm.hip bn_stats_kernel; the fused
epilogue keeps per-tile sums around each tile's first row and bn_part_fold moves them to K with
bn_shift_fold of bn_chan.h: s = s_t + n_t d, q = q_t + 2 d s_t + n_t d^2, d = K_t - K).  ``conditions``
replays that fold for both tile heights with absolute values and requires every intermediate below
2^24.  BN-backward statistics (sum g, sum g * (x - mean) * invstd of the final dx): integer x and mean,
invstd in {0.5, 1, 2}, gamma in +-{1, 2}, beta = integer + 0.25 (no pre-activation is 0: the recomputed
ReLU mask has no ties); both are exact multiples of 1/4.

Guards: every input is a view into a larger flat buffer with GUARD elements of NaN (0xFF for mask bytes)
on both sides; every output (y, dx, dw, stats) a view between guards holding SENT.  GUARD elements are a
multiple of 16 bytes in every dtype, so the views keep the kernels' alignment.  y and dx are pre-filled
with NaN unless the case accumulates onto old integer contents; the statistics with non-zero integers
that the oracle adds.

The oracle is a float64 loop over taps written from the definitions in igemm.h and the ops.conv_*
docstrings (forward: gather from the padded source; data gradient: scatter of dY . W[tap] to
(oy * stride - pad + kh, ox * stride - pad + kw), with no notion of phases; weight gradient: one
tensordot per tap).  It shares no code with the conv2d / conv2d_input / conv2d_weight CPU paths.
"""
import dataclasses
import zlib

import numpy as np
import torch

from dtfe import ops

GUARD = 64
SENT = -512.0
UNIT_CAP = 256
UNIT_LADDER = ((2, 2), (2, 1), (1, 1))   # (max|source|, max|weight|)
ROUNDED_LADDER = (2, 3, 5, 7)
LIMIT = float(2 ** 24)
KNOBS = ("DTFE_IG_TILE", "DTFE_IG_SPLIT", "DTFE_IG_WSPLIT", "DTFE_IG_W3")


# --------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    """One launch.  kind "fwd": x [B][H][W][C] * w [Cout][KH][KW][C] -> y; "dgrad": dy [B][OH][OW][Cout] *
    wt [C][KH][KW][Cout] -> dx [B][H][W][C]; "wgrad": dy, x -> dw [Cout][KH][KW][C] += scale * sum.
    tile / split / wsplit / w3: the DTFE_IG_* knobs (None: unset)."""
    kind: str
    H: int
    W: int
    C: int
    Cout: int
    KH: int = 1
    KW: int = 1
    stride: int = 1
    pad: int = 0
    B: int = 2
    regime: str = "unit"
    tile: str = None
    split: int = None
    wsplit: int = None
    w3: int = None
    stats: bool = False        # fwd: BatchNorm statistics of y
    accumulate: bool = False   # dgrad: dx += dX
    acc_src: bool = False      # dgrad: dx = dX + src * bit
    bn: str = ""               # dgrad: BN-backward statistics; "none" | "relu_x" | "relu_y" (the act and its mask source)
    scale: float = 1.0         # wgrad
    free: int = 0              # fwd 1x1: only ``free`` channels do not cancel in pairs (keeps |y| small)

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())

    @property
    def OH(self):
        return (self.H + 2 * self.pad - self.KH) // self.stride + 1

    @property
    def OW(self):
        return (self.W + 2 * self.pad - self.KW) // self.stride + 1

    @property
    def geom(self):
        return dict(B=self.B, H=self.H, W=self.W, C=self.C, Cout=self.Cout, OH=self.OH, OW=self.OW, KH=self.KH,
                    KW=self.KW, stride=self.stride, pad=self.pad)

    @property
    def env(self):
        vals = (self.tile, self.split, self.wsplit, self.w3)
        return {k: str(v) for k, v in zip(KNOBS, vals) if v is not None}


def apply_env(monkeypatch, c):
    """The case's knobs and nothing else of DTFE_IG_* (read by the launchers at every launch)."""
    for k in KNOBS:
        if k in c.env:
            monkeypatch.setenv(k, c.env[k])
        else:
            monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------ dispatch, mirrored
def _cdiv(a, b):
    return (a + b - 1) // b


def pick_tile(c, M, N, nphase):
    """pick_tile (igemm.hip): DTFE_IG_TILE when N % BN == 0, else the largest tile with >= 240 workgroups."""
    if c.tile:
        bm, bn = (int(v) for v in c.tile.split("x"))
        if bm in (64, 128) and bn in (64, 128) and N % bn == 0:
            return bm, bn
    for bm, bn in ((128, 128), (128, 64), (64, 64)):
        if N % bn == 0 and _cdiv(M, bm) * (N // bn) * nphase >= 240:
            return bm, bn
    return 64, 64


def dgrad_phases(c):
    """launch_igemm_dgrad's phases before any is dropped: (py, px, RH, RW, ntaps) per output parity class."""
    st, out = c.stride, []
    for py in range(st):
        for px in range(st):
            nt = sum(1 for kh in range(c.KH) for kw in range(c.KW)
                     if (py + c.pad - kh) % st == 0 and (px + c.pad - kw) % st == 0)
            out.append((py, px, (c.H - py + st - 1) // st, (c.W - px + st - 1) // st, nt))
    return out


def gemm_info(c):
    """run_igemm for a forward / data-gradient case: tile, splits, the phases launched, how the statistics run."""
    if c.kind == "fwd":
        N, SC, ostr = c.Cout, c.C, 1
        ph = [(0, 0, c.OH, c.OW, c.KH * c.KW)]
        want_stats, bwd = c.stats, False
    else:
        N, SC, ostr = c.C, c.Cout, c.stride
        ph = dgrad_phases(c)
        if c.accumulate and not c.bn:       # a phase no tap reaches adds nothing: dropped
            ph = [p for p in ph if p[4] > 0]
        want_stats, bwd = bool(c.bn), bool(c.bn)
    nphase = len(ph)
    Mmax = max(c.B * p[2] * p[3] for p in ph)
    if nphase == 1 and bwd:                 # one-phase data gradient: the separate statistics pass
        bwd = False
        fused_ok = False
    else:
        fused_ok = True
    bm, bn = pick_tile(c, Mmax, N, nphase)
    splits = 1
    if nphase == 1 and ostr == 1 and not c.acc_src:   # (a masked accumulation source never splits)
        blocks = _cdiv(Mmax, bm) * (N // bn)
        nk = ph[0][4] * (SC // 64)
        sp = c.split or 0
        if sp <= 0:
            sp = 1
            while blocks * sp < 200 and nk // (sp * 2) >= 6:
                sp *= 2
        splits = max(1, min(sp, nk))
    accum = c.kind == "dgrad" and c.accumulate
    fuse = want_stats and fused_ok and splits == 1 and (bwd or (nphase == 1 and not accum))
    tiles_m = _cdiv(Mmax, bm)
    tiles_all = tiles_m * (nphase if bwd else 1)
    absent = sum(tiles_m - _cdiv(c.B * p[2] * p[3], bm) for p in ph)
    return dict(bm=bm, bn=bn, splits=splits, nphase=nphase, zero=sum(1 for p in ph if p[4] == 0), Mmax=Mmax,
                stat=("fused" if fuse else "pass") if want_stats else "none", tiles=tiles_all,
                chunks=_cdiv(tiles_all, 64), absent=absent)


def reduce_slices(splits, length):
    """launch_wgrad_splits_reduce's S."""
    n4 = (length + 3) // 4
    S = 1
    while S < 16 and S * 2 <= splits and (n4 * S) // 256 < 512:
        S *= 2
    return S


def wgrad_info(c):
    """launch_igemm_wgrad: the all-taps kernel's admission (and use_wgrad3), the m-split arithmetic of both kernels."""
    mode = 2 if c.w3 is None else c.w3
    use3 = mode == 1 or (mode == 2 and c.C <= 64 and c.Cout <= 64)
    length = c.Cout * c.KH * c.KW * c.C
    if (c.KH == 3 and c.KW == 3 and c.stride == 1 and c.pad == 1 and c.OH == c.H and c.OW == c.W and c.W <= 62 and
            (64 // c.W + 2) * (c.W + 2) <= 192 and use3):
        R = 64 // c.W
        kpi = _cdiv(c.H, R)
        tiles = (c.Cout // 64) * (c.C // 64)
        T = c.B * kpi
        sp = c.wsplit or 0
        if sp <= 0:
            sp = max(1, min(_cdiv(192, tiles), T // 4))
            sp = max(1, min(sp, (40 << 20) // (length * 4)))
        sp = min(sp, T)
        info = dict(kern="w3", splits=sp, T=T, R=R, kpi=kpi)
    else:
        bm = 128 if c.Cout % 128 == 0 else 64
        bn = 128 if c.C % 128 == 0 else 64
        tiles = (c.Cout // bm) * c.KH * c.KW * (c.C // bn)
        M = c.B * c.OH * c.OW
        sp = c.wsplit or 0
        if sp <= 0:
            sp = max(1, min(_cdiv(192, tiles), (M + 255) // 256))
            sp = max(1, min(sp, (32 << 20) // (length * 4)))
        mchunk = _cdiv(_cdiv(M, sp), 64) * 64
        sp = _cdiv(M, mchunk)
        info = dict(kern="tap%dx%d" % (bm, bn), splits=sp, mchunk=mchunk, M=M)
    sp = info["splits"]
    info["S"] = reduce_slices(sp, length) if sp > 1 else 0
    info["unrolled"] = sp > 1 and sp > 7 * info["S"]   # slice 0 takes the 8-way unrolled trip at least once
    return info


def info(c):
    return wgrad_info(c) if c.kind == "wgrad" else gemm_info(c)


def path(c):
    """The name of what the case's launch reaches, from the mirrored host conditions (nothing observes which
    kernel really ran: a dispatch change keeps a case passing under its old name until this mirror follows).
      fwd|dgrad : BMxBN : s<k-splits> : p<phases launched>z<of them with zero taps> : none|fused|pass
      wgrad : w3|tap<BM>x<BN> : s<m-splits> : r<reduce S, 0 = no reduce>[u = its 8-way unrolled loop runs]"""
    i = info(c)
    if c.kind == "wgrad":
        return "wgrad:%s:s%d:r%d%s" % (i["kern"], i["splits"], i["S"], "u" if i["unrolled"] else "")
    return "%s:%dx%d:s%d:p%dz%d:%s" % (c.kind, i["bm"], i["bn"], i["splits"], i["nphase"], i["zero"], i["stat"])


def instantiations(c):
    """The kernel instantiations the case's launch runs (names as in igemm.hip)."""
    i = info(c)
    if c.kind == "wgrad":
        k = "igemm_wgrad3_kernel" if i["kern"] == "w3" else "igemm_wgrad_kernel<%s>" % i["kern"][3:].replace("x", ",")
        return {k} | ({"wgrad_splits_reduce_kernel<%d>" % i["S"]} if i["S"] else set())
    bb = c.kind == "dgrad" and i["stat"] == "fused"
    out = {"igemm_kernel<%d,%d,%s>" % (i["bm"], i["bn"], "BB" if bb else "-")}
    if i["splits"] > 1:
        out.add("splitk_to_bf16_kernel")
    if i["stat"] == "fused":
        out.add("bn_part_fold")
    return out


# every instantiation the launchers of igemm.hip can select (all are reached; NST = 2 and MINB = 2 are
# the only values launch_ig passes, BKW = 32 / NS = 4 / MINB = 2 the only ones launch_igemm_wgrad passes)
INSTANTIATIONS = tuple(
    ["igemm_kernel<%d,%d,%s>" % (bm, bn, bb) for bm in (64, 128) for bn in (64, 128) for bb in ("-", "BB")] +
    ["splitk_to_bf16_kernel", "bn_part_fold", "igemm_wgrad3_kernel"] +
    ["igemm_wgrad_kernel<%d,%d>" % (bm, bn) for bm in (64, 128) for bn in (64, 128)] +
    ["wgrad_splits_reduce_kernel<%d>" % s for s in (1, 2, 4, 8, 16)])


# --------------------------------------------------------------------------- buffers
_DT = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}


class Built:
    """The CPU buffers of one case: ``bufs[name]`` flat, guards included; ``shape[name]`` of the logical view
    at [GUARD, GUARD + numel); ``log[name]`` the logical values as stored (float64 / uint8)."""

    def __init__(self, case):
        self.case = case
        self.bufs, self.shape, self.log, self.outputs = {}, {}, {}, []
        self.rung = None
        self._ref = {}

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


def _fill(b, hs, hw):
    c = b.case
    rng = np.random.default_rng(c.seed)
    nan = float("nan")
    if c.kind == "fwd":
        x = _ints(rng, (c.B, c.H, c.W, c.C), hs)
        w = _ints(rng, (c.Cout, c.KH, c.KW, c.C), hw)
        if c.free:   # channels free.. in pairs (2i, 2i+1): equal sources, opposite weights - their terms cancel
            assert c.KH == c.KW == 1 and (c.C - c.free) % 2 == 0
            x[..., c.free + 1::2] = x[..., c.free::2]
            w[..., c.free + 1::2] = -w[..., c.free::2]
        b.put("x", x, "bf16", nan)
        b.put("w", w, "bf16", nan)
        b.put("y", np.full((c.B, c.OH, c.OW, c.Cout), nan), "bf16", SENT, output=True)
        if c.stats:
            b.put("stats", _ints(rng, (2 * c.Cout,), 3), "f32", SENT, output=True)
    elif c.kind == "dgrad":
        b.put("dy", _ints(rng, (c.B, c.OH, c.OW, c.Cout), hs), "bf16", nan)
        b.put("wt", _ints(rng, (c.C, c.KH, c.KW, c.Cout), hw), "bf16", nan)
        xs = (c.B, c.H, c.W, c.C)
        old = _ints(rng, xs, 3 if c.regime == "unit" else 2 * hs)
        if c.acc_src:
            assert c.accumulate and c.stride == 1
            b.put("src", old, "bf16", nan)
            keep = rng.integers(0, 2, size=(c.B * c.H * c.W, c.C)).astype(np.uint8)
            b.put("bits", np.packbits(keep, axis=1, bitorder="little").reshape(-1), "u8", 0xFF)
        b.put("dx", old if (c.accumulate and not c.acc_src) else np.full(xs, nan), "bf16", SENT, output=True)
        if c.bn:
            b.put("bn_x", _ints(rng, xs, 3), "bf16", nan)
            if c.bn == "relu_y":
                b.put("bn_y", _ints(rng, xs, 2), "bf16", nan)
            b.put("bn_mean", rng.integers(-1, 2, size=(c.C,)).astype(np.float64), "f32", nan)
            b.put("bn_invstd", rng.choice([0.5, 1.0, 2.0], size=(c.C,)), "f32", nan)
            b.put("bn_gamma", _ints(rng, (c.C,), 2), "f32", nan)
            b.put("bn_beta", rng.integers(-2, 3, size=(c.C,)) + 0.25, "f32", nan)
            b.put("bn_stats", _ints(rng, (2 * c.C,), 3), "f32", SENT, output=True)
    else:
        b.put("dy", _ints(rng, (c.B, c.OH, c.OW, c.Cout), hs), "bf16", nan)
        b.put("x", _ints(rng, (c.B, c.H, c.W, c.C), hw), "bf16", nan)
        b.put("dw", _ints(rng, (c.Cout, c.KH, c.KW, c.C), 3), "f32", SENT, output=True)


def build(c):
    """CPU buffers of one case (deterministic in the case), on the rung of its regime's ladder that meets the
    regime's condition (the last rung if none does: ``conditions`` then fails)."""
    if c.kind == "wgrad":
        ladder = ((2, 2),)
    elif c.regime == "unit":
        ladder = UNIT_LADDER[-1:] if c.free else UNIT_LADDER
    else:
        ladder = tuple((h, h) for h in ROUNDED_LADDER)
    for rung in ladder:
        b = Built(c)
        b.rung = rung
        _fill(b, *rung)
        if c.kind == "wgrad":
            break
        ref, i = oracle(b)
        if (i["max_abs"] <= UNIT_CAP) if c.regime == "unit" else (i["ties_up"] and i["ties_down"]):
            if not c.stats or _stats_bound(c, ref) + 3 < LIMIT:
                break
    return b


# --------------------------------------------------------------------------- oracle
def rne_bf16(v, trunc=False):
    """float64 -> the nearest bf16 value, ties to even (``trunc``: toward zero), as float64.  The finite inputs
    are multiples of 1/4 below 2^24 in magnitude, so the step through fp32 is exact; NaN stays NaN."""
    nan = np.isnan(v)
    f = np.ascontiguousarray(np.where(nan, 0.0, v), dtype=np.float32)
    assert (f.astype(np.float64) == np.where(nan, 0.0, v)).all()
    u = f.view(np.uint32).astype(np.uint64)
    if not trunc:
        u = u + 0x7FFF + ((u >> 16) & 1)
    u = (u & 0xFFFF0000).astype(np.uint32)
    return np.where(nan, np.nan, u.view(np.float32).astype(np.float64))


def _ties(v):
    """(ties RNE moves up in magnitude, ties it moves down, values that are not exact in bf16)."""
    u = np.ascontiguousarray(v[~np.isnan(v)], dtype=np.float32).view(np.uint32)
    tie = (u & 0xFFFF) == 0x8000
    up = ((u >> 16) & 1) == 1
    return int((tie & up).sum()), int((tie & ~up).sum()), int(((u & 0xFFFF) != 0).sum())


MUTATIONS = ("drop_tap", "swap_hw", "swap_k", "pad_off", "border", "stats_last_tile", "truncate", "mask_bit_order",
             "old_dx", "phase_offset", "phase_unwritten", "msplit_dropped")
_BIG = 12   # spare zero rows / columns around the padded arrays: every mutated index stays inside


def _swap_hw(s):
    """Source pixel (sy, sx) fetched from flat pixel sy * SH + sx (H where W belongs)."""
    B, SH, SW, C = s.shape
    sy, sx = np.indices((SH, SW))
    idx = (sy * SH + sx) % (SH * SW)
    return s.reshape(B, SH * SW, C)[:, idx.reshape(-1)].reshape(B, SH, SW, C)


def _taps(c, m):
    """(weight tap kh, kw; source offset dh, dw) per tap the (possibly mutated) kernel visits."""
    out = []
    for kh in range(c.KH):
        for kw in range(c.KW):
            if m == "drop_tap" and (kh, kw) == (c.KH - 1, c.KW - 1):      # (1) the last tap is never visited
                continue
            dh, dw = kh, kw
            wh, ww = kh, kw
            if m == "swap_k":                                             # (3)
                if c.KH == c.KW:
                    wh, ww = kw, kh        # the weight tap of the transposed position
                else:
                    t = kh * c.KW + kw     # tap t placed as if the kernel were KW x KH
                    dh, dw = t // c.KH, t % c.KH
            out.append((wh, ww, dh, dw))
    return out


def _source(c, s, m):
    """The source the taps read: H/W swapped (2); every term of its last row missing (5)."""
    if m == "swap_hw":
        s = _swap_hw(s)
    if m == "border":
        s = s.copy()
        s[:, -1] = 0
    return s


def _fwd_sums(c, x, w, m):
    ph, pw = c.pad, c.pad + (1 if m == "pad_off" else 0)                  # (4) the x padding off by one
    s = c.stride
    z = np.zeros((c.B, c.OH, c.OW, c.Cout))
    for wh, ww, dh, dw in _taps(c, m):
        src = _source(c, x, m)
        xp = np.pad(src, ((0, 0), (ph, _BIG), (pw, _BIG), (0, 0)))
        patch = xp[:, dh:dh + (c.OH - 1) * s + 1:s, dw:dw + (c.OW - 1) * s + 1:s, :]
        z += patch @ w[:, wh, ww, :].T
    return z


def _dgrad_sums(c, dy, wt, m):
    ph, pw = c.pad, c.pad + (1 if m == "pad_off" else 0)
    s = c.stride
    full = np.zeros((c.B, c.H + 2 * _BIG + (c.OH - 1) * s, c.W + 2 * _BIG + (c.OW - 1) * s, c.C))
    for wh, ww, dh, dw in _taps(c, m):
        src = _source(c, dy, m)
        full[:, dh:dh + (c.OH - 1) * s + 1:s, dw:dw + (c.OW - 1) * s + 1:s, :] += src @ wt[:, wh, ww, :].T
    return full[:, ph:ph + c.H, pw:pw + c.W, :].copy()


def _wgrad_sums(c, dy, x, m):
    ph, pw = c.pad, c.pad + (1 if m == "pad_off" else 0)
    s = c.stride
    if m == "msplit_dropped":                                             # (12) one m-split's rows never summed
        i = wgrad_info(c)
        dy = dy.copy()
        if i["kern"] == "w3":    # the last split's last k-tile: R output rows of the last image
            dy[-1, (i["kpi"] - 1) * i["R"]:] = 0
        else:
            dy.reshape(-1, c.Cout)[(i["splits"] - 1) * i["mchunk"]:] = 0
    dw = np.zeros((c.Cout, c.KH, c.KW, c.C))
    for wh, ww, dh, dw_ in _taps(c, m):
        src = _source(c, x, m)
        xp = np.pad(src, ((0, 0), (ph, _BIG), (pw, _BIG), (0, 0)))
        patch = xp[:, dh:dh + (c.OH - 1) * s + 1:s, dw_:dw_ + (c.OW - 1) * s + 1:s, :]
        dw[:, wh, ww, :] += np.tensordot(dy, patch, axes=([0, 1, 2], [0, 1, 2]))
    return dw


def _last_tile_rows(M):
    return M % 64 or 64


def _oracle(b, m, split_rounding):
    c = b.case
    L = b.log
    trunc = m == "truncate"                                               # (7)
    ref, inf = {}, {"ties_up": 0, "ties_down": 0, "inexact": 0}

    def note(v):
        u, d, n = _ties(v)
        inf["ties_up"] += u
        inf["ties_down"] += d
        inf["inexact"] += n

    if c.kind == "wgrad":
        s = _wgrad_sums(c, L["dy"], L["x"], m)
        inf["max_sum"] = float(np.abs(s).max())
        ref["dw"] = L["dw"] + c.scale * s
        return ref, inf
    if c.kind == "fwd":
        z = _fwd_sums(c, L["x"], L["w"], m)
        inf["max_sum"] = inf["max_abs"] = float(np.abs(z).max())
        note(z)
        y = rne_bf16(z, trunc)
        ref["y"] = y
        if c.stats:
            rows = y.reshape(-1, c.Cout)
            d = rows - rows[0]
            if m == "stats_last_tile":                                    # (6)
                d = d[:len(d) - _last_tile_rows(len(d))]
            ref["stats"] = L["stats"] + np.concatenate([d.sum(0), (d * d).sum(0)])
        return ref, inf
    z = _dgrad_sums(c, L["dy"], L["wt"], m)
    inf["max_sum"] = cap = float(np.abs(z).max())
    if c.accumulate:
        if c.acc_src:
            bits = L["bits"].reshape(-1, c.C // 8)
            keep = np.unpackbits(bits, axis=1, bitorder="big" if m == "mask_bit_order" else "little")   # (8)
            old = L["src"] * keep.reshape(z.shape)
            if m == "old_dx":                                             # (9)
                old = L["dx"]
        else:
            old = L["dx"]
        split = gemm_info(c)["splits"] > 1 if split_rounding is None else split_rounding
        if not split:      # the tile is stored as bf16 in LDS, then the old value is added
            note(z)
            z = rne_bf16(z, trunc)
        z = z + old
        cap = max(cap, float(np.abs(np.nan_to_num(z)).max()))
    note(z)
    dx = rne_bf16(z, trunc)
    inf["max_abs"] = cap
    if c.stride == 2:
        if m == "phase_offset":                                           # (10) phase (0, 0) computed with phase (0, 1)'s tap offsets
            n = dx[:, 0::2, 1::2].shape[2]
            dx = dx.copy()
            dx[:, 0::2, 0:2 * n:2] = dx[:, 0::2, 1::2]
        if m == "phase_unwritten":                                        # (11) a zero-tap phase keeps the old contents
            dx = dx.copy()
            for py, px, _, _, nt in dgrad_phases(c):
                if nt == 0:
                    dx[:, py::2, px::2] = L["dx"][:, py::2, px::2]
    ref["dx"] = dx
    if c.bn:
        g = dx.reshape(-1, c.C)
        x = L["bn_x"].reshape(-1, c.C)
        if c.bn == "relu_x":
            sc = L["bn_gamma"] * L["bn_invstd"]
            g = np.where(x * sc + (L["bn_beta"] - L["bn_mean"] * sc) > 0, g, 0.0)
        elif c.bn == "relu_y":
            g = np.where(L["bn_y"].reshape(-1, c.C) > 0, g, 0.0)
        t = g * (x - L["bn_mean"]) * L["bn_invstd"]
        inf["bn_abs"] = float(max(np.abs(g).sum(0).max(), np.abs(t).sum(0).max()))
        if m == "stats_last_tile":
            n = len(g) - _last_tile_rows(len(g))
            g, t = g[:n], t[:n]
        ref["bn_stats"] = L["bn_stats"] + np.concatenate([g.sum(0), t.sum(0)])
    return ref, inf


def oracle(b, mutate=None, split_rounding=None):
    """({output name: exact expected logical values}, info) of the case.  ``mutate``: one of MUTATIONS - what a
    wrong kernel would give (numbered (1)-(12) in the code).  ``split_rounding``: None = as the mirrored
    dispatch says; False / True = an accumulating case rounded as the unsplit epilogue / the split-K combine."""
    key = (mutate, split_rounding)
    if key not in b._ref:
        out = _oracle(b, mutate, split_rounding)
        if mutate is not None:
            return out
        b._ref[key] = out      # (callers leave the arrays as they are)
    return b._ref[key]


def mutations(b):
    """The mutations that apply to the case.
    drop_tap, pad_off, border: every case.  swap_hw: the source's H != W.  swap_k: more than one tap.
    stats_last_tile: fwd stats / dgrad bn.  truncate: something stored is not exact in bf16.
    mask_bit_order, old_dx: acc_src.  phase_offset: stride-2 dgrad.  phase_unwritten: a non-accumulating
    stride-2 dgrad with a zero-tap phase.  msplit_dropped: wgrad with more than one m-split."""
    c = b.case
    inf = oracle(b)[1]
    out = ["drop_tap", "pad_off", "border"]
    sh, sw = (c.OH, c.OW) if c.kind == "dgrad" else (c.H, c.W)
    if sh != sw:
        out.append("swap_hw")
    if c.KH * c.KW > 1:
        out.append("swap_k")
    if c.stats or c.bn:
        out.append("stats_last_tile")
    if c.kind != "wgrad" and inf["inexact"]:
        out.append("truncate")
    if c.acc_src:
        out += ["mask_bit_order", "old_dx"]
    if c.kind == "dgrad" and c.stride == 2:
        out.append("phase_offset")
        if not c.accumulate and any(p[4] == 0 for p in dgrad_phases(c)):
            out.append("phase_unwritten")
    if c.kind == "wgrad" and wgrad_info(c)["splits"] > 1:
        out.append("msplit_dropped")
    return out


def _fold_bound(rows, bm):
    """The largest magnitude any intermediate of the fused forward statistics can take with tiles of ``bm`` rows:
    the per-tile sums, bn_part_fold's chunk fold (64 tiles onto the chunk's first K) and its fold of the chunks
    onto row 0's K, every term replaced by its absolute value."""
    M = len(rows)
    worst = 0.0
    K0 = rows[0]
    Sa = Qa = 0.0
    for c0 in range(0, M, 64 * bm):
        Kc = rows[c0]
        Sc = Qc = 0.0
        for t0 in range(c0, min(M, c0 + 64 * bm), bm):
            d = np.abs(rows[t0:t0 + bm] - rows[t0])
            n = len(d)
            a, q = d.sum(0), (d * d).sum(0)
            dk = np.abs(rows[t0] - Kc)
            Sc = Sc + a + n * dk
            Qc = Qc + q + 2 * dk * a + n * dk * dk
        n = min(M, c0 + 64 * bm) - c0
        dk = np.abs(Kc - K0)
        Sa = Sa + Sc + n * dk
        Qa = Qa + Qc + 2 * dk * Sc + n * dk * dk
        worst = max(worst, float(np.max(Qc)), float(np.max(Sc)))
    return max(worst, float(np.max(Sa)), float(np.max(Qa)))


def _stats_bound(c, ref):
    rows = ref["y"].reshape(-1, c.Cout)
    return max(_fold_bound(rows, bm) for bm in (64, 128))


def conditions(b):
    """Assert the data conditions of the case's regime on its reference (bounds by sums of absolute values)."""
    c = b.case
    ref, inf = oracle(b)
    hs, hw = b.rung
    for name in ("x", "w", "dy", "wt", "src", "bn_x", "bn_y", "bn_gamma"):
        if name in b.log:
            assert (b.log[name] != 0).all() and (b.log[name] == np.round(b.log[name])).all(), (c, name)
    terms = c.B * c.OH * c.OW if c.kind == "wgrad" else c.KH * c.KW * (c.C if c.kind == "fwd" else c.Cout)
    assert terms * hs * hw + 4 * max(hs, 3) < LIMIT, c        # sum |terms| + |old value|: every partial sum is exact
    if c.kind == "wgrad":
        assert c.scale in (0.25, 0.5, 1.0) and (b.log["dw"] != 0).all(), c
        assert 4 * (inf["max_sum"] + 3) < LIMIT, (c, inf)    # scale * sum + old is a multiple of 1/4 below 2^24
        return
    if c.regime == "unit":
        assert inf["max_abs"] <= UNIT_CAP and inf["inexact"] == 0, (c, inf)
    else:
        assert inf["ties_up"] > 0 and inf["ties_down"] > 0, (c, inf)
    if c.stats:
        assert _stats_bound(c, ref) + 3 < LIMIT, (c, _stats_bound(c, ref))   # (+ 3: the pre-filled statistics)
    if c.bn:
        assert ((b.log["bn_beta"] * 4) % 4 == 1).all() and set(np.unique(b.log["bn_invstd"])) <= {0.5, 1.0, 2.0}, c
        assert 4 * (inf["bn_abs"] + 3) < LIMIT, (c, inf)     # multiples of 1/4


# --------------------------------------------------------------------------- run and check
def launch(b, dev):
    """Launch the case of ``b`` = build(case) on ``dev`` ("cuda": the HIP kernels under the DTFE_IG_* knobs in
    force, "cpu": the project's fp32 reference path); returns the whole buffers on ``dev``."""
    c = b.case
    t = {k: v.clone().to(dev) for k, v in b.bufs.items()}
    v = lambda name: view(t, b, name)  # noqa: E731
    if c.kind == "fwd":
        ops.conv_fwd(v("x"), v("w"), None, v("y"), None, c.geom, act=ops.ACT_NONE, stats=v("stats"))
    elif c.kind == "dgrad":
        bn = None
        if c.bn:
            bn = (v("bn_x"), v("bn_y"), v("bn_mean"), v("bn_invstd"), v("bn_gamma"), v("bn_beta"), v("bn_stats"),
                  ops.ACT_NONE if c.bn == "none" else ops.ACT_RELU)
        ops.conv_dgrad(v("dy"), v("wt"), v("dx"), c.geom, accumulate=c.accumulate, bn_bwd=bn,
                       acc_src=(v("src"), v("bits")) if c.acc_src else None)
    else:
        ops.conv_wgrad(v("dy"), v("x"), v("dw"), None, c.geom, c.scale)
    return t


def run(b, dev):
    """launch + fetch: the whole buffers of ``b``, guards included, on the CPU."""
    return {k: x.cpu() for k, x in launch(b, dev).items()}


def as_buffers(b, ref):
    """Logical outputs (an oracle's) laid into sentinel-guarded buffers, as ``run`` returns them."""
    got = {}
    for name in b.outputs:
        buf = b.bufs[name].clone()
        n = buf.numel() - 2 * GUARD
        buf[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(ref[name])).to(buf.dtype).reshape(-1)
        got[name] = buf
    return got


def _first_diff(c, name, a, r):
    diff = a != r
    i = tuple(int(k) for k in np.argwhere(diff)[0])
    return "%s [%s]: %s%s = %r, expected %r (%d of %d elements differ)" % (
        c, path(c), name, list(i), a[i].item(), r[i].item(), int(diff.sum()), diff.size)


def check(b, got, ref=None):
    """Assert the sentinels untouched, no NaN in the logical outputs (an unwritten element, or a stray read of
    a guard) and every value bit-equal to the oracle's."""
    c = b.case
    ref = ref or oracle(b)[0]
    for name in b.outputs:
        buf = got[name]
        n = buf.numel() - 2 * GUARD
        guards = torch.cat([buf[:GUARD], buf[GUARD + n:]])
        logical = buf[GUARD:GUARD + n].view(b.shape[name])
        r = ref[name]
        assert tuple(r.shape) == b.shape[name], (c, name, r.shape)
        assert (guards == SENT).all(), "%s [%s]: %s written outside its logical elements" % (c, path(c), name)
        assert not torch.isnan(logical).any(), "%s [%s]: NaN in %s (%d elements: unwritten, or poisoned by a stray read)" % (
            c, path(c), name, int(torch.isnan(logical).sum()))
        assert not np.isnan(r).any(), (c, name, "NaN in the reference")
        want = torch.from_numpy(np.ascontiguousarray(r)).to(logical.dtype)
        assert (want.double().numpy() == r).all(), "%s: the reference of %s is not exact in %s" % (c, name, logical.dtype)
        if not torch.equal(logical, want):
            raise AssertionError(_first_diff(c, name, logical.double().numpy(), r))


# --------------------------------------------------------------------------- case groups
def _geometry(kind, **kw):
    """The geometry set, always H != W: 1x1 s1 64->64 at 5x7 (70 rows: a partial second 64-row tile), 1x1 s2
    128->256 at 9x6, 3x3 s1 pad 1 64->128 at 6x10, 3x3 s2 pad 1 128->64 at 7x12, 3x3 pad 0 64->64 at 6x5,
    1x3 and 3x1 at pad 0, 2x2 stride 2 pad 0 (four one-tap dgrad phases)."""
    C = lambda **g: Case(kind=kind, **{**g, **kw})  # noqa: E731
    return [
        C(H=5, W=7, C=64, Cout=64),
        C(H=9, W=6, C=128, Cout=256, stride=2),
        C(H=6, W=10, C=64, Cout=128, KH=3, KW=3, pad=1),
        C(H=7, W=12, C=128, Cout=64, KH=3, KW=3, stride=2, pad=1),
        C(H=6, W=5, C=64, Cout=64, KH=3, KW=3),
        C(H=6, W=7, C=64, Cout=64, KH=1, KW=3),
        C(H=7, W=5, C=64, Cout=64, KH=3, KW=1),
        C(H=6, W=10, C=64, Cout=64, KH=2, KW=2, stride=2),
    ]


TILES = ("64x64", "128x64", "64x128", "128x128")


def _with_tiles(cases):
    """Each case under every tile its output channel count allows."""
    out = []
    for c in cases:
        n = c.Cout if c.kind == "fwd" else c.C
        out += [dataclasses.replace(c, tile=t) for t in TILES if n % int(t.split("x")[1]) == 0]
    return out


def fwd_cases():
    F = lambda **g: Case(kind="fwd", **g)  # noqa: E731
    geo = _geometry("fwd")
    deep = dict(H=7, W=7, C=512, Cout=128, KH=3, KW=3, pad=1)
    return geo + _with_tiles(geo) + [dataclasses.replace(c, stats=True) for c in geo] + [
        F(regime="rounded", **deep),                                    # split-K on auto: 8 splits
        F(regime="rounded", split=1, **deep),
        F(regime="rounded", split=1, tile="128x128", **deep),
        F(H=5, W=7, C=640, Cout=64, split=3),                           # 10 k-tiles over 3 splits: 3, 3, 4
        F(H=5, W=7, C=128, Cout=64, split=5),                           # clipped to the 2 k-tiles
        F(H=5, W=7, C=640, Cout=64, split=3, stats=True),               # split-K: the statistics take the separate pass
        F(H=48, W=48, C=64, Cout=64, tile="64x64", stats=True),         # 72 tiles, 2 chunks
        F(H=48, W=48, C=64, Cout=128, tile="128x128", stats=True),      # 36 tiles of 128 rows
        F(H=257, W=256, C=64, Cout=64, tile="64x64", stats=True, free=4),   # 2056 tiles, 33 chunks: stage 2's second trip
    ]


def dgrad_cases():
    D = lambda **g: Case(kind="dgrad", **g)  # noqa: E731
    geo = _geometry("dgrad")
    acc = [dataclasses.replace(c, accumulate=True) for c in geo]
    deep = dict(H=7, W=7, C=128, Cout=512, KH=3, KW=3, pad=1, regime="rounded")
    s3 = dict(H=7, W=7, C=64, Cout=128, KH=3, KW=3, pad=1)             # 18 k-tiles, 2 workgroups: 2 splits on auto
    return geo + acc + _with_tiles([geo[2], geo[3], acc[2], acc[3]]) + [
        D(**deep), D(accumulate=True, **deep),                          # auto split-K: RNE(S + old)
        D(split=1, **deep), D(split=1, accumulate=True, **deep),        # unsplit: RNE(RNE(S) + old)
        D(H=6, W=10, C=64, Cout=128, KH=3, KW=3, pad=1, split=2, accumulate=True),
        D(accumulate=True, **s3),
        # masked accumulation source: unsplit, DTFE_IG_SPLIT=2 on a 1x1, the automatic split of a 3x3
        D(H=5, W=7, C=64, Cout=64, accumulate=True, acc_src=True),
        D(H=6, W=10, C=128, Cout=64, KH=3, KW=3, pad=1, split=1, accumulate=True, acc_src=True),
        D(H=6, W=10, C=128, Cout=64, KH=3, KW=3, pad=1, split=1, tile="128x128", accumulate=True, acc_src=True),
        D(H=7, W=7, C=512, Cout=128, split=2, accumulate=True, acc_src=True),
        D(accumulate=True, acc_src=True, **s3),
        D(accumulate=True, acc_src=True, **{**deep, "C": 64}),
        D(split=1, accumulate=True, acc_src=True, **{**deep, "C": 64}),
    ]


def dgrad_stats_cases():
    D = lambda **g: Case(kind="dgrad", **g)  # noqa: E731
    s2 = dict(C=128, Cout=64, KH=3, KW=3, stride=2, pad=1, B=6)        # unequal phase grids: absent tiles
    out = []
    for hw in (dict(H=7, W=12), dict(H=9, W=9)):
        out += _with_tiles([D(bn="relu_x", **hw, **s2)])
    out += [
        D(H=7, W=12, bn="none", **s2), D(H=7, W=12, bn="relu_y", **s2),
        D(H=7, W=12, bn="relu_x", accumulate=True, **s2), D(H=9, W=9, bn="relu_y", accumulate=True, tile="128x64", **s2),
        D(H=9, W=6, C=128, Cout=256, stride=2, bn="relu_x"),            # 1x1 s2: the zero-tap phases stay, write zeros
        D(H=9, W=6, C=128, Cout=256, stride=2, bn="none", accumulate=True),
        D(H=6, W=10, C=64, Cout=64, KH=2, KW=2, stride=2, bn="relu_y"),
    ]
    one = dict(H=6, W=10, C=64, Cout=128, KH=3, KW=3, pad=1)           # one phase: the separate pass
    out += [D(bn=a, **one) for a in ("none", "relu_x", "relu_y")] + [
        D(bn="relu_x", accumulate=True, **one), D(bn="none", split=1, **one), D(H=5, W=7, C=64, Cout=64, bn="relu_x")]
    return out


def wgrad_tap_cases():
    Wc = lambda **g: Case(kind="wgrad", w3=0, **g)  # noqa: E731
    out = [Wc(H=6, W=10, C=ci, Cout=co, KH=3, KW=3, pad=1, scale=0.5) for co in (64, 128) for ci in (64, 128)]  # M = 120
    out += [dataclasses.replace(c, w3=0, scale=s) for c, s in zip(_geometry("wgrad"), (1.0, 0.5, 0.25, 1.0, 0.5, 0.25, 1.0, 0.5))]
    sweep = dict(B=10, H=16, W=16, C=64, Cout=64, KH=3, KW=3, pad=1, scale=0.25)
    out += [Wc(wsplit=s, **sweep) for s in (1, 2, 3, 5, 9, 17, 40)] + [Wc(**sweep)]
    big = dict(C=512, Cout=128, KH=3, KW=3, pad=1, scale=0.5)         # 589824 floats: the reduce stays at S = 1
    out += [Wc(H=7, W=7, wsplit=2, **big), Wc(B=10, H=8, W=8, wsplit=10, **big)]
    return out


def wgrad_w3_cases():
    Wc = lambda **g: Case(kind="wgrad", w3=1, KH=3, KW=3, pad=1, **g)  # noqa: E731
    out = []
    for w in (2, 7, 13, 31, 32, 33, 62):
        out += [Wc(H=5, W=w, C=64, Cout=64, wsplit=1, scale=0.5), Wc(H=5, W=w, C=64, Cout=64, scale=0.25)]
    out += [
        Wc(H=5, W=7, C=64, Cout=64, wsplit=50),                         # T = 2: clipped
        Wc(H=5, W=62, C=64, Cout=128, wsplit=50, scale=0.5),            # T = 10: clipped, two co tiles
        Wc(B=9, H=5, W=13, C=128, Cout=64, scale=0.5),                  # auto: 4 splits of 18 k-tiles
        Case(kind="wgrad", H=5, W=13, C=64, Cout=64, KH=3, KW=3, pad=1),   # DTFE_IG_W3 unset: 64 -> 64 is admitted
        Wc(H=5, W=63, C=64, Cout=64),                                   # W > 62: the per-tap kernel
        dataclasses.replace(Wc(H=6, W=62, C=64, Cout=64), pad=0),       # pad 0: the per-tap kernel
    ]
    return out


GROUPS = {
    "fwd": fwd_cases,
    "dgrad": dgrad_cases,
    "dgrad_stats": dgrad_stats_cases,
    "wgrad_tap": wgrad_tap_cases,
    "wgrad_w3": wgrad_w3_cases,
}
