"""Cases, float64 oracle and derived error bound for the dense MFMA GEMM (tiles 0-4 of ``ops.gemm``).

Shared by tests/test_gemm_dense_paths_gpu.py (the kernels) and tests/test_gemm_dense_oracle_cpu.py
(the oracle itself: agreement with the project's fp32 CPU reference, and sensitivity).

Inputs: magnitudes uniform in [0.5, 1.5] with a random sign, rounded to the operand's dtype; the
oracle works from the values as stored.  No product is near zero: a k-term that goes missing or is
counted twice moves an output element by at least 0.25 * |alpha|.

Guarding: every operand, bias and aux tensor is a view into a larger NaN-filled buffer (NaN in the
padding between the logical width and the leading dimension, and GUARD elements of NaN before and
after), so an element read outside the logical matrix and used poisons the output.  Outputs are
pre-filled with NaN where they must be written (with the old values where the epilogue reads them:
beta, atomic) and with the sentinel SENT everywhere else, which must survive.

Bound (per element, derived - never tuned):

    |got - ref| <= (K + splits + 8) * 2^-24 * |alpha| * (|A| . |B|^T)[m, n] + out_rounding

the worst-case bound of a K-term fp32 dot product summed in any order (K product roundings for fp32
operands, K - 1 additions, splits - 1 more for the split-K combine), with 8 further roundings of
slack for the epilogue (alpha, bias, act'(aux) = up to 3, beta = 2, atomic adds).  Those epilogue
roundings act on alpha * acc plus the bias / beta * old / old addends, not on |alpha| * |A|.|B|^T
alone, so ``oracle`` asserts for every case that the slack really covers them (``_slack_ok``).
out_rounding is 2^-8 * |ref| for a bf16 destination and 2^-24 * |ref| for fp32.  Through an
activation the error e of the pre-activation z becomes e * sup|act'| over [z - e, z + e] (ReLU: 1,
sigmoid / tanh: act' at max(|z| - e, 0), both derivatives fall with |z|) plus ACT_ALLOW * |act(z)|, the
device function's own error (module docstring of test_gemm_dense_paths_gpu.py); through act'(aux)
it is scaled by |act'(aux)| <= 1.
"""
import dataclasses
import itertools
import zlib

import numpy as np
import torch

from dtfe import ops

U = 2.0 ** -24          # fp32 unit roundoff
U_BF16 = 2.0 ** -8      # bf16 unit roundoff (8 significant bits)
GUARD = 16              # elements of NaN / sentinel around every buffer (>= 32 B, a multiple of 16 B)
SENT = -512.0           # exact in bf16 and fp32, far outside every result
TILE_DIMS = {t: ops.TILE_DIMS[t] for t in range(5)}
KT = ops.GEMM_KTILE
LAYOUTS = list(itertools.product([ops.KMAJ, ops.RMAJ], [ops.KMAJ, ops.RMAJ]))
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}

# relative error allowance of the device's sigmoid (1 / (1 + __expf(-x))) and tanhf on their fp32 argument:
# 4 x the largest value measured over this file's cases, 4.58e-7 (2^-21.06) and 1.32e-7 (2^-22.85), the
# fp32 store's rounding included (module docstring of test_gemm_dense_paths_gpu.py)
ACT_ALLOW = {ops.ACT_NONE: 0.0, ops.ACT_RELU: 0.0, ops.ACT_SIGMOID: 4 * 4.58e-7, ops.ACT_TANH: 4 * 1.32e-7}


def prefetch_depth(tile, dtype):
    """Host mirror of gemm_core.h PrefetchDepth<T, Cfg>::VALUE for the dense tiles (k-tile 64, 256 threads)."""
    bm, bn = TILE_DIMS[tile]
    slot_regs = 4 * ((bm + bn) * KT * (2 if dtype == "bf16" else 4) // 16 // 256)
    return 4 if slot_regs <= 24 else (3 if slot_regs <= 32 else 1)


def expected_loop(tile, dtype, nk):
    """The k-loop gemm_mainloop picks for an interior workgroup whose nk k-tiles are all whole
    (all_fast): the deep ring needs D > 1 and nk > 2."""
    d = prefetch_depth(tile, dtype)
    return "deep%d" % d if d > 1 and nk > 2 else "fast"


@dataclasses.dataclass(frozen=True)
class Case:
    tile: int
    dtype: str                 # operand dtype: "bf16" | "f32"
    amode: int
    bmode: int
    M: int
    N: int
    K: int
    ld: str = "tight"          # operand leading dims: "tight" | "pad8" (next multiple of 8) | "pad3" (never vectorised)
    off: int = 0               # operand views start `off` elements after a 16-B aligned address
    ldc: int = 0               # 0: N
    out_off: int = 0
    out_dtype: str = "f32"
    bias_axis: int = -1        # -1: no bias
    act: int = 0
    alpha: float = 1.0
    beta: float = 0.0
    out2: str = ""             # "" | "f32" | "bf16"
    out2_trans: bool = False
    aux: str = ""              # "" | "f32" | "bf16"
    ld_aux: int = 0
    aux_act: int = 0
    ones: str = ""             # "" | "a" (a_ones_row = M - 1) | "b" (b_ones_row = N - 1), both with bias_out
    atomic: bool = False
    splits: int = 1

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())

    @property
    def ldc_(self):
        return self.ldc or self.N


def _ld(width, how):
    if how == "tight":
        return width
    if how == "pad8":
        return (width + 7) // 8 * 8
    ld = width + 3
    return ld + 1 if ld % 4 == 0 else ld   # no multiple of either vector width


def _values(rng, shape, lo=0.5, hi=1.5, signed=True):
    v = rng.uniform(lo, hi, size=shape)
    if signed:
        v = v * rng.choice([-1.0, 1.0], size=shape)
    return v


def _guarded(logical, dtype, ld, off, fill, tail=0):
    """Flat buffer holding the 2-D float64 ``logical`` at [start + r*ld + c], ``fill`` everywhere else;
    returns (buffer, start, the values as stored in float64)."""
    rows, width = logical.shape
    assert ld >= width and off >= 0
    need = (rows - 1) * ld + width if rows else 0
    start = GUARD + off
    buf = torch.full((start + need + GUARD + tail,), fill, dtype=dtype)
    assert start + (rows - 1) * ld + width <= buf.numel() - GUARD   # every logical element inside, guard after it
    idx = start + (torch.arange(rows).unsqueeze(1) * ld + torch.arange(width).unsqueeze(0))
    buf[idx] = torch.from_numpy(np.ascontiguousarray(logical)).to(dtype)
    return buf, start, buf[idx].double().numpy()


@dataclasses.dataclass
class Built:
    case: Case
    A: torch.Tensor
    a_start: int
    lda: int
    B: torch.Tensor
    b_start: int
    ldb: int
    A_log: np.ndarray          # [M, K] float64 as stored, ones row included
    B_log: np.ndarray          # [N, K]
    out: torch.Tensor
    out_start: int
    out_rows: int
    out_cols: int
    old: np.ndarray = None     # what `out` held where the epilogue reads it (beta / atomic)
    bias: torch.Tensor = None
    bias_start: int = 0
    bias_log: np.ndarray = None
    aux: torch.Tensor = None
    aux_start: int = 0
    aux_log: np.ndarray = None
    out2: torch.Tensor = None
    out2_start: int = 0
    ldc2: int = 0
    bias_out: torch.Tensor = None
    bias_out_old: np.ndarray = None


def build(c):
    """CPU buffers of one case (deterministic in the case)."""
    rng = np.random.default_rng(c.seed)
    dt = DTYPES[c.dtype]
    nan = float("nan")
    ra, rb = c.M - (c.ones == "a"), c.N - (c.ones == "b")   # rows that exist in memory

    def operand(rows, mode):
        logical = _values(rng, (rows, c.K))
        if mode == ops.KMAJ:
            ld = _ld(c.K, c.ld)
            buf, start, stored = _guarded(logical, dt, ld, c.off, nan)
        else:
            ld = _ld(rows, c.ld)
            buf, start, stored = _guarded(logical.T, dt, ld, c.off, nan)
            stored = stored.T
        return buf, start, ld, stored

    A, a_start, lda, A_log = operand(ra, c.amode)
    B, b_start, ldb, B_log = operand(rb, c.bmode)
    if c.ones == "a":
        A_log = np.concatenate([A_log, np.ones((1, c.K))], 0)
    if c.ones == "b":
        B_log = np.concatenate([B_log, np.ones((1, c.K))], 0)
    odt = DTYPES[c.out_dtype]
    ldc = c.ldc_
    assert ldc >= c.N
    reads_old = c.beta != 0.0 or c.atomic
    first = _values(rng, (ra, rb)) if reads_old else np.full((ra, rb), nan)
    out, out_start, old = _guarded(first, odt, ldc, c.out_off, SENT, tail=2 * ldc)
    b = Built(c, A, a_start, lda, B, b_start, ldb, A_log, B_log, out, out_start, ra, rb, old if reads_old else None)
    if c.bias_axis >= 0:
        n = c.N if c.bias_axis == 0 else c.M
        b.bias, b.bias_start, v = _guarded(_values(rng, (1, n)), torch.float32, n, 0, nan)
        b.bias_log = v[0]
    if c.aux:
        if c.aux_act == ops.ACT_RELU:
            y = _values(rng, (c.M, c.N))
        else:  # outputs of the activation whose derivative stays away from 0
            y = _values(rng, (c.M, c.N), 0.2, 0.8, signed=c.aux_act == ops.ACT_TANH)
        b.aux, b.aux_start, b.aux_log = _guarded(y, DTYPES[c.aux], c.ld_aux or ldc, 0, nan)
    if c.out2:
        shape = (c.N, c.M) if c.out2_trans else (c.M, c.N)
        b.ldc2 = shape[1] + 3
        b.out2, b.out2_start, _ = _guarded(np.full(shape, nan), DTYPES[c.out2], b.ldc2, 0, SENT)
    if c.ones:
        n = c.N if c.ones == "a" else c.M
        v = _values(rng, (1, n)) if c.atomic else np.full((1, n), nan)
        b.bias_out, _, v = _guarded(v, torch.float32, n, 0, SENT)
        b.bias_out_old = v[0]
    return b


def run(b, dev, workspace=None):
    """Launch the case on ``dev`` ("cuda": the HIP kernel, "cpu": ops.gemm's fp32 reference path);
    returns the whole output buffers, guards included, on the CPU.  workspace: the (ws, tile_ctr) of a
    ticketed split-K launch on the GPU."""
    c = b.case
    nb = 0 if c.bias_axis < 0 else (c.N if c.bias_axis == 0 else c.M)
    nbo = c.N if c.ones == "a" else c.M
    mv = lambda t: None if t is None else t.clone().to(dev)  # noqa: E731
    A, B, out, bias, aux, out2, bias_out = (mv(t) for t in (b.A, b.B, b.out, b.bias, b.aux, b.out2, b.bias_out))
    kw = {} if workspace is None else {"workspace": workspace}
    ops.gemm(A[b.a_start:], B[b.b_start:], out[b.out_start:], M=c.M, N=c.N, K=c.K, amode=c.amode, lda=b.lda,
             bmode=c.bmode, ldb=b.ldb, ldc=c.ldc_, bias=None if bias is None else bias[b.bias_start:b.bias_start + nb],
             bias_axis=max(c.bias_axis, 0), act=c.act, alpha=c.alpha, beta=c.beta, atomic=c.atomic, splits=c.splits,
             tile=c.tile, aux=None if aux is None else aux[b.aux_start:], ld_aux=c.ld_aux or c.ldc_, aux_act=c.aux_act,
             a_ones_row=c.M - 1 if c.ones == "a" else -1, b_ones_row=c.N - 1 if c.ones == "b" else -1,
             out2=None if out2 is None else out2[b.out2_start:], ldc2=b.ldc2, out2_trans=c.out2_trans,
             bias_out=None if bias_out is None else bias_out[GUARD:GUARD + nbo], **kw)
    return {k: v.cpu() for k, v in (("out", out), ("out2", out2), ("bias_out", bias_out)) if v is not None}


def _act(z, act):
    if act == ops.ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ops.ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-z))
    if act == ops.ACT_TANH:
        return np.tanh(z)
    return z


def _act_grad_from_out(y, act):
    if act == ops.ACT_RELU:
        return (y > 0).astype(np.float64)
    if act == ops.ACT_SIGMOID:
        return y * (1.0 - y)
    if act == ops.ACT_TANH:
        return 1.0 - y * y
    return np.ones_like(y)


def _slack_ok(c, b, aS):
    """The 8 spare roundings of the bound cover this case's epilogue: each multiplication rounds a value of
    at most |alpha| * |A|.|B|^T =: aS (act'(aux) <= 1), each addition one of at most aS plus the addends."""
    muls = (c.alpha != 1.0) + (3 if c.aux else 0) + (c.beta != 0.0)
    adds = 0.0
    if b.bias_log is not None:
        adds += aS + np.abs(b.bias_log).max()
    if c.beta != 0.0:
        adds += aS + 1.5 + abs(c.beta) * np.abs(b.old).max()
    if c.atomic:
        adds += c.splits * (aS + 1.5)
    if c.act in (ops.ACT_SIGMOID, ops.ACT_TANH) and (c.aux or c.beta != 0.0 or c.atomic):
        return False   # e * sup|act'| may shrink to nothing: no rounding of x may follow a saturating act
    return muls * aS + adds <= 8 * aS


def oracle(b, mutate=None):
    """{name: (ref, bound)} in float64 for the outputs "out", "out2", "bias_out" of the case.
    mutate: None | "drop_last" (last k-term missing) | "dup_first" (first k-term twice) - a wrong kernel;
    the bound always belongs to the unmutated reference."""
    c = b.case
    A, B = b.A_log, b.B_log
    acc = A[:, :-1] @ B[:, :-1].T if mutate == "drop_last" else A @ B.T
    if mutate == "dup_first":
        acc = acc + np.outer(A[:, 0], B[:, 0])
    S = np.abs(A) @ np.abs(B).T
    e = (c.K + c.splits + 8) * U * abs(c.alpha) * S
    assert _slack_ok(c, b, abs(c.alpha) * S.min()), c
    res = {}
    if c.ones:
        if c.ones == "a":
            bo, ebo, acc, e = c.alpha * acc[-1], e[-1], acc[:-1], e[:-1]
        else:
            bo, ebo, acc, e = c.alpha * acc[:, -1], e[:, -1], acc[:, :-1], e[:, :-1]
        if c.atomic:
            bo = bo + b.bias_out_old
        res["bias_out"] = (bo, ebo + U * np.abs(bo))
    r_out = U if c.out_dtype == "f32" else U_BF16
    if c.atomic:
        x = b.old + c.alpha * acc
        res["out"] = (x, e + r_out * np.abs(x))
        return res
    z = c.alpha * acc
    if b.bias_log is not None:
        z = z + (b.bias_log[None, :z.shape[1]] if c.bias_axis == 0 else b.bias_log[:z.shape[0], None])
    x = _act(z, c.act)
    if c.act in (ops.ACT_SIGMOID, ops.ACT_TANH):
        zz = np.maximum(np.abs(z) - e, 0.0)
        sup = _act_grad_from_out(_act(zz, c.act), c.act)
        e = e * sup + ACT_ALLOW[c.act] * np.abs(x)
    if c.aux:
        g = _act_grad_from_out(b.aux_log[:x.shape[0], :x.shape[1]], c.aux_act)
        x, e = x * g, e * np.abs(g)
    if c.beta != 0.0:
        x = x + c.beta * b.old
    res["out"] = (x, e + r_out * np.abs(x))
    if c.out2:
        x2, e2 = (x.T, e.T) if c.out2_trans else (x, e)
        res["out2"] = (x2, e2 + (U if c.out2 == "f32" else U_BF16) * np.abs(x2))
    return res


def _split(buf, start, rows, cols, ld):
    """(logical [rows, cols] float64, everything else) of a flat output buffer."""
    idx = start + (torch.arange(rows).unsqueeze(1) * ld + torch.arange(cols).unsqueeze(0))
    rest = torch.ones(buf.numel(), dtype=torch.bool)
    rest[idx.reshape(-1)] = False
    return buf[idx].double().numpy(), buf[rest].double().numpy()


def logical_outputs(b, got):
    """{name: (logical values float64, the rest of the buffer)} of what ``run`` returned."""
    c = b.case
    o = {"out": _split(got["out"], b.out_start, b.out_rows, b.out_cols, c.ldc_)}
    if c.out2:
        rows, cols = (c.N, c.M) if c.out2_trans else (c.M, c.N)
        o["out2"] = _split(got["out2"], b.out2_start, rows, cols, b.ldc2)
    if c.ones:
        n = c.N if c.ones == "a" else c.M
        o["bias_out"] = _split(got["bias_out"], GUARD, 1, n, n)
        o["bias_out"] = (o["bias_out"][0][0], o["bias_out"][1])
    return o


def check(b, got, ref=None):
    """Assert every output of the case within its bound and every sentinel untouched; returns the
    largest err / bound ratio."""
    c = b.case
    ref = ref or oracle(b)
    worst = 0.0
    for name, (val, rest) in logical_outputs(b, got).items():
        r, bound = ref[name]
        assert val.shape == r.shape, (c, name, val.shape, r.shape)
        assert (rest == SENT).all(), "%s: %s written outside its logical elements" % (c, name)
        assert not np.isnan(val).any(), "%s: NaN in %s (%d elements: unwritten, or poisoned by a stray read)" % (
            c, name, int(np.isnan(val).sum()))
        err = np.abs(val - r)
        with np.errstate(divide="ignore", invalid="ignore"):   # bound 0 (act'(aux) = 0): the result is exact
            ratio = np.where(err == 0.0, 0.0, err / bound)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[i] <= 1.0, "%s: %s%s = %r, ref %r, err / bound = %.3g" % (c, name, list(i), val[i], r[i], ratio[i])
        worst = max(worst, float(ratio[i]))
    return worst


# --------------------------------------------------------------------------- cases
def kloop_cases(tiles=range(5)):
    """2 x 2 tiles, one interior workgroup and three edge ones in one launch; whole k-tiles, aligned
    operands: the interior workgroup takes the loop ``expected_loop`` names, the others gemm_kloop<false>."""
    out = []
    for tile in tiles:
        bm, bn = TILE_DIMS[tile]
        for dtype, (am, bmd), nk in itertools.product(("bf16", "f32"), LAYOUTS, (1, 2, 3, 4, 5, 7, 9)):
            out.append(Case(tile, dtype, am, bmd, bm + bm // 2 + 1, bn + 9, KT * nk, ld="pad8"))
    return out


def splitk_cases(tiles=range(5)):
    """The same grid with split-K: 6 k-tiles as 3 + 3 and 2 + 2 + 2, 7 as 4 + 3 and 3 + 3 + 1; ticketed and atomic."""
    out = []
    for tile in tiles:
        bm, bn = TILE_DIMS[tile]
        for dtype, (am, bmd), nk, splits, atomic in itertools.product(("bf16", "f32"), LAYOUTS, (6, 7), (2, 3),
                                                                      (False, True)):
            out.append(Case(tile, dtype, am, bmd, bm + bm // 2 + 1, bn + 9, KT * nk, ld="pad8", splits=splits,
                            atomic=atomic))
    return out


def ktail_cases(tiles=(0, 1, 4)):
    """K tails and unaligned operands: 2 x 2 tiles (the first interior in its rows), every loader branch."""
    out = []
    for tile in tiles:
        bm, bn = TILE_DIMS[tile]
        for dtype, (am, bmd), K in itertools.product(("bf16", "f32"), LAYOUTS, (1, 7, 8, 9, 63, 65, 127, 129, 201)):
            for ld, off in (("tight", 0), ("pad8", 0), ("pad3", 0), ("pad8", 1)):
                out.append(Case(tile, dtype, am, bmd, bm + 5, bn + 3, K, ld=ld, off=off))
    return out


def edge_cases(tiles=range(5)):
    """M and N edges; strides padded to 8, so RMAJ operands load by vector except the last row chunk
    (rows % VEC != 0), which is scalar.  K = one whole k-tile + 8."""
    out = []
    for tile in tiles:
        bm, bn = TILE_DIMS[tile]
        ms, ns = (1, 15, 17, bm - 1, bm + 1), (1, 7, 9, bn - 1, bn + 1)
        pairs = itertools.product(ms, ns) if tile in (0, 4) else zip(ms, ns)
        for (M, N), dtype, (am, bmd) in itertools.product(list(pairs), ("bf16", "f32"), LAYOUTS):
            out.append(Case(tile, dtype, am, bmd, M, N, 72, ld="pad8"))
    return out


_STORES = ((72, 72, 0), (72, 77, 0), (72, 80, 1), (70, 72, 0))  # N, ldc, out_off


def store_cases():
    out = []
    for tile, dtype, (N, ldc, off), odt in itertools.product((0, 4), ("bf16", "f32"), _STORES, ("f32", "bf16")):
        bm = TILE_DIMS[tile][0]
        for am, bmd in ((ops.KMAJ, ops.KMAJ), (ops.KMAJ, ops.RMAJ)):
            out.append(Case(tile, dtype, am, bmd, bm + 5, N, 72, ld="pad8", ldc=ldc, out_off=off, out_dtype=odt))
    return out


def epilogue_cases():
    """Every epilogue feature with the 8-wide vector store open to it (ldc = 72) and closed (ldc = 77)."""
    out = []
    for dtype, ldc in itertools.product(("bf16", "f32"), (72, 77)):
        def mk(K=72, **kw):
            out.append(Case(0, dtype, ops.KMAJ, ops.RMAJ, 69, 72, K, ld="pad8", ldc=ldc, **kw))
        mk(bias_axis=0)
        mk(bias_axis=1)
        mk(act=ops.ACT_RELU, bias_axis=0)
        for act in (0, 1):
            mk(act=act)
        for act in (2, 3):   # K = 4: |z| <= 9, so a k-term still moves act(z) by more than the bound
            mk(K=4, act=act)
        mk(alpha=-0.5)
        mk(alpha=-0.5, bias_axis=0, act=ops.ACT_RELU, out_dtype="bf16")
        mk(beta=0.75)
        mk(beta=0.75, out_dtype="bf16")
        for o2, tr in itertools.product(("f32", "bf16"), (False, True)):
            mk(out2=o2, out2_trans=tr)
        for aux_act in (1, 2, 3):
            mk(aux="f32", aux_act=aux_act)
            mk(aux="bf16", aux_act=aux_act, ld_aux=80)
            mk(aux="bf16", aux_act=aux_act, ld_aux=77)
    return out


def ones_cases():
    """a_ones_row = M - 1 / b_ones_row = N - 1 with bias_out: inside an edge tile, and first of a tile (M - 1 = BM)."""
    out = []
    for dtype, (am, bmd), atomic, ldc in itertools.product(("bf16", "f32"), ((ops.RMAJ, ops.RMAJ), (ops.KMAJ, ops.KMAJ)),
                                                            (False, True), (80, 77)):
        for M, N, ones in ((70, 72, "a"), (65, 72, "a"), (69, 71, "b"), (69, 65, "b")):
            out.append(Case(0, dtype, am, bmd, M, N, 72, ld="pad8", ldc=ldc, ones=ones, atomic=atomic))
    return out


def combined_cases():
    """bias + ReLU + bf16 aux + bf16 out + ticketed split-K (a whole k-tile and a tail of 8, one per split)."""
    return [Case(0, dtype, ops.KMAJ, ops.RMAJ, 69, 72, 72, ld="pad8", ldc=ldc, out_dtype="bf16", bias_axis=0,
                 act=ops.ACT_RELU, aux="bf16", aux_act=ops.ACT_RELU, ld_aux=ldc, splits=2)
            for dtype, ldc in itertools.product(("bf16", "f32"), (72, 77))]


GROUPS = {"kloop": kloop_cases, "splitk": splitk_cases, "ktail": ktail_cases, "edges": edge_cases,
          "stores": store_cases, "epilogues": epilogue_cases, "ones": ones_cases, "combined": combined_cases}
