"""Cases, float64 oracles and error bounds for the persistent LSTM sequence kernels (csrc/kernels/lstm_seq.hip:
single-workgroup and 4- / 8-way split forward and BPTT) and the per-step cell kernels (elementwise.hip).

Shared by tests/test_lstm_seq_paths_gpu.py (the kernels) and tests/test_lstm_seq_oracle_cpu.py (the oracle
itself: agreement with float64 autograd, the fp32 CPU path inside every bound, sensitivity to wrong kernels).

Inputs (recipe of gemm_dense_cases): magnitudes uniform in [0.5, 1.5] with a random sign; K scaled by
1 / sqrt(I + H) so pre-activations are O(1); bias magnitudes in [0.25, 0.75], never zero; forget_bias from
{0, 1, 2.5}; h_{-1} (xh[0][:, I:]) non-zero unless the launch stages the batch.  The backward cases take
synthetic act (sigmoid columns in (0.05, 0.95), tanh columns in (-0.95, 0.95)) and c (magnitude in [0.5, 1.5]),
so they do not depend on the forward kernel.

Guarding: every tensor is a view into a larger buffer with GUARD elements of SENT on either side.  Outputs
that must be written start as NaN; everything else must come back bitwise as it was.

Forward, teacher-forced (derived bounds; each step from the values the kernel itself stored):
    act[t] from the kernel's xh[t] row:  pre-activation bound e = (KT + 8) U (|A| . |K|) + U |bias|, through the
        activation as in gemm_dense_cases: e * act'(max(|z| - e, 0)) + ACT_ALLOW * |act(z)|.  The 8 spare
        roundings cover bias + forget_bias and the accumulator + bias addition wherever |A| . |K| >= 1
        (asserted).
    c[t] from the kernel's act[t] and c[t-1]:  3 U (|c_prev sf| + |si tj|)
    h_t  from the kernel's c[t] and o gate:    (ACT_ALLOW[tanh] + 2 U) |h|
Forward, free-running: float64 recurrence from the inputs; per tensor and step in relative Frobenius norm
    against 16 x the running maximum of the fp32 CPU path's error plus ACT_ALLOW[sigmoid].
Backward: float64 BPTT with a running first-order bound: input errors times |sensitivity|, U |result| per fp32
    operation, ACT_ALLOW[tanh] |tanh c|, (n + p) U sum |terms| per dot product (n = 4H, p = 8 for dh_{t-1};
    n = nc, p = 1 for dl . wo^T).  Every operation also gets the fp32 underflow allowance TINY.
Backward, teacher-forced (bwd_teacher): the running bound grows by a step's absolute gain (about 4 x with these
    inputs), so some twenty steps from the end it passes anything.  Each step is therefore also recomputed from
    the dg[t+1] the kernel itself stored (dh_t = dg[t+1] . K_h^T, dc_t recovered from its d_j column), which
    keeps the bound at a few U at every step.
"""
import dataclasses
import zlib

import numpy as np
import torch

from dtfe import ops
from gemm_dense_cases import ACT_ALLOW, GUARD, SENT, U, _values

H = 128                 # the persistent kernels' hidden size
LR = 16                 # batch rows per row group
MAX_GROUPS = 64         # lstm_seq.hip: exchange buffers are sized for this many row groups
A_SIG, A_TANH = ACT_ALLOW[ops.ACT_SIGMOID], ACT_ALLOW[ops.ACT_TANH]
FREE_FACTOR = 16        # free-running check: err_gpu(t) <= FREE_FACTOR * max_{s<=t} err_cpu32(s) + A_SIG
NAN = float("nan")


def _atoi(s):
    s = s.strip()
    n = 0
    while n < len(s) and (s[n].isdigit() or (n == 0 and s[n] in "+-")):
        n += 1
    try:
        return int(s[:n])
    except ValueError:
        return 0


def expected_split(B, T, I, env, hidden=H):
    """Host mirror of lstm_seq.hip split_ns: workgroups per row group the launchers pick (0: the single
    kernel).  env: the value of DTFE_LSTM_SPLIT, None when unset."""
    v = _atoi(env) if env is not None else 1
    if v == 0 or hidden != 128 or I != 28 or B % LR != 0 or B // LR > MAX_GROUPS or T >= 255:
        return 0
    groups = B // LR
    if v != 4 and groups * 8 <= 256:
        return 8
    return 4 if groups * 4 <= 256 else 0


def declines(kind, B, I, hidden=H):
    """Host mirror of the launchers' shape checks: True where launch_lstm_seq_fwd / _bwd returns false."""
    if kind == "fwd":
        return hidden != 128 or I != 28 or B % LR != 0
    return hidden != 128 or B % LR != 0 or (I + hidden) % 4 != 0


# --------------------------------------------------------------------------- buffers
def _f32(a):
    """float64 array -> (fp32 torch tensor, the values as stored in float64)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
    return t, t.double().numpy()


def guarded(t):
    """flat buffer: GUARD x SENT, the tensor, GUARD x SENT"""
    buf = torch.full((t.numel() + 2 * GUARD,), SENT, dtype=t.dtype)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return buf


def view(buf, shape):
    n = int(np.prod(shape))
    assert buf.numel() == n + 2 * GUARD, (buf.numel(), shape)
    return buf[GUARD:GUARD + n].view(*shape)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


def guards_intact(buf):
    g = torch.full((GUARD,), SENT, dtype=buf.dtype)
    return same_bits(buf[:GUARD], g) and same_bits(buf[-GUARD:], g)


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / bound)


# --------------------------------------------------------------------------- forward
@dataclasses.dataclass(frozen=True)
class FwdCase:
    B: int
    T: int
    split: object = None        # DTFE_LSTM_SPLIT: None (unset) | "0" | "4"
    forget_bias: float = 1.0
    I: int = 28
    hidden: int = H
    staged: bool = False        # xsrc / ysrc / ydst / zero0 / zero1: batch staging folded into the launch
    kscale: float = 1.0         # 8: the saturating case

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())


@dataclasses.dataclass
class Built:
    case: object
    shapes: dict                # name -> logical shape
    bufs: dict                  # name -> guarded flat CPU buffer as the launch finds it
    inp: dict                   # float64 numpy values as stored


NC_LABELS = 10


def build_fwd(c):
    rng = np.random.default_rng(c.seed)
    T, B, I, Hh = c.T, c.B, c.I, c.hidden
    KT = I + Hh
    x, x64 = _f32(_values(rng, (T, B, I)))
    h0, h064 = _f32(np.zeros((B, Hh)) if c.staged else _values(rng, (B, Hh), 0.25, 0.75))
    K, K64 = _f32(_values(rng, (KT, 4 * Hh)) * (c.kscale / np.sqrt(KT)))
    bias, b64 = _f32(_values(rng, (4 * Hh,), 0.25, 0.75))
    xh = torch.full((T, B, KT), NAN)
    if not c.staged:
        xh[:, :, :I] = x
        xh[0, :, I:] = h0
    t = {"xh": xh, "K": K, "bias": bias, "act": torch.full((T, B, 4 * Hh), NAN), "c": torch.full((T, B, Hh), NAN),
         "hT": torch.full((B, Hh), NAN)}
    if c.staged:
        t["xsrc"] = x.transpose(0, 1).reshape(B, T * I).contiguous()   # the images: row t of image b is x_t[b]
        t["ysrc"] = _f32(_values(rng, (B, NC_LABELS)))[0]
        t["ydst"] = torch.full((B, NC_LABELS), NAN)
        t["zero0"] = torch.full((1,), 3.5)
        t["zero1"] = torch.full((1,), 77, dtype=torch.int32)
    inp = {"x": x64, "h0": h064, "K": K64, "bias": b64, "fb": float(c.forget_bias), "I": I, "H": Hh}
    return Built(c, {k: tuple(v.shape) for k, v in t.items()}, {k: guarded(v) for k, v in t.items()}, inp)


def _matmul32(a, b, reverse_k):
    if reverse_k:   # the same products, the k-sum taken in reversed order
        return a.flip(1).contiguous() @ b.flip(0).contiguous()
    return a @ b


def run_fwd(b, dev, reverse_k=False):
    """Launch the case: "cuda" the persistent kernel (torch.ops.dtfe.lstm_seq_fwd), "cpu" the project's fp32
    per-step path (ops.lstm_cell_fwd with a float32 matmul).  Returns (what the launcher returned, the whole
    buffers afterwards on the CPU)."""
    c = b.case
    bufs = {k: v.clone().to(dev) for k, v in b.bufs.items()}
    v = {k: view(bufs[k], b.shapes[k]) for k in bufs}
    if dev != "cpu":
        st = [v.get(k) for k in ("xsrc", "ysrc", "ydst", "zero0", "zero1")]
        ok = bool(ops.require().lstm_seq_fwd(v["xh"], v["K"], v["bias"], c.forget_bias, v["act"], v["c"], v["hT"], *st))
        torch.cuda.synchronize()
    else:
        ok = True
        T, I = c.T, c.I
        if c.staged:
            v["xh"][:, :, :I] = v["xsrc"].view(c.B, T, I).transpose(0, 1)
            v["xh"][0, :, I:] = 0
            v["ydst"].copy_(v["ysrc"])
            v["zero0"].zero_()
            v["zero1"].zero_()
        for t in range(T):
            gates = _matmul32(v["xh"][t], v["K"], reverse_k) + v["bias"]
            h_out = v["xh"][t + 1, :, I:] if t + 1 < T else v["hT"]
            ops.lstm_cell_fwd(gates, v["act"][t], v["c"][t - 1] if t > 0 else None, v["c"][t], h_out,
                              I + c.hidden if t + 1 < T else c.hidden, c.forget_bias)
    return ok, {k: t.cpu() for k, t in bufs.items()}


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _activate(z, Hh, tanh_block=1):
    a = _sig(z)
    s = slice(tanh_block * Hh, (tanh_block + 1) * Hh)
    a[..., s] = np.tanh(z[..., s])
    return a


def _with_fb(z, Hh, fb, gate=2):
    z = z.copy()
    z[..., gate * Hh:(gate + 1) * Hh] += fb
    return z


def fwd_free(inp, mutate=None):
    """The float64 recurrence from the inputs alone: {"xh" [T][B][KT], "act", "c", "hT"}.
    mutate: a wrong kernel (None: the reference).  One-step mutations act on the last step, t0 = T - 1:
      fb_drop    forget_bias not applied            fb_on_o    forget_bias applied to gate o
      bias_shift bias read one column off           swap_jf    gates j and f treated as each other
      drop_hk    one h k-term missing at t0         row_shift  row r consumes row r + 1's h at t0
      no_h0      h_{-1} taken as zero
    In every mutant the stored xh holds the right h: the mutant consumes a wrong one, as a stale or
    misrouted exchange word would."""
    x, K, bias, fb, I, Hh = inp["x"], inp["K"], inp["bias"], inp["fb"], inp["I"], inp["H"]
    T, B = x.shape[:2]
    t0, u0 = T - 1, 5
    if mutate == "bias_shift":
        bias = np.roll(bias, 1)
    xh = np.zeros((T, B, I + Hh))
    act = np.zeros((T, B, 4 * Hh))
    cs = np.zeros((T, B, Hh))
    h, c = inp["h0"].copy(), np.zeros((B, Hh))
    for t in range(T):
        xh[t, :, :I], xh[t, :, I:] = x[t], h
        hin = h
        if mutate == "no_h0" and t == 0:
            hin = np.zeros_like(h)
        if mutate == "row_shift" and t == t0:
            hin = np.roll(h, -1, axis=0)
        z = np.concatenate([x[t], hin], 1) @ K
        if mutate == "drop_hk" and t == t0:
            z = z - np.outer(hin[:, u0], K[I + u0])
        z = z + bias
        if mutate == "swap_jf":
            a = _activate(_with_fb(z, Hh, fb, 1), Hh, tanh_block=2)
        elif mutate == "fb_drop":
            a = _activate(z, Hh)
        else:
            a = _activate(_with_fb(z, Hh, fb, 3 if mutate == "fb_on_o" else 2), Hh)
        c = c * a[:, 2 * Hh:3 * Hh] + a[:, :Hh] * a[:, Hh:2 * Hh]
        h = np.tanh(c) * a[:, 3 * Hh:]
        act[t], cs[t] = a, c
    return {"xh": xh, "act": act, "c": cs, "hT": h}


FWD_MUTATIONS = ("fb_drop", "fb_on_o", "bias_shift", "swap_jf", "drop_hk", "row_shift", "no_h0")


def fwd_mutation_applies(c, how):
    if how in ("fb_drop", "fb_on_o"):
        return c.forget_bias != 0.0
    if how == "no_h0":
        return not c.staged
    if how in ("drop_hk", "row_shift"):   # the h consumed at the last step must be non-zero
        return c.T >= 2 or not c.staged
    return True


def as_stored(vals):
    """round a {name: float64 array} to fp32 and back: what a kernel computing exactly these values stores"""
    return {k: v.astype(np.float32).astype(np.float64) for k, v in vals.items()}


def fwd_teacher(inp, xh, act, c, hT):
    """Teacher-forced forward check: {"act", "c", "h"} -> err / bound per element ([T][B][*]), each step
    recomputed in float64 from the values the kernel stored for it."""
    K, bias, fb, I, Hh = inp["K"], inp["bias"], inp["fb"], inp["I"], inp["H"]
    T, B, KT = xh.shape
    A = xh.reshape(T * B, KT)
    z = _with_fb(A @ K + bias, Hh, fb)
    S = np.abs(A) @ np.abs(K)
    assert S.min() >= 1.0, "the 8 spare roundings of the pre-activation bound need |A| . |K| >= 1"
    e = (KT + 8) * U * S + U * np.abs(bias)
    a_ref = _activate(z, Hh)
    zz = np.maximum(np.abs(z) - e, 0.0)
    s = _sig(zz)
    sup = s * (1.0 - s)
    tj = np.tanh(zz[:, Hh:2 * Hh])
    sup[:, Hh:2 * Hh] = 1.0 - tj * tj
    allow = np.full(4 * Hh, A_SIG)
    allow[Hh:2 * Hh] = A_TANH
    r_act = _ratio(np.abs(act.reshape(T * B, 4 * Hh) - a_ref), e * sup + allow * np.abs(a_ref)).reshape(T, B, 4 * Hh)
    si, tjk, sf, so = (act[:, :, k * Hh:(k + 1) * Hh] for k in range(4))
    c_prev = np.concatenate([np.zeros((1, B, Hh)), c[:-1]], 0)
    keep, new = c_prev * sf, si * tjk
    r_c = _ratio(np.abs(c - (keep + new)), 3 * U * (np.abs(keep) + np.abs(new)))
    h_ref = np.tanh(c) * so
    h_got = np.concatenate([xh[1:, :, I:], hT[None]], 0)
    r_h = _ratio(np.abs(h_got - h_ref), (A_TANH + 2 * U) * np.abs(h_ref))
    return {"act": r_act, "c": r_c, "h": r_h}


def fwd_free_errs(ref, got):
    """relative Frobenius error per tensor and timestep: {"act", "c", "h"} -> [T]"""
    I = ref["xh"].shape[2] - ref["hT"].shape[1]
    hs = lambda d: np.concatenate([d["xh"][1:, :, I:], d["hT"][None]], 0)  # noqa: E731
    out = {}
    for name, (r, g) in {"act": (ref["act"], got["act"]), "c": (ref["c"], got["c"]), "h": (hs(ref), hs(got))}.items():
        T = r.shape[0]
        num = np.sqrt(((g - r) ** 2).reshape(T, -1).sum(1))
        out[name] = num / np.sqrt((r ** 2).reshape(T, -1).sum(1))
    return out


def logical(b, got):
    """{name: float64 numpy logical tensor} of the buffers ``run_*`` returned"""
    return {k: view(v, b.shapes[k]).double().numpy() for k, v in got.items()}


def check_untouched(b, got, names):
    for k in names:
        assert same_bits(got[k], b.bufs[k]), "%s: %s changed" % (b.case, k)


def check_fwd(b, got, cpu32=None):
    """Assert guards, untouched inputs, staging, finiteness and the teacher-forced bounds of a forward launch;
    with cpu32 (the fp32 CPU path's buffers of the same case) the free-running check too.  Returns
    {"act" | "c" | "h": largest err / bound, "free": largest err_gpu / err_cpu32 or None}."""
    c = b.case
    I = c.I
    for k, buf in got.items():
        assert guards_intact(buf), "%s: guard of %s overwritten" % (c, k)
    check_untouched(b, got, [k for k in ("K", "bias", "xsrc", "ysrc") if k in got])
    v = {k: view(t, b.shapes[k]) for k, t in got.items()}
    if c.staged:
        x_want = view(b.bufs["xsrc"], b.shapes["xsrc"]).view(c.B, c.T, I).transpose(0, 1)
        assert same_bits(v["xh"][:, :, :I], x_want), "%s: staged x columns differ from the images" % (c,)
        assert same_bits(v["xh"][0, :, I:], torch.zeros(c.B, c.hidden)), "%s: h_{-1} not zeroed" % (c,)
        assert same_bits(v["ydst"], v["ysrc"]), "%s: labels not copied" % (c,)
        assert float(v["zero0"][0]) == 0.0 and int(v["zero1"][0]) == 0, "%s: accumulators not cleared" % (c,)
    else:
        w = view(b.bufs["xh"], b.shapes["xh"])
        assert same_bits(v["xh"][:, :, :I], w[:, :, :I]), "%s: x columns of xh changed" % (c,)
        assert same_bits(v["xh"][0, :, I:], w[0, :, I:]), "%s: h_{-1} changed" % (c,)
    d = {k: v[k].double().numpy() for k in ("xh", "act", "c", "hT")}
    for k in d:
        assert np.isfinite(d[k]).all(), "%s: %d non-finite elements in %s (unwritten, or poisoned)" % (
            c, int((~np.isfinite(d[k])).sum()), k)
    worst = {}
    for name, r in fwd_teacher(b.inp, d["xh"], d["act"], d["c"], d["hT"]).items():
        i = np.unravel_index(np.argmax(r), r.shape)
        assert r[i] <= 1.0, "%s: teacher-forced %s[t, row, col = %s]: err / bound = %.3g" % (c, name, list(i), r[i])
        worst[name] = float(r[i])
    worst["free"] = None
    if cpu32 is not None:
        ref = fwd_free(b.inp)
        eg = fwd_free_errs(ref, d)
        ec = fwd_free_errs(ref, {k: view(cpu32[k], b.shapes[k]).double().numpy() for k in ("xh", "act", "c", "hT")})
        worst["free"] = 0.0
        for name in eg:
            run_max = np.maximum.accumulate(ec[name])
            lim = FREE_FACTOR * run_max + A_SIG
            t = int(np.argmax(eg[name] / lim))
            assert eg[name][t] <= lim[t], "%s: free-running %s[t = %d]: err %.3g, fp32 CPU path %.3g (running max)" % (
                c, name, t, eg[name][t], run_max[t])
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(eg[name] == 0.0, 0.0, eg[name] / run_max)
            worst["free"] = max(worst["free"], float(q.max()))
    return worst


FBS = (0.0, 1.0, 2.5)


def fwd_grid_cases():
    """B in {16, 48, 128} x T in {1, 2, 3, 28} x split in {"0", "4", unset}; forget_bias cycles so that
    every value meets every split mode (and every B, and every T but one)."""
    out = []
    for si, split in enumerate(("0", "4", None)):
        for bi, B in enumerate((16, 48, 128)):
            for ti, T in enumerate((1, 2, 3, 28)):
                out.append(FwdCase(B, T, split, FBS[(si + bi + ti) % 3]))
    return out


def fwd_edge_cases():
    """the dispatch edges of split_ns: (case, expected lstm_last_split)"""
    return [(FwdCase(528, 3, None, 2.5), 4),      # groups * 8 = 264 > 256: the default drops to NS = 4
            (FwdCase(528, 3, "4", 0.0), 4),
            (FwdCase(1024, 2, None, 1.0), 4),     # groups == MAX_GROUPS
            (FwdCase(1040, 2, None, 2.5), 0),     # groups > MAX_GROUPS: the single kernel
            (FwdCase(16, 254, None, 0.0), 8),     # the largest split T: tags up to base + 254
            (FwdCase(16, 255, None, 1.0), 0)]     # past the T limit


def fwd_staged_cases():
    return [FwdCase(B, 28, split, fb, staged=True) for (B, split, fb) in
            ((48, "0", 0.0), (48, None, 1.0), (128, "0", 2.5), (128, None, 0.0))]


def fwd_saturating_cases():
    return [FwdCase(48, 3, None, 1.0, kscale=8.0), FwdCase(48, 3, "0", 1.0, kscale=8.0)]


def all_fwd_cases():
    return fwd_grid_cases() + [c for c, _ in fwd_edge_cases()] + fwd_staged_cases() + fwd_saturating_cases()


# --------------------------------------------------------------------------- backward
@dataclasses.dataclass(frozen=True)
class BwdCase:
    B: int
    T: int
    split: object = None
    nc: int = 0                 # 0: dh_T given (dhT); else dl [B][nc] . wo [H][nc]^T formed by the kernel
    I: int = 28
    hidden: int = H

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())


def _synthetic_act(rng, shape_rows, Hh):
    a = rng.uniform(0.05, 0.95, size=shape_rows + (4 * Hh,))
    a[..., Hh:2 * Hh] = rng.uniform(-0.95, 0.95, size=shape_rows + (Hh,))
    return a


def build_bwd(c):
    rng = np.random.default_rng(c.seed)
    T, B, I, Hh = c.T, c.B, c.I, c.hidden
    KT = I + Hh
    K, K64 = _f32(_values(rng, (KT, 4 * Hh)) / np.sqrt(KT))
    act, a64 = _f32(_synthetic_act(rng, (T, B), Hh))
    cc, c64 = _f32(_values(rng, (T, B, Hh)))
    t = {"K": K, "act": act, "c": cc, "dg": torch.full((T, B, 4 * Hh), NAN)}
    inp = {"K": K64, "act": a64, "c": c64, "I": I, "H": Hh, "dhT": None, "dl": None, "wo": None}
    if c.nc:
        t["dhT"] = torch.full((B, Hh), NAN)   # not read when dl / wo are given
        t["dl"], inp["dl"] = _f32(_values(rng, (B, c.nc)))
        t["wo"], inp["wo"] = _f32(_values(rng, (Hh, c.nc)))
    else:
        t["dhT"], inp["dhT"] = _f32(_values(rng, (B, Hh)))
    return Built(c, {k: tuple(v.shape) for k, v in t.items()}, {k: guarded(v) for k, v in t.items()}, inp)


def run_bwd(b, dev, reverse_k=False):
    c = b.case
    bufs = {k: v.clone().to(dev) for k, v in b.bufs.items()}
    v = {k: view(bufs[k], b.shapes[k]) for k in bufs}
    if dev != "cpu":
        ok = bool(ops.require().lstm_seq_bwd(v["K"], v["act"], v["c"], v["dhT"], v["dg"], c.I, v.get("dl"), v.get("wo")))
        torch.cuda.synchronize()
    else:
        ok = True
        dh = (v["dl"] @ v["wo"].t()).contiguous() if c.nc else v["dhT"].clone()
        dc = torch.zeros(c.B, c.hidden)
        Kh = v["K"][c.I:]
        for t in range(c.T - 1, -1, -1):
            ops.lstm_cell_bwd(v["act"][t], v["c"][t - 1] if t > 0 else None, v["c"][t], dh, None, dc, v["dg"][t], dc)
            if t > 0:
                dh = _matmul32(v["dg"][t], Kh.t().contiguous(), reverse_k)
    return ok, {k: t.cpu() for k, t in bufs.items()}


# (value, first-order error bound) pairs: every fp32 operation adds U * |result| - and TINY, the smallest normal
# fp32: below it a result is rounded to a denormal or flushed to zero (the T = 254 BPTT decays through that range)
TINY = 2.0 ** -126


def _ex(v):
    v = np.asarray(v, dtype=np.float64)
    return v, np.zeros_like(v)


def _mul(a, b):
    v = a[0] * b[0]
    return v, a[1] * np.abs(b[0]) + np.abs(a[0]) * b[1] + U * np.abs(v) + TINY


def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v) + TINY


def _neg(a):
    return -a[0], a[1]


def cell_bwd(act_t, c_t, cp, DH, DC, Hh):
    """One cell-backward step on (value, bound) pairs: returns ([d_i, d_j, d_f, d_o], dc carried to t - 1)."""
    si, tj, sf, so = (_ex(act_t[:, k * Hh:(k + 1) * Hh]) for k in range(4))
    one = _ex(np.ones_like(c_t))
    tc = np.tanh(c_t)
    TC = (tc, A_TANH * np.abs(tc))
    DCT = _add(DC, _mul(_mul(DH, so), _add(one, _neg(_mul(TC, TC)))))
    d0 = _mul(_mul(_mul(DCT, tj), si), _add(one, _neg(si)))
    d1 = _mul(_mul(DCT, si), _add(one, _neg(_mul(tj, tj))))
    d2 = _mul(_mul(_mul(DCT, _ex(cp)), sf), _add(one, _neg(sf)))
    d3 = _mul(_mul(_mul(DH, TC), so), _add(one, _neg(so)))
    return [d0, d1, d2, d3], _mul(DCT, sf)


def bwd_oracle(inp, mutate=None):
    """float64 BPTT: (dg [T][B][4H], running first-order error bound of the same shape).
    mutate: drop_dc (the dc carry into step T - 2 dropped) | cp0 (c_prev of step 0 taken from step 1: c[0]) |
    drop_col (one dgate column missing from dh_{T-2}) | wo_T (wo read transposed); the bound of a mutant is
    meaningless - compare it against the reference's."""
    K, act, c, I, Hh = inp["K"], inp["act"], inp["c"], inp["I"], inp["H"]
    T, B = c.shape[:2]
    Kh = K[I:]                      # [H][4H]
    aKh = np.abs(Kh)
    if inp["dl"] is not None:
        dl, wo = inp["dl"], inp["wo"]
        nc = wo.shape[1]
        if mutate == "wo_T":
            wo = wo.reshape(nc, Hh).T   # element [u][c] read at c * H + u
        DH = (dl @ wo.T, (nc + 1) * U * (np.abs(dl) @ np.abs(wo).T))
    else:
        DH = _ex(inp["dhT"])
    DC = _ex(np.zeros((B, Hh)))
    dg, bound = np.zeros((T, B, 4 * Hh)), np.zeros((T, B, 4 * Hh))
    for t in range(T - 1, -1, -1):
        cp = c[t - 1] if t > 0 else np.zeros((B, Hh))
        if mutate == "cp0" and t == 0:
            cp = c[0]
        if mutate == "drop_dc" and t == T - 2:
            DC = _ex(np.zeros((B, Hh)))
        d4, DC = cell_bwd(act[t], c[t], cp, DH, DC, Hh)
        dg[t] = np.concatenate([d[0] for d in d4], 1)
        bound[t] = np.concatenate([d[1] for d in d4], 1)
        if t > 0:
            g = dg[t]
            if mutate == "drop_col" and t == T - 1:
                g = g.copy()
                g[:, 2 * Hh + 7] = 0.0
            DH = (g @ Kh.T, bound[t] @ aKh.T + (4 * Hh + 8) * (U * (np.abs(dg[t]) @ aKh.T) + TINY))
    return dg, bound


def bwd_teacher(inp, dg):
    """Teacher-forced backward check: err / bound per dg element, step t recomputed in float64 from the dg[t+1]
    the kernel itself stored.  The running bound of bwd_oracle grows by the absolute gain of a step (about 4 x
    here), so after some twenty steps it says nothing; this one stays at a few U at every step:
      dh_t  = dg[t+1] . K_h^T                       bound (4H + 8) U (|dg[t+1]| . |K_h|^T)
      dc_t  = d_j[t+1] / (si (1 - tj^2)) * sf       the stored d_j is the kernel's dc * si * (1 - tj^2) after 3
              roundings and tj^2's, which 1 - tj^2 magnifies by tj^2 / (1 - tj^2); one more for * sf, one spare:
              (5 + tj^2 / (1 - tj^2)) U |dc_t|      (the synthetic act keeps si >= 0.05 and |tj| <= 0.95)
    (each with the underflow allowance TINY per operation, which the division magnifies like the value)
    and then one cell_bwd step with its per-operation bounds."""
    K, act, c, I, Hh = inp["K"], inp["act"], inp["c"], inp["I"], inp["H"]
    T, B = c.shape[:2]
    Kh = K[I:]
    aKh = np.abs(Kh)
    out = np.zeros_like(dg)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            if inp["dl"] is not None:
                dl, wo = inp["dl"], inp["wo"]
                DH = (dl @ wo.T, (wo.shape[1] + 1) * U * (np.abs(dl) @ np.abs(wo).T))
            else:
                DH = _ex(inp["dhT"])
            DC = _ex(np.zeros((B, Hh)))
        else:
            g = dg[t + 1]
            DH = (g @ Kh.T, (4 * Hh + 8) * (U * (np.abs(g) @ aKh.T) + TINY))
            si, tj, sf = (act[t + 1][:, k * Hh:(k + 1) * Hh] for k in range(3))
            gj = 1.0 - tj * tj
            v = g[:, Hh:2 * Hh] / (si * gj) * sf
            DC = (v, (5.0 + tj * tj / gj) * (U * np.abs(v) + TINY * sf / (si * gj)))
        cp = c[t - 1] if t > 0 else np.zeros((B, Hh))
        d4, _ = cell_bwd(act[t], c[t], cp, DH, DC, Hh)
        ref = np.concatenate([d[0] for d in d4], 1)
        out[t] = _ratio(np.abs(dg[t] - ref), np.concatenate([d[1] for d in d4], 1))
    return out


BWD_MUTATIONS = ("drop_dc", "cp0", "drop_col", "wo_T")


def bwd_mutation_applies(c, how):
    if how in ("drop_dc", "drop_col"):
        return c.T >= 2
    if how == "wo_T":
        return c.nc > 1
    if how == "cp0":   # acts on dg[0], which at T = 254 has decayed below the smallest fp32 denormal: both are 0
        return c.T <= 28
    return True


def check_bwd(b, got, ref=None):
    """Assert guards, untouched inputs and every dg element within the running bound; returns the largest err / bound."""
    c = b.case
    for k, buf in got.items():
        assert guards_intact(buf), "%s: guard of %s overwritten" % (c, k)
    check_untouched(b, got, [k for k in got if k != "dg"])
    dg = view(got["dg"], b.shapes["dg"]).double().numpy()
    assert np.isfinite(dg).all(), "%s: %d non-finite elements in dg" % (c, int((~np.isfinite(dg)).sum()))
    r, bound = ref if ref is not None else bwd_oracle(b.inp)
    q = _ratio(np.abs(dg - r), bound)
    i = np.unravel_index(np.argmax(q), q.shape)
    assert q[i] <= 1.0, "%s: dg[t, row, col = %s] = %r, ref %r, err / bound = %.3g" % (c, list(i), dg[i], r[i], q[i])
    qt = bwd_teacher(b.inp, dg)
    j = np.unravel_index(np.argmax(qt), qt.shape)
    assert qt[j] <= 1.0, "%s: teacher-forced dg[t, row, col = %s] = %r: err / bound = %.3g" % (c, list(j), dg[j], qt[j])
    return max(float(q[i]), float(qt[j]))


def bwd_worst(inp, dg, ref):
    """largest err / bound of a dg over both backward checks (the mutation tests' measure)"""
    return max(float(_ratio(np.abs(dg - ref[0]), ref[1]).max()), float(bwd_teacher(inp, dg).max()))


BWD_HEADS = (0, 1, 10, 16)      # dhT, and dl / wo at nc = 1, 10, 16
# the forward grid trimmed to 12 (B, T, split): every B, T, split mode, both split_coords branches, T = 1 (no
# exchange), both exchange parities, the NS switch, the last split size, the fallback past it, the largest split T
BWD_COMBOS = ((16, 1, None), (16, 2, "4"), (16, 28, "0"), (48, 1, "4"), (48, 3, None), (48, 28, None),
              (128, 2, None), (128, 3, "0"), (128, 28, "4"), (528, 3, None), (1024, 2, None), (16, 254, None))


def bwd_cases():
    out = [BwdCase(B, T, split, nc) for (B, T, split) in BWD_COMBOS for nc in BWD_HEADS]
    out += [BwdCase(1040, 2, None, 10)]                      # past MAX_GROUPS: the single kernel
    out += [BwdCase(32, 3, "0", nc, I=12) for nc in BWD_HEADS]   # I = 12: the single kernel takes any (I + H) % 4 == 0
    out += [BwdCase(32, 3, None, 0, I=12)]                   # ... and split_ns keeps I != 28 off the split kernels
    return out


# --------------------------------------------------------------------------- per-step cell kernels
@dataclasses.dataclass(frozen=True)
class CellCase:
    B: int
    hidden: int
    a: bool                     # forward: c_prev given;  backward: dh2 given
    b: bool                     # forward: h_out strided (ld_h = I + H);  backward: dc_next given
    forget_bias: float = 1.0
    I: int = 28

    @property
    def seed(self):
        return zlib.crc32(repr(self).encode())


def cell_cases():
    out = []
    k = 0
    for B in (1, 37, 256):
        for Hh in (128, 96):
            for a in (False, True):
                for bb in (False, True):
                    out.append(CellCase(B, Hh, a, bb, FBS[k % 3]))
                    k += 1
    return out


def build_cell_fwd(c):
    rng = np.random.default_rng(c.seed)
    B, Hh = c.B, c.hidden
    ld = c.I + Hh if c.b else Hh
    gates, g64 = _f32(_values(rng, (B, 4 * Hh)))
    h = torch.full((B, ld), SENT)
    h[:, ld - Hh:] = NAN
    t = {"gates": gates, "act": torch.full((B, 4 * Hh), NAN), "c": torch.full((B, Hh), NAN), "h": h}
    inp = {"gates": g64, "fb": float(c.forget_bias), "H": Hh, "c_prev": None}
    if c.a:
        t["c_prev"], inp["c_prev"] = _f32(_values(rng, (B, Hh)))
    return Built(c, {k: tuple(v.shape) for k, v in t.items()}, {k: guarded(v) for k, v in t.items()}, inp)


def run_cell_fwd(b, dev):
    c = b.case
    bufs = {k: v.clone().to(dev) for k, v in b.bufs.items()}
    v = {k: view(bufs[k], b.shapes[k]) for k in bufs}
    ld = b.shapes["h"][1]
    ops.lstm_cell_fwd(v["gates"], v["act"], v.get("c_prev"), v["c"], v["h"][:, ld - c.hidden:], ld, c.forget_bias)
    if dev != "cpu":
        torch.cuda.synchronize()
    return {k: t.cpu() for k, t in bufs.items()}


def check_cell_fwd(b, got):
    """the per-step forward bounds: act from the given gates (one rounding of z_f + forget_bias), c and h
    from the kernel's own act / c; returns the largest err / bound"""
    c, Hh = b.case, b.case.hidden
    for k, buf in got.items():
        assert guards_intact(buf), "%s: guard of %s overwritten" % (c, k)
    check_untouched(b, got, [k for k in ("gates", "c_prev") if k in got])
    d = logical(b, got)
    ld = b.shapes["h"][1]
    assert (d["h"][:, :ld - Hh] == SENT).all(), "%s: h_out written left of its columns" % (c,)
    h = d["h"][:, ld - Hh:]
    for k, a in (("act", d["act"]), ("c", d["c"]), ("h", h)):
        assert np.isfinite(a).all(), "%s: non-finite %s" % (c, k)
    z = _with_fb(b.inp["gates"], Hh, b.inp["fb"])
    e = np.zeros_like(z)
    e[:, 2 * Hh:3 * Hh] = U * np.abs(z[:, 2 * Hh:3 * Hh])
    a_ref = _activate(z, Hh)
    zz = np.maximum(np.abs(z) - e, 0.0)
    s = _sig(zz)
    sup = s * (1.0 - s)
    allow = np.full(4 * Hh, A_SIG)
    allow[Hh:2 * Hh] = A_TANH
    r_act = _ratio(np.abs(d["act"] - a_ref), e * sup + allow * np.abs(a_ref))
    si, tj, sf, so = (d["act"][:, k * Hh:(k + 1) * Hh] for k in range(4))
    cp = b.inp["c_prev"] if b.inp["c_prev"] is not None else np.zeros_like(d["c"])
    keep, new = cp * sf, si * tj
    r_c = _ratio(np.abs(d["c"] - (keep + new)), 3 * U * (np.abs(keep) + np.abs(new)))
    h_ref = np.tanh(d["c"]) * so
    r_h = _ratio(np.abs(h - h_ref), (A_TANH + 2 * U) * np.abs(h_ref))
    worst = 0.0
    for name, r in (("act", r_act), ("c", r_c), ("h", r_h)):
        i = np.unravel_index(np.argmax(r), r.shape)
        assert r[i] <= 1.0, "%s: %s%s: err / bound = %.3g" % (c, name, list(i), r[i])
        worst = max(worst, float(r[i]))
    return worst


def build_cell_bwd(c):
    rng = np.random.default_rng(c.seed + 1)
    B, Hh = c.B, c.hidden
    act, a64 = _f32(_synthetic_act(rng, (B,), Hh))
    t, inp = {"act": act}, {"act": a64, "H": Hh, "dh2": None, "dc_next": None}
    for k in ("c", "c_prev", "dh") + (("dh2",) if c.a else ()) + (("dc_next",) if c.b else ()):
        t[k], inp[k] = _f32(_values(rng, (B, Hh)))
    t["dgates"] = torch.full((B, 4 * Hh), NAN)
    t["dc_prev"] = torch.full((B, Hh), NAN)
    return Built(c, {k: tuple(v.shape) for k, v in t.items()}, {k: guarded(v) for k, v in t.items()}, inp)


def run_cell_bwd(b, dev):
    bufs = {k: v.clone().to(dev) for k, v in b.bufs.items()}
    v = {k: view(bufs[k], b.shapes[k]) for k in bufs}
    ops.lstm_cell_bwd(v["act"], v["c_prev"], v["c"], v["dh"], v.get("dh2"), v.get("dc_next"), v["dgates"], v["dc_prev"])
    if dev != "cpu":
        torch.cuda.synchronize()
    return {k: t.cpu() for k, t in bufs.items()}


def check_cell_bwd(b, got):
    c, Hh, inp = b.case, b.case.hidden, b.inp
    for k, buf in got.items():
        assert guards_intact(buf), "%s: guard of %s overwritten" % (c, k)
    check_untouched(b, got, [k for k in got if k not in ("dgates", "dc_prev")])
    d = logical(b, got)
    DH = _ex(inp["dh"])
    if inp["dh2"] is not None:
        DH = _add(DH, _ex(inp["dh2"]))
    DC = _ex(inp["dc_next"] if inp["dc_next"] is not None else np.zeros_like(inp["c"]))
    d4, carry = cell_bwd(inp["act"], inp["c"], inp["c_prev"], DH, DC, Hh)
    ref = np.concatenate([x[0] for x in d4], 1), np.concatenate([x[1] for x in d4], 1)
    worst = 0.0
    for name, val, (r, bound) in (("dgates", d["dgates"], ref), ("dc_prev", d["dc_prev"], carry)):
        assert np.isfinite(val).all(), "%s: non-finite %s" % (c, name)
        q = _ratio(np.abs(val - r), bound)
        i = np.unravel_index(np.argmax(q), q.shape)
        assert q[i] <= 1.0, "%s: %s%s: err / bound = %.3g" % (c, name, list(i), q[i])
        worst = max(worst, float(q[i]))
    return worst
