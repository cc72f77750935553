"""Shared pieces of the eval_metrics tests: the float64 oracle, the loss bound and the inputs.

The loss bound.  Write u = 2^-24 (float32 unit roundoff), m = max z, R = max z - min z, S = sum_j exp(z_j - m)
(1 <= S <= NC).  The kernel and the host mirror both compute, in float32,

    d_j = z_j - m                 |d_j| <= R: one rounding, absolute error <= u R, a relative error u R in exp(d_j)
    e_j = exp(d_j)                E_exp ulp = 2 u E_exp relative
    S   = sum of NC terms >= 0    any order: relative error <= (NC - 1) u
    l   = log(S)                  E_log ulp of |l| <= log NC, plus S's relative error as an absolute one
    lse = m + l                   one rounding of |lse| <= |m| + log NC
    loss = lse - z_t              one rounding of |loss| <= |m| + |z_t| + log NC

which sums to u [(NC - 1) + R + 2 E_exp + 2 E_log log NC + (|m| + log NC) + (|m| + |z_t| + log NC)]
<= 2 u [NC + R + E_exp + E_log log NC + 2 (|m| + |z_t| + log NC)], the per-row bound used here.

E_exp, E_log: no accuracy table for the device's expf / logf ships with the toolchain, so they were measured
on the MI355X against float64 at 2^22 points per range: expf 0.84 ulp on [-1, 0], 0.86 ulp on [-20, 0], 1.00 ulp
on [-104, 0] (below that it returns 0, like float64 rounded: 0.49 ulp of the smallest denormal), logf 2.05 ulp on
[1, 2], 2.31 ulp on [1, 10], 2.29 ulp on [1, 1000].  With a 4x margin: E_EXP = 4, E_LOG = 10.  (The host mirror
rounds float64 exp / log once: 0.5 ulp each, inside the same constants.)

The set's bound adds the fold's rounding: the kernel adds the row losses serially in float64, so a sum of r
rows is off by at most (r - 1) 2^-53 sum |loss| to first order; the oracle's own sum is math.fsum (exact).
"""
import math

import numpy as np

U = 2.0 ** -24
E_EXP, E_LOG = 4.0, 10.0
PAD_LABEL = -7  # what the rows behind the last valid one hold: NaN logits and this label


def oracle_rows(z, t):
    """float64 cross-entropy per row of float32 logits z [R][NC] at labels t (all inside [0, NC))."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    return lse - z[np.arange(z.shape[0]), t]


def row_bounds(z, t):
    z = np.asarray(z, dtype=np.float64)
    NC = z.shape[1]
    m, lo = z.max(1), z.min(1)
    zt = z[np.arange(z.shape[0]), t]
    ln = math.log(NC)
    return 2 * U * (NC + (m - lo) + E_EXP + E_LOG * ln + 2 * (np.abs(m) + np.abs(zt) + ln))


def set_bound(losses64, bounds):
    """Bound of a folded sum over rows with float64 losses ``losses64`` and per-row bounds ``bounds``."""
    r = len(losses64)
    return float(np.sum(bounds)) + max(r - 1, 0) * 2.0 ** -53 * float(np.sum(np.abs(losses64) + bounds))


def argsort_hits(z, t, k):
    """(hit1, hitk) from an independent construction: the position of t in a stable descending sort."""
    order = np.argsort(-np.asarray(z, dtype=np.float64), axis=1, kind="stable")
    pos = np.array([int(np.nonzero(order[r] == t[r])[0][0]) for r in range(z.shape[0])])
    return pos == 0, pos < k


def special_rows(NC, nan_target):
    """Hand-built (logits row, label) pairs for NC >= 3 classes."""
    f = np.float32
    rows = []
    rows.append((np.full(NC, 0.25, f), 1))                      # all equal: the label ranks behind class 0
    rows.append((np.full(NC, 0.25, f), 0))                      # all equal, label first: rank 0
    a = np.linspace(-1, 0, NC).astype(f); a[0] = 2; a[1] = 2    # a duplicate maximum before the target
    rows.append((a, 1))
    b = np.linspace(-1, 0, NC).astype(f); b[0] = 2; b[NC - 1] = 2  # ... and one after it
    rows.append((b, 0))
    c = np.linspace(0, 1, NC).astype(f)
    rows.append((c.copy(), 0))                                  # target first (the smallest logit)
    rows.append((c.copy(), NC - 1))                             # target last (the largest)
    d = np.where(np.arange(NC) % 2 == 0, f(3e4), f(-3e4)).astype(f)
    rows.append((d.copy(), 0))                                  # magnitudes of +-3e4, target at +3e4
    rows.append((d.copy(), 1))                                  # ... and at -3e4
    if nan_target:
        e = np.linspace(-1, 1, NC).astype(f); e[2] = np.nan
        rows.append((e, 2))
    return rows


def make_set(B, NC, seed, nan_target=False, bad_label=True):
    """n = 2B + ceil(B / 3) rows: the special rows spread over the chunks, random rows (with ties) between
    them, one out-of-range label in a valid row.  Returns (z [n][NC] float32, t [n] int32)."""
    n = 2 * B + -(-B // 3)
    rng = np.random.RandomState(seed)
    z = (rng.randn(n, NC) * 3).astype(np.float32)
    z[::3] = np.round(z[::3])  # every third row: integer logits, so exact ties occur
    t = rng.randint(0, NC, size=n).astype(np.int32)
    sp = special_rows(NC, nan_target)
    at = np.linspace(0, n - 1, len(sp)).astype(int)  # first and last row included
    for r, (row, lab) in zip(at, sp):
        z[r], t[r] = row, lab
    if bad_label:
        free = [r for r in range(n) if r not in set(at.tolist())]
        t[free[len(free) // 2]] = NC
    return z, t


def chunk_inputs(z, t, B, c):
    """Launch c's buffers: rows [c B, c B + B) of the set, NaN logits and PAD_LABEL behind its end."""
    n, NC = z.shape
    zc = np.full((B, NC), np.nan, np.float32)
    tc = np.full(B, PAD_LABEL, np.int32)
    lo = c * B
    m = max(0, min(B, n - lo))
    zc[:m], tc[:m] = z[lo:lo + m], t[lo:lo + m]
    return zc, tc
