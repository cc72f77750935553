"""ops.eval_metrics on the host mirror: hits against a sort, the loss against float64 under the derived
bound (eval_metrics_cases), the bound's sensitivity, and the mask / cursor arithmetic."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_metrics_cases import (PAD_LABEL, argsort_hits, chunk_inputs, make_set, oracle_rows, row_bounds,  # noqa: E402
                                set_bound)

from dtfe import ops  # noqa: E402

NCS = (3, 10, 70, 1000)


@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("k", (1, 3))
def test_hits_equal_the_position_in_a_stable_sort(NC, k):
    rng = np.random.RandomState(NC + k)
    z = rng.randn(64, NC).astype(np.float32)
    z[::2] = np.round(z[::2] * 2)  # half of the rows hold exact ties
    t = rng.randint(0, NC, size=64).astype(np.int32)
    _loss, hit1, hitk, bad = ops.eval_rows_ref(z, t, k)
    e1, ek = argsort_hits(z, t, k)
    assert not bad.any()
    assert np.array_equal(hit1, e1) and np.array_equal(hitk, ek)
    assert 0 < e1.sum() < 64 or NC > 10  # both outcomes occur at the small class counts


@pytest.mark.parametrize("NC", NCS)
def test_loss_within_the_bound_and_the_bound_is_sensitive(NC):
    """z uniform in [-0.5, 0.5]: the mirror stays inside the per-row bound, and a float64 loss with one class
    term dropped or doubled - the smallest one, the hardest to notice - lies outside it in every row."""
    rng = np.random.RandomState(100 + NC)
    z = (rng.rand(32, NC) - 0.5).astype(np.float32)
    t = rng.randint(0, NC, size=32).astype(np.int32)
    ref, bound = oracle_rows(z, t), row_bounds(z, t)
    loss = ops.eval_rows_ref(z, t, 1)[0]
    assert (np.abs(loss.astype(np.float64) - ref) <= bound).all()
    z64 = z.astype(np.float64)
    m = z64.max(1)
    e = np.exp(z64 - m[:, None])
    zt = z64[np.arange(32), t]
    for factor in (0.0, 2.0):  # the smallest term dropped / doubled
        s = e.sum(1) + (factor - 1.0) * e.min(1)
        wrong = m + np.log(s) - zt
        assert (np.abs(wrong - ref) > bound).all(), (NC, factor)


def _run_mirror(z, t, B, k, launches, with_idx=True):
    n = z.shape[0]
    st = ops.eval_state("cpu", n)
    idx = torch.full((B,), -1, dtype=torch.int32) if with_idx else None
    states = []
    for c in range(launches):
        zc, tc = chunk_inputs(z, t, B, c)
        ops.eval_metrics(torch.from_numpy(zc), torch.from_numpy(tc), k, st, idx=idx)
        states.append((ops.eval_state_dict(st), None if idx is None else idx.clone()))
    return states


@pytest.mark.parametrize("B,NC,k", [(6, 10, 1), (6, 10, 5), (7, 3, 3), (5, 70, 5), (4, 1000, 5)])
def test_mirror_chunks_against_the_oracle(B, NC, k):
    z, t = make_set(B, NC, seed=B * NC + k)
    n = z.shape[0]
    chunks = -(-n // B)
    good = (t >= 0) & (t < NC)
    e1, ek = argsort_hits(z[good], t[good], k)
    ref, bnd = oracle_rows(z[good], t[good]), row_bounds(z[good], t[good])
    states = _run_mirror(z, t, B, k, chunks + 2)
    for c, (st, idx) in enumerate(states):
        rows = min(n, (c + 1) * B)
        g = int(good[:rows].sum())
        assert st["cursor"] == min(c + 1, chunks) and st["n"] == n and st["count"] == rows
        assert st["bad_labels"] == rows - g
        assert st["hits1"] == int(e1[:g].sum()) and st["hitsk"] == int(ek[:g].sum())
        assert abs(st["loss_sum"] - math.fsum(ref[:g])) <= set_bound(ref[:g], bnd[:g])
        want = np.minimum(min(c + 1, chunks) * B + np.arange(B), n - 1)
        assert np.array_equal(idx.numpy(), want)
    assert states[-1][0]["bad_labels"] == 1


def test_nan_target_is_a_miss_and_poisons_only_the_loss():
    z, t = make_set(6, 10, seed=5, nan_target=True, bad_label=False)
    n = z.shape[0]
    st = _run_mirror(z, t, 6, 5, 3, with_idx=False)[-1][0]
    nan_row = int(np.nonzero(np.isnan(z[np.arange(n), t]))[0][0])
    keep = np.arange(n) != nan_row
    e1, ek = argsort_hits(z[keep], t[keep], 5)
    assert st["count"] == n and st["hits1"] == int(e1.sum()) and st["hitsk"] == int(ek.sum())
    assert math.isnan(st["loss_sum"])


@pytest.mark.parametrize("last_hit", (True, False))
def test_mask_and_cursor_mistakes_show(last_hit):
    """n = 13, B = 6: chunks of 6, 6 and 1.  Every row is a top-1 hit, except the last one in the second
    fixture; the five rows behind it in the last chunk hold hits too (stale rows a broken mask would count)."""
    n, B, NC = 13, 6, 10
    rng = np.random.RandomState(7)
    t = rng.randint(0, NC, size=n).astype(np.int32)
    z = rng.randn(n, NC).astype(np.float32)
    z[np.arange(n), t] = 9.0
    if not last_hit:
        z[n - 1, (t[n - 1] + 1) % NC] = 10.0
    st = ops.eval_state("cpu", n)
    for c in range(3):
        zc, tc = chunk_inputs(z, t, B, c)
        stale = tc == PAD_LABEL
        tc[stale] = 3
        zc[stale] = 0.0
        zc[stale, 3] = 1.0
        ops.eval_metrics(torch.from_numpy(zc), torch.from_numpy(tc), 1, st)
    got = ops.eval_state_dict(st)
    want = (n, n if last_hit else n - 1)
    assert (got["count"], got["hits1"]) == want

    def padded(z_, t_):  # the same set with the stale rows where chunk_inputs puts the padding
        def rule_inputs(rule):
            count = hits = 0
            for c in range(3):
                zc, tc = chunk_inputs(z_, t_, B, c)
                stale = tc == PAD_LABEL
                tc[stale], zc[stale] = 3, 0.0
                zc[stale, 3] = 1.0
                v = rule(n, c, B)
                h1, _ = argsort_hits(zc[:v], tc[:v], 1)
                count, hits = count + v, hits + int(h1.sum())
            return count, hits
        return rule_inputs

    score = padded(z, t)
    right = lambda n_, c, B_: max(0, min(B_, n_ - c * B_))  # noqa: E731
    assert score(right) == want
    no_mask = lambda n_, c, B_: B_  # noqa: E731
    late = lambda n_, c, B_: max(0, min(B_, n_ - (c + 1) * B_))  # noqa: E731  cursor one ahead
    early = lambda n_, c, B_: max(0, min(B_, n_ - (c - 1) * B_)) if c else B_  # noqa: E731  cursor one behind
    for rule in (no_mask, late, early):
        count, hits = score(rule)
        assert count != want[0] and hits != want[1], (count, hits)


def test_k_outside_the_classes_raises():
    st = ops.eval_state("cpu", 4)
    z, t = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)
    for k in (0, 4):
        with pytest.raises(ValueError, match="eval_metrics"):
            ops.eval_metrics(z, t, k, st)
