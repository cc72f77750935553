"""The eval_metrics kernel against the host mirror and the float64 oracle, launch by launch: counters exact,
loss within the derived bound (eval_metrics_cases), next-chunk indices, past-the-end launches, bitwise
reproducibility eagerly and under graph replay."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_metrics_cases import chunk_inputs, make_set, oracle_rows, row_bounds, set_bound  # noqa: E402

from dtfe import ops  # noqa: E402
from dtfe.utils.graphs import StepGraph  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, NC, k); (256, 10, 5) is 64 workgroups: the ticket path with many arrivals
SHAPES = [(6, 10, 1), (6, 10, 5), (7, 3, 3), (5, 70, 5), (4, 1000, 5), (130, 10, 1), (256, 10, 5)]
EXACT = ("cursor", "n", "count", "hits1", "hitsk", "bad_labels")


def _buffers(B, NC, n):
    return dict(z=torch.empty(B, NC, device=DEV), t=torch.empty(B, dtype=torch.int32, device=DEV),
                state=ops.eval_state(DEV, n), idx=torch.full((B,), -1, dtype=torch.int32, device=DEV),
                ws=torch.zeros(2 * B, dtype=torch.int32, device=DEV),
                ticket=torch.zeros(1, dtype=torch.int32, device=DEV))


def _run_gpu(z, t, B, k, launches, graph=False):
    """The state words (int64, loss bits included) and idx after every launch."""
    n, NC = z.shape
    b = _buffers(B, NC, n)

    def launch():
        ops.eval_metrics(b["z"], b["t"], k, b["state"], idx=b["idx"], ws=b["ws"], ticket=b["ticket"])

    runner = StepGraph(launch, warmup=0) if graph else launch
    out = []
    for c in range(launches):
        zc, tc = chunk_inputs(z, t, B, c)
        b["z"].copy_(torch.from_numpy(zc))
        b["t"].copy_(torch.from_numpy(tc))
        runner()
        out.append((b["state"].cpu().clone(), b["idx"].cpu().clone()))
    if graph:
        assert runner.capture_error is None and runner.graph is not None
    assert int(b["ticket"].item()) == 0
    return out


@pytest.mark.parametrize("nan_target", (False, True))
@pytest.mark.parametrize("B,NC,k", SHAPES)
def test_eval_metrics_launch_by_launch(B, NC, k, nan_target):
    z, t = make_set(B, NC, seed=B * NC + k, nan_target=nan_target)
    n = z.shape[0]
    chunks = -(-n // B)
    launches = chunks + 2  # the last two run past the end: they change nothing
    good = (t >= 0) & (t < NC)
    nan_rows = np.isnan(z[np.arange(n), np.where(good, t, 0)]) & good
    fin = good & ~nan_rows
    ref, bnd = np.zeros(n), np.zeros(n)
    ref[fin], bnd[fin] = oracle_rows(z[fin], t[fin]), row_bounds(z[fin], t[fin])
    mirror = ops.eval_state("cpu", n)
    midx = torch.full((B,), -1, dtype=torch.int32)
    got = _run_gpu(z, t, B, k, launches)
    for c in range(launches):
        zc, tc = chunk_inputs(z, t, B, c)
        ops.eval_metrics(torch.from_numpy(zc), torch.from_numpy(tc), k, mirror, idx=midx)
        want, have = ops.eval_state_dict(mirror), ops.eval_state_dict(got[c][0])
        rows = min(n, (c + 1) * B)
        print(B, NC, k, "launch", c, have, "mirror loss", want["loss_sum"])
        for w in EXACT:
            assert have[w] == want[w], (w, c, have, want)
        assert have["cursor"] == min(c + 1, chunks) and have["count"] == rows
        assert torch.equal(got[c][1], midx), c
        if nan_rows[:rows].any():
            assert math.isnan(have["loss_sum"]) and math.isnan(want["loss_sum"])
        else:
            sel = fin[:rows]
            err = abs(have["loss_sum"] - math.fsum(ref[:rows][sel]))
            bound = set_bound(ref[:rows][sel], bnd[:rows][sel])
            print("   loss error %.3e, bound %.3e" % (err, bound))
            assert err <= bound
    assert ops.eval_state_dict(got[-1][0])["bad_labels"] == 1
    assert torch.equal(got[-1][0], got[chunks - 1][0]) and torch.equal(got[-1][1], got[chunks - 1][1])


@pytest.mark.parametrize("B,NC,k", SHAPES)
def test_eval_metrics_is_bitwise_reproducible_eager_and_replayed(B, NC, k):
    z, t = make_set(B, NC, seed=B * NC + k)
    launches = -(-z.shape[0] // B) + 2
    a = _run_gpu(z, t, B, k, launches)
    b = _run_gpu(z, t, B, k, launches)
    g = _run_gpu(z, t, B, k, launches, graph=True)
    for c in range(launches):
        assert torch.equal(a[c][0], b[c][0]) and torch.equal(a[c][1], b[c][1]), c  # int64 words: loss bits too
        assert torch.equal(a[c][0], g[c][0]) and torch.equal(a[c][1], g[c][1]), c


def test_eval_metrics_argument_checks():
    b = _buffers(4, 3, 4)
    b["z"].zero_()
    b["t"].zero_()
    for k in (0, 4):
        with pytest.raises(ValueError, match="eval_metrics"):
            ops.eval_metrics(b["z"], b["t"], k, b["state"], idx=b["idx"], ws=b["ws"], ticket=b["ticket"])
    with pytest.raises(RuntimeError, match="eval_metrics"):
        ops.eval_metrics(b["z"], b["t"], 1, b["state"], idx=b["idx"], ws=b["ws"][:4], ticket=b["ticket"])
    with pytest.raises(RuntimeError, match="eval_metrics"):
        ops.eval_metrics(b["z"], b["t"].long(), 1, b["state"], idx=b["idx"], ws=b["ws"], ticket=b["ticket"])
