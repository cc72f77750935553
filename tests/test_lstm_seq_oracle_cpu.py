"""The oracles and bounds of tests/test_lstm_seq_paths_gpu.py, checked without a GPU.

Agreement: the free-running float64 recurrence and the float64 BPTT equal float64 autograd through an
independently written BasicLSTMCell (the formulation of _tf_basic_lstm in test_models_cpu.py) to 1e-12.

Honesty: the project's fp32 CPU per-step path (ops.lstm_cell_fwd / ops.lstm_cell_bwd with float32 matmuls, and
again with the k-sum in reversed order) stays inside the teacher-forced and backward bounds on every case.

Sensitivity: every wrong kernel of lstm_seq_cases.FWD_MUTATIONS / BWD_MUTATIONS, expressed as a mutated
oracle whose values are rounded to fp32 as a kernel would store them, pushes at least one element outside
the bounds on every case it applies to - while the unmutated oracle, rounded the same way, stays inside.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_seq_cases as lc  # noqa: E402


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


FWD_GROUPS = {"grid": lc.fwd_grid_cases, "edges": lambda: [c for c, _ in lc.fwd_edge_cases()],
              "staged": lc.fwd_staged_cases, "saturating": lc.fwd_saturating_cases}


def _basic_lstm_autograd(x, h0, K, b, Hh, fb):
    """BasicLSTMCell unrolled in double with autograd; x [B][T][I].  Returns (z_t list, act, c, h per step)."""
    B, T, _ = x.shape
    h, c = h0, torch.zeros(B, Hh, dtype=torch.float64)
    zs, acts, cs, hs = [], [], [], []
    for t in range(T):
        g = torch.cat([x[:, t], h], 1) @ K + b
        g.retain_grad()
        i, j, f, o = g.split(Hh, 1)
        si, tj, sf, so = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + fb), torch.sigmoid(o)
        c = c * sf + si * tj
        h = torch.tanh(c) * so
        zs.append(g)
        acts.append(torch.cat([si, tj, sf, so], 1))
        cs.append(c)
        hs.append(h)
    return zs, acts, cs, hs


@pytest.mark.parametrize("T", [1, 2, 3, 28])
@pytest.mark.parametrize("nc", [0, 10])
def test_oracles_match_float64_autograd(T, nc):
    c = lc.FwdCase(16, T, None, lc.FBS[T % 3])
    b = lc.build_fwd(c)
    inp = b.inp
    ref = lc.fwd_free(inp)
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    K = td(inp["K"]).requires_grad_(True)
    zs, acts, cs, hs = _basic_lstm_autograd(td(inp["x"]).transpose(0, 1), td(inp["h0"]), K, td(inp["bias"]), c.hidden,
                                            inp["fb"])
    for t in range(T):
        assert np.abs(acts[t].detach().numpy() - ref["act"][t]).max() <= 1e-12
        assert np.abs(cs[t].detach().numpy() - ref["c"][t]).max() <= 1e-12
        h_ref = ref["xh"][t + 1][:, c.I:] if t + 1 < T else ref["hT"]
        assert np.abs(hs[t].detach().numpy() - h_ref).max() <= 1e-12
    rng = np.random.default_rng(T * 100 + nc)
    binp = {"K": inp["K"], "act": ref["act"], "c": ref["c"], "I": c.I, "H": c.hidden, "dhT": None, "dl": None, "wo": None}
    if nc:
        binp["dl"], binp["wo"] = lc._values(rng, (c.B, nc)), lc._values(rng, (c.hidden, nc))
        loss = ((hs[-1] @ td(binp["wo"])) * td(binp["dl"])).sum()
    else:
        binp["dhT"] = lc._values(rng, (c.B, c.hidden))
        loss = (hs[-1] * td(binp["dhT"])).sum()
    loss.backward()
    dg, bound = lc.bwd_oracle(binp)
    for t in range(T):
        want = zs[t].grad.numpy()
        assert np.abs(dg[t] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), t
    assert (bound >= 0).all() and np.isfinite(bound).all()


@pytest.mark.parametrize("group", list(FWD_GROUPS))
def test_cpu32_forward_inside_teacher_forced_bounds(group):
    worst = {}
    for c in FWD_GROUPS[group]():
        b = lc.build_fwd(c)
        for rev in (False, True):
            ok, got = lc.run_fwd(b, "cpu", reverse_k=rev)
            w = lc.check_fwd(b, got)
            for k in ("act", "c", "h"):
                worst[k] = max(worst.get(k, 0.0), w[k])
    print("%s: fp32 CPU path, largest err / bound: %s" % (group, worst))


@pytest.mark.parametrize("group", list(FWD_GROUPS))
def test_forward_bounds_catch_wrong_kernels(group):
    margin = {}
    for c in FWD_GROUPS[group]():
        b = lc.build_fwd(c)
        good = lc.as_stored(lc.fwd_free(b.inp))
        r = lc.fwd_teacher(b.inp, good["xh"], good["act"], good["c"], good["hT"])
        assert max(float(v.max()) for v in r.values()) <= 1.0, c
        for how in lc.FWD_MUTATIONS:
            if not lc.fwd_mutation_applies(c, how):
                continue
            bad = lc.as_stored(lc.fwd_free(b.inp, mutate=how))
            r = lc.fwd_teacher(b.inp, bad["xh"], bad["act"], bad["c"], bad["hT"])
            m = max(float(v.max()) for v in r.values())
            assert m > 1.0, "%s: %s stays inside the bounds (largest err / bound %.3g)" % (c, how, m)
            margin[how] = min(margin.get(how, np.inf), m)
    print("%s: smallest (largest err / bound) per mutation: %s" % (group, margin))


def test_every_forward_mutation_applies_somewhere():
    for how in lc.FWD_MUTATIONS:
        assert any(lc.fwd_mutation_applies(c, how) for c in lc.all_fwd_cases()), how
    for how in lc.BWD_MUTATIONS:
        assert any(lc.bwd_mutation_applies(c, how) for c in lc.bwd_cases()), how


def test_cpu32_free_running_error_is_small():
    """the yardstick of the free-running check: the fp32 CPU path against the float64 recurrence"""
    for c in (lc.FwdCase(128, 28, None, 1.0), lc.FwdCase(16, 254, None, 0.0)):
        b = lc.build_fwd(c)
        _, got = lc.run_fwd(b, "cpu")
        e = lc.fwd_free_errs(lc.fwd_free(b.inp), lc.logical(b, {k: got[k] for k in ("xh", "act", "c", "hT")}))
        for k, v in e.items():
            assert 0.0 < v.max() < 1e-5, (c, k, v.max())


def _bwd_chunks():
    cs = lc.bwd_cases()
    return [cs[i::4] for i in range(4)]


@pytest.mark.parametrize("chunk", range(4))
def test_cpu32_backward_inside_bounds_and_mutations_caught(chunk):
    worst, margin = 0.0, {}
    for c in _bwd_chunks()[chunk]:
        b = lc.build_bwd(c)
        ref = lc.bwd_oracle(b.inp)
        for rev in (False, True):
            ok, got = lc.run_bwd(b, "cpu", reverse_k=rev)
            worst = max(worst, lc.check_bwd(b, got, ref))
        assert lc.bwd_worst(b.inp, ref[0].astype(np.float32).astype(np.float64), ref) <= 1.0, c
        for how in lc.BWD_MUTATIONS:
            if not lc.bwd_mutation_applies(c, how):
                continue
            bad =lc.bwd_oracle(b.inp, mutate=how)[0].astype(np.float32).astype(np.float64)
            m = lc.bwd_worst(b.inp, bad, ref)
            assert m > 1.0, "%s: %s stays inside the bound (largest err / bound %.3g)" % (c, how, m)
            margin[how] = min(margin.get(how, np.inf), m)
    print("chunk %d: fp32 CPU path largest err / bound %.3g; smallest (largest err / bound) per mutation: %s" % (
        chunk, worst, margin))


def test_cell_cases_cpu32_inside_bounds():
    wf = wb = 0.0
    for c in lc.cell_cases():
        b = lc.build_cell_fwd(c)
        wf = max(wf, lc.check_cell_fwd(b, lc.run_cell_fwd(b, "cpu")))
        b = lc.build_cell_bwd(c)
        wb = max(wb, lc.check_cell_bwd(b, lc.run_cell_bwd(b, "cpu")))
    print("cell kernels, fp32 CPU path: forward %.3g, backward %.3g of the bound" % (wf, wb))


def test_expected_split_mirrors_the_dispatch_edges():
    es = lc.expected_split
    assert [es(B, 28, 28, None) for B in (16, 48, 128, 512, 528, 1024, 1040)] == [8, 8, 8, 8, 4, 4, 0]
    assert [es(B, 28, 28, "4") for B in (16, 48, 128, 528, 1024, 1040)] == [4, 4, 4, 4, 4, 0]
    assert [es(B, 28, 28, "1") for B in (512, 528)] == [8, 4]
    assert es(128, 28, 28, "8") == 8 and es(528, 3, 28, "8") == 4
    assert all(es(B, 28, 28, "0") == 0 for B in (16, 48, 128, 528))
    assert es(16, 254, 28, None) == 8 and es(16, 255, 28, None) == 0 and es(16, 254, 28, "4") == 4
    assert es(32, 3, 12, None) == 0 and es(24, 3, 28, None) == 0 and es(16, 3, 28, None, hidden=64) == 0
    for c, want in lc.fwd_edge_cases():
        assert es(c.B, c.T, c.I, c.split) == want, c
    assert lc.declines("fwd", 24, 28) and lc.declines("fwd", 16, 28, 64) and lc.declines("fwd", 32, 12)
    assert lc.declines("bwd", 32, 27) and not lc.declines("bwd", 32, 12) and not lc.declines("fwd", 1040, 28)


def test_case_lists_cover_what_they_claim():
    grid = lc.fwd_grid_cases()
    assert len(grid) == 36 and len(set(grid)) == 36
    for split in ("0", "4", None):
        assert {c.forget_bias for c in grid if c.split == split} == set(lc.FBS)
    assert {c.forget_bias for c in lc.all_fwd_cases()} == set(lc.FBS)
    assert len(lc.BWD_COMBOS) <= 12
    bw = lc.bwd_cases()
    assert {c.nc for c in bw} == {0, 1, 10, 16}
    assert {lc.expected_split(c.B, c.T, c.I, c.split) for c in bw} == {0, 4, 8}
    # the largest buffers stay small (act / dg: T * B * 4H floats)
    assert max(c.T * c.B * 4 * lc.H * 4 for c in lc.all_fwd_cases() + bw) <= 9 << 20
    for c in lc.all_fwd_cases() + bw:   # every launch inside what the launchers accept
        assert not lc.declines("fwd" if isinstance(c, lc.FwdCase) else "bwd", c.B, c.I, c.hidden), c
