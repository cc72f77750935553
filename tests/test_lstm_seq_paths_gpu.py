"""The persistent LSTM sequence kernels (lstm_seq.hip: single-workgroup, 4-way and 8-way split forward and
BPTT) and the per-step cell kernels against float64, inside guarded buffers, with derived bounds.

Cases, oracles, guards and bounds live in tests/lstm_seq_cases.py (its docstring states the bounds);
tests/test_lstm_seq_oracle_cpu.py proves on the CPU that the oracles equal float64 autograd, that the fp32 CPU
path stays inside every bound and that the bounds catch each listed wrong kernel.

Every launch goes through torch.ops.dtfe.lstm_seq_fwd / lstm_seq_bwd directly, with a non-zero gate bias,
forget_bias in {0, 1, 2.5} and (unstaged) a non-zero h_{-1}; after every launch lstm_last_split() must equal
the host mirror expected_split(...) of the dispatch - a silent fallback to the single kernel fails the test -
and every case ends with lstm_status(False) == 0.

Measured on an MI355X at the commit that added this file (37 tests, 6.8 s for the whole file; every case
launched the kernel expected_split names - the MI355X declined co-residency nowhere, B = 1024 x NS = 4 = 256
workgroups included - and no test exposed a bug in the kernels or launchers):

    largest err / bound, derived bounds            act     c       h       (teacher-forced forward)
        forward grid (36 cases)                    0.046   0.625   0.284
        dispatch edges (B 528 - 1040, T 254, 255)  0.043   0.642   0.289
        staging folded in                          0.041   0.647   0.294
        saturating (K x 8)                         0.056   0.625   0.272
        stale state across shapes                  0.040   0.592   0.280
      (c sits near 0.6 on the fp32 CPU path too: 3 U against the two roundings of c_prev * f + i * j.)
                                                   dhT     nc = 1  nc = 10  nc = 16   (running and teacher-forced dg)
        backward grid (12 x 4 cases)               0.336   0.318   0.194    0.259
        backward single kernel, B 1040 and I 12    0.29
        stale state across shapes (nc = 10)        0.181
        cell kernels                               forward 0.571, backward 0.823

    largest err_gpu / err_cpu32, free-running forward (limit 16)
        forward grid 1.03, dispatch edges 1.02, staging folded in 1.05, saturating 1.02, stale state 1.01
      the kernels' drift from the float64 recurrence is that of the fp32 CPU path: the activations dominate it,
      not the summation order, so the factor 16 has a wide margin.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_seq_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _exchange_clean():
    yield
    assert int(lc.ops.require().lstm_status(False)) == 0, "a split kernel's exchange timed out"


def _setenv(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("DTFE_LSTM_SPLIT", raising=False)
    else:
        monkeypatch.setenv("DTFE_LSTM_SPLIT", split)


def _fwd(c, monkeypatch, want=None):
    """run one forward case on the GPU and through the fp32 CPU path; every check; returns (worst, buffers)"""
    _setenv(monkeypatch, c.split)
    b = lc.build_fwd(c)
    ok, got = lc.run_fwd(b, DEV)
    ran = int(lc.ops.require().lstm_last_split())
    assert ok, c
    want = lc.expected_split(c.B, c.T, c.I, c.split) if want is None else want
    assert ran == want == lc.expected_split(c.B, c.T, c.I, c.split), "%s: launched NS = %d, expected %d" % (c, ran, want)
    _, cpu32 = lc.run_fwd(b, "cpu")
    return lc.check_fwd(b, got, cpu32), got


def _report(name, worst):
    keys = ("act", "c", "h", "free")
    print("%s: largest err / bound act %.3g, c %.3g, h %.3g; largest err_gpu / err_cpu32 %.3g" % (
        (name,) + tuple(max(w[k] for w in worst) for k in keys)))


@pytest.mark.parametrize("split", ["0", "4", None])
@pytest.mark.parametrize("B", [16, 48, 128])
def test_forward_grid(B, split, monkeypatch):
    """T in {1, 2, 3, 28}: T = 1 has no exchange, no xh write and no backward GEMM; T = 2, 3 both parities of the
    exchange slots and the first slot reuse.  B = 48: groups % 8 != 0 (consecutive workgroup ids per row group),
    B = 128: groups % 8 == 0 (the XCD-local mapping)."""
    cases = [c for c in lc.fwd_grid_cases() if c.B == B and c.split == split]
    assert [c.T for c in cases] == [1, 2, 3, 28]
    _report("forward B %d split %s" % (B, split), [_fwd(c, monkeypatch)[0] for c in cases])


@pytest.mark.parametrize("k", range(6))
def test_forward_dispatch_edges(k, monkeypatch):
    """the NS = 8 -> 4 switch at B = 528, forced 4 there, the last split size B = 1024, the single kernel past
    MAX_GROUPS, the largest split T = 254 (tags up to base + 254) and the single kernel at T = 255"""
    c, want = lc.fwd_edge_cases()[k]
    _report("forward edge %s" % (c,), [_fwd(c, monkeypatch, want)[0]])


@pytest.mark.parametrize("k", range(4))
def test_forward_staging_folded_in(k, monkeypatch):
    """xsrc / ysrc / ydst / zero0 / zero1: x columns of xh bitwise the transposed images, h_{-1} zeroed over NaN,
    labels copied, both accumulators cleared from non-zero (check_fwd), all forward bounds"""
    c = lc.fwd_staged_cases()[k]
    _report("forward staged %s" % (c,), [_fwd(c, monkeypatch)[0]])


@pytest.mark.parametrize("k", range(2))
def test_forward_saturating(k, monkeypatch):
    """K scaled by 8 more: gates saturate; everything finite (check_fwd), the same bounds, and past |z| = 18,
    where 1 + __expf(-z) and tanh round to 1 in fp32, the stored gate is exactly 1 (tanh: -1 on the other side).
    (|z| stays below 88 at this scale, so __expf itself never overflows: small sigmoids are small normal
    numbers, which the bounds cover.)"""
    c = lc.fwd_saturating_cases()[k]
    w, got = _fwd(c, monkeypatch)
    b = lc.build_fwd(c)
    d = lc.logical(b, {k_: got[k_] for k_ in ("xh", "act")})
    z = lc._with_fb(d["xh"].reshape(-1, c.I + c.hidden) @ b.inp["K"] + b.inp["bias"], c.hidden, b.inp["fb"])
    act = d["act"].reshape(z.shape)
    sig = np.ones(4 * c.hidden, dtype=bool)
    sig[c.hidden:2 * c.hidden] = False
    far = np.abs(z) > 18.0    # exp(-18) = 1.5e-8 < 2^-24 / 3: 1 + it rounds to 1 in fp32; 1 - tanh(18) = 4.6e-16
    assert far.sum() >= 10 and np.abs(z).max() < 80.0, "the case does not saturate as meant"
    assert (act[far & (z > 0)] == 1.0).all(), "%s: a saturated gate is not exactly 1" % (c,)
    neg = far & (z < 0)
    assert (act[neg & ~sig[None, :]] == -1.0).all(), "%s: a saturated tanh is not exactly -1" % (c,)
    _report("forward saturating %s" % (c,), [w])


def _bwd(c, monkeypatch):
    _setenv(monkeypatch, c.split)
    b = lc.build_bwd(c)
    ok, got = lc.run_bwd(b, DEV)
    ran = int(lc.ops.require().lstm_last_split())
    want = lc.expected_split(c.B, c.T, c.I, c.split)
    assert ok and ran == want, "%s: launched NS = %d, expected %d" % (c, ran, want)
    return lc.check_bwd(b, got), got


@pytest.mark.parametrize("combo", lc.BWD_COMBOS, ids=lambda v: "B%d-T%d-%s" % v)
def test_backward_grid(combo, monkeypatch):
    """each (B, T, split) with dh_T given (dhT) and formed in the kernel from dl / wo at nc = 1, 10, 16"""
    cases = [c for c in lc.bwd_cases() if (c.B, c.T, c.split) == combo and c.I == 28]
    assert [c.nc for c in cases] == list(lc.BWD_HEADS)
    worst = [_bwd(c, monkeypatch)[0] for c in cases]
    print("backward %s: largest err / bound per head %s" % (combo, ["%.3g" % w for w in worst]))


def test_backward_single_kernel_other_shapes(monkeypatch):
    """past MAX_GROUPS (B = 1040) and I = 12 (any (I + H) % 4 == 0 is accepted; split_ns keeps I != 28 off the
    split kernels, so unset and "0" both launch the single kernel)"""
    cases = [c for c in lc.bwd_cases() if c.I != 28 or c.B == 1040]
    assert len(cases) == 6 and all(lc.expected_split(c.B, c.T, c.I, c.split) == 0 for c in cases)
    worst = [_bwd(c, monkeypatch)[0] for c in cases]
    print("backward single-kernel shapes: largest err / bound %.3g" % max(worst))


def test_stale_exchange_state_across_shapes(monkeypatch):
    """Back-to-back launches of different B, NS and T in one process, nothing reset in between: stale words of
    another T parity and another NS layout must never match.  Every launch inside its bounds; the repeated
    first case bitwise equal to its first run."""
    seq = [(128, 3, None), (528, 2, None), (16, 28, "4"), (128, 3, None)]
    runs = []
    for (B, T, split) in seq:
        fc, bc = lc.FwdCase(B, T, split, 1.0), lc.BwdCase(B, T, split, 10)
        (wf, gf), (wb, gb) = _fwd(fc, monkeypatch), _bwd(bc, monkeypatch)
        runs.append((gf, gb))
        print("stale-state %s: forward %s, backward %.3g" % ((B, T, split), wf, wb))
    assert [lc.expected_split(B, T, 28, s) for (B, T, s) in seq] == [8, 4, 4, 8]
    for first, again in zip(runs[0], runs[3]):
        for k in first:
            assert lc.same_bits(first[k], again[k]), "repeat of the first case differs in %s" % k


def test_declined_shapes_leave_everything_untouched():
    """forward B = 24, H = 64, I = 12 and backward I = 27: the launcher returns False, lstm_last_split() is -1
    and every buffer, outputs and guards included, is bitwise as it was"""
    for c in (lc.FwdCase(24, 2), lc.FwdCase(16, 2, hidden=64), lc.FwdCase(32, 2, I=12)):
        assert lc.declines("fwd", c.B, c.I, c.hidden)
        b = lc.build_fwd(c)
        ok, got = lc.run_fwd(b, DEV)
        assert not ok and int(lc.ops.require().lstm_last_split()) == -1, c
        lc.check_untouched(b, got, list(got))
    c = lc.BwdCase(32, 2, None, 0, I=27)
    assert lc.declines("bwd", c.B, c.I, c.hidden)
    b = lc.build_bwd(c)
    ok, got = lc.run_bwd(b, DEV)
    assert not ok and int(lc.ops.require().lstm_last_split()) == -1, c
    lc.check_untouched(b, got, list(got))


def test_cell_kernels():
    """lstm_cell_fwd / lstm_cell_bwd on their own at B in {1, 37, 256}, H in {128, 96}: c_prev None / given, h_out
    strided (ld_h = I + H) / tight; dh2 None / given, dc_next None / given; the per-step bounds"""
    wf = wb = 0.0
    for c in lc.cell_cases():
        b = lc.build_cell_fwd(c)
        wf = max(wf, lc.check_cell_fwd(b, lc.run_cell_fwd(b, DEV)))
        b = lc.build_cell_bwd(c)
        wb = max(wb, lc.check_cell_bwd(b, lc.run_cell_bwd(b, DEV)))
    print("cell kernels: largest err / bound forward %.3g, backward %.3g" % (wf, wb))
