"""The persistent GRU kernels (csrc/kernels/gru_seq.hip) through torch.ops.dtfe_rnn and the GruProgram step against
the float64 recurrence of tests/test_gru_cpu.py.  Bound: with e_cpu the largest absolute error of the op's fp32 CPU
path on the same inputs, err_gpu <= 16 * max(e_cpu, 2^-23 max|ref|), the LSTM kernels' limit.  Largest err_gpu / max(..)
measured on an MI355X when this file was added (34 tests, 2.6 s): forward g 1.30, cand 1.76, hT 2.96, h of xh 1.92, r*h
of xrh 1.72 (at B 16, T 28, scale 4); backward dgg 1.23, dgc 1.00; step gradients <= 1.24, loss after 3 steps 0.32."""
import pytest
import torch
from test_gru_cpu import gru_ref64  # (tests/ is on sys.path: rootdir conftest, no package)

from dtfe import ops
from dtfe.models.lstm import H, I, NC, LstmModel
from dtfe.optim import Optimizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD = ("xh", "xrh", "Wg", "bg", "Wc", "bc", "g", "cand", "hT")
BWD = ("xh", "Wg", "Wc", "g", "cand", "dhT", "dgg", "dgc")
OUT = ("xh", "xrh", "g", "cand", "hT", "dgg", "dgc")


def _inputs(B, T, scale=1.0, In=I, Hn=H):
    """random x, h_{-1}, biases, glorot kernels * ``scale`` (4 saturates); every buffer to be written holds 7; nc = 10"""
    g, KT = torch.Generator().manual_seed(1000 * B + 10 * T + int(scale)), In + Hn
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    glorot = lambda n: (torch.rand(KT, n, generator=g) * 2 - 1) * scale * (6.0 / (KT + n)) ** 0.5  # noqa: E731
    d = dict(xh=rnd(T, B, KT), Wg=glorot(2 * Hn), bg=rnd(2 * Hn) * 0.5, Wc=glorot(Hn), bc=rnd(Hn) * 0.5,
             dhT=rnd(B, Hn), dl=rnd(B, NC) * 0.1, wo=rnd(Hn, NC), hT=torch.full((B, Hn), 7.0))
    d.update({k: torch.full((T, B, n), 7.0) for k, n in zip(OUT[1:4] + OUT[5:], (KT, 2 * Hn, Hn, 2 * Hn, Hn))})
    d["xh"][1:, :, In:] = 7.0
    return d


def _run(op, names, d, dev, **kw):
    d = {k: v.clone().to(dev) for k, v in d.items()}
    ok = op(*(d[k] for k in names), **{k: d[k] for k in kw})
    return ok, {k: v.cpu() for k, v in d.items()}


def _ratio(name, gpu, cpu32, ref):
    e_gpu, e_cpu = (gpu.double() - ref).abs().max().item(), (cpu32.double() - ref).abs().max().item()
    ratio = e_gpu / max(e_cpu, 2.0 ** -23 * ref.abs().max().item())
    assert ratio <= 16.0, "%s: err_gpu %.3g, e_cpu %.3g, ratio %.3g > 16" % (name, e_gpu, e_cpu, ratio)  # (NaN fails)
    return round(ratio, 3)


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("T", [1, 2, 3, 28])
@pytest.mark.parametrize("B", [16, 48])
def test_forward(B, T, scale):
    """T 1: no recurrent write-back; 2, 3: first reuse of the h / r*h tiles; 28: the model's; B 48: three workgroups"""
    d = _inputs(B, T, scale)
    (ok, gpu), (_, cpu) = _run(ops.gru_seq_fwd, FWD, d, DEV), _run(ops.gru_seq_fwd, FWD, d, "cpu")
    ref = gru_ref64(d["xh"], d["Wg"], d["bg"], d["Wc"], d["bc"])
    assert ok and torch.equal(gpu["xh"][0], d["xh"][0])
    for k in ("xh", "xrh"):  # x columns: bitwise the inputs; the written columns: bounded
        assert torch.equal(gpu[k][:, :, :I], d["xh"][:, :, :I]), k
        gpu[k], cpu[k], ref[k] = gpu[k][:, :, I:], cpu[k][:, :, I:], ref[k][:, :, I:]
    print("forward", B, T, scale, {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in OUT[:5]})


@pytest.mark.parametrize("head", [False, True], ids=["dhT", "dl-wo"])
@pytest.mark.parametrize("T", [1, 3, 28])
@pytest.mark.parametrize("B", [16, 48])
def test_backward(B, T, head):
    d, kw = _inputs(B, T), (dict(dl=1, wo=1) if head else {})
    ref = gru_ref64(d["xh"], d["Wg"], d["bg"], d["Wc"], d["bc"],
                    d["dl"].double() @ d["wo"].double().t() if head else d["dhT"])
    d.update({k: ref[k].float() for k in ("xh", "g", "cand")})  # the float64 forward rounded: the backward on its own
    (ok, gpu), (_, cpu) = _run(ops.gru_seq_bwd, BWD, d, DEV, **kw), _run(ops.gru_seq_bwd, BWD, d, "cpu", **kw)
    assert ok
    print("backward", B, T, head, {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in OUT[5:]})


@pytest.mark.parametrize("B,In,Hn", [(24, I, H), (16, I, 64), (32, 12, H)])
def test_declined_shapes_leave_every_output_untouched(B, In, Hn):
    d = _inputs(B, 2, In=In, Hn=Hn)
    for op, names in ((ops.gru_seq_fwd, FWD), (ops.gru_seq_bwd, BWD)):
        ok, got = _run(op, names, d, DEV)
        assert ok is False and all(torch.equal(got[k], d[k]) for k in OUT)


@pytest.mark.parametrize("op,names", [("gru_seq_fwd", FWD), ("gru_seq_bwd", BWD)])
def test_argument_checks(op, names):
    fn, d = getattr(torch.ops.dtfe_rnn, op), {k: v.to(DEV) for k, v in _inputs(16, 2).items()}
    keep = {k: d[k].clone() for k in OUT}
    # a wrong dtype, a short g and a CPU tensor raise before anything is written; the valid call is accepted
    for bad in (dict(Wc=d["Wc"].double()), dict(g=d["g"][:1].contiguous()), dict(Wg=d["Wg"].cpu())):
        with pytest.raises(RuntimeError, match=op):
            fn(*(bad.get(k, d[k]) for k in names))
    assert all(torch.equal(d[k], keep[k]) for k in OUT)
    assert fn(*(d[k] for k in names)) is True and not torch.equal(d[names[-1]], keep[names[-1]])


def test_whole_step_gradients_and_three_sgd_steps():
    """GruProgram at B = 16 against float64 autograd of the model, the CPU program as e_cpu: all six gradients, the loss"""
    B, lr, g = 16, 0.1, torch.Generator().manual_seed(5)
    model = LstmModel(lr=lr, cell="gru")
    x, y = torch.rand(B, 28 * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    progs, opts, loss, (cfg, names, _) = {}, {}, {}, model.opt_groups[0]
    for dev in ("cpu", DEV):
        p = progs[dev] = model.program(dev, B, seed=3)
        p.P.master.copy_(progs["cpu"].P.master)
        opts[dev] = Optimizer(cfg, p.P, var_list=names)
    w = [progs["cpu"].P.view(n).double().clone().requires_grad_() for n in names]
    xh, f64 = torch.zeros(28, B, I + H), dict(dtype=torch.float64)
    xh[:, :, :I] = x.reshape(B, 28, I).transpose(0, 1)
    for k in range(4):  # the 4th loss is the loss after 3 optimizer steps
        for dev, p in progs.items():
            p.load_batch((x.to(dev), y.to(dev)))
            loss[dev] = torch.tensor(float(p.compute_grads()["loss"]), **f64)
        l64 = -(torch.log_softmax(gru_ref64(xh, *w[2:])["hT"] @ w[0] + w[1], 1) * y.double()).sum(1).mean()
        grads = torch.autograd.grad(l64, w)
        if k == 0:
            print("gradients", {n: _ratio(n, progs[DEV].P.gview(n).cpu(), progs["cpu"].P.gview(n), gr)
                                for n, gr in zip(names, grads)})
        for v, gr in zip(w, grads):
            v.data -= lr * gr
        for o in opts.values():
            o.step()
    print("loss after 3 steps", loss, l64.item(), _ratio("loss", loss[DEV], loss["cpu"], l64.detach()))
