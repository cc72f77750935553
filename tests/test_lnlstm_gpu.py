"""The persistent layer-normalised LSTM kernels (csrc/kernels/lnlstm_seq.hip) through torch.ops.dtfe_rnn and the
LnLstmProgram step against the float64 recurrence of tests/test_lnlstm_cpu.py.  Bound: with e_cpu the largest absolute
error of the op's fp32 CPU path on the same inputs, err_gpu <= 16 * max(e_cpu, 2^-23 max|ref|), the LSTM and GRU
kernels' limit.  Largest err_gpu / max(..) measured on an MI355X when this file was added (28 tests, 2.5 s): forward
zhat 1.10, chat 1.13, rs 1.10, h of xh 1.78 (at B 16, T 28, scale 1), hT 1.27; backward dg 1.52, dln 1.37; step
gradients <= 1.39, loss after 3 steps 0.52."""
import pytest
import torch
from test_gru_seq_gpu import _ratio, _run  # (tests/ is on sys.path: rootdir conftest, no package)
from test_lnlstm_cpu import NAMES, lnlstm_ref64

from dtfe import ops
from dtfe.models.lstm import H, I, NC, LstmModel
from dtfe.optim import Optimizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD = ("xh", "K", "ln", "zhat", "chat", "rs", "hT")
BWD = ("K", "ln", "zhat", "chat", "rs", "dhT", "dg", "dln", "ws")
OUT = ("xh", "zhat", "chat", "rs", "hT", "dg", "dln")


def _inputs(B, T, scale=1.0, In=I, Hn=H):
    """random x and h_{-1}, a glorot kernel * ``scale`` (4: large pre-activations), gamma 1 +- 0.5, beta +- 0.5; every
    buffer to be written holds 7"""
    g, KT = torch.Generator().manual_seed(1000 * B + 10 * T + int(scale)), In + Hn
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ln = torch.rand(10, Hn, generator=g) - 0.5
    ln[0::2] += 1
    d = dict(xh=rnd(T, B, KT), K=(torch.rand(KT, 4 * Hn, generator=g) * 2 - 1) * scale * (6.0 / (KT + 4 * Hn)) ** 0.5, ln=ln,
             dhT=rnd(B, Hn), dl=rnd(B, NC) * 0.1, wo=rnd(Hn, NC), hT=torch.full((B, Hn), 7.0), dln=torch.full((10, Hn), 7.0),
             ws=torch.zeros(max(B // 16, 1), 10, Hn))
    d.update({k: torch.full((T, B, n), 7.0) for k, n in (("zhat", 4 * Hn), ("chat", Hn), ("rs", 5), ("dg", 4 * Hn))})
    d["xh"][1:, :, In:] = 7.0
    return d


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("T", [1, 2, 3, 28])
@pytest.mark.parametrize("B", [16, 48])
def test_forward(B, T, scale):
    """T 1: no write-back; 2, 3: first reuse of the tiles and of the carried normalised c; B 48: three workgroups;
    scale 4: large pre-activations, where an uncentred variance fails"""
    d = _inputs(B, T, scale)
    (ok, gpu), (_, cpu) = _run(ops.lnlstm_seq_fwd, FWD, d, DEV), _run(ops.lnlstm_seq_fwd, FWD, d, "cpu")
    ref = lnlstm_ref64(d["xh"], d["K"], d["ln"])
    ref["hT"] = ref["hT"].detach()
    assert ok and torch.equal(gpu["xh"][0], d["xh"][0]) and torch.equal(gpu["xh"][:, :, :I], d["xh"][:, :, :I])
    gpu["xh"], cpu["xh"], ref["xh"] = gpu["xh"][:, :, I:], cpu["xh"][:, :, I:], ref["xh"][:, :, I:]
    print("forward", B, T, scale, {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in OUT[:5]})


@pytest.mark.parametrize("B,T,head", [(16, 1, False), (16, 3, True), (16, 28, False), (48, 1, True), (48, 3, False),
                                      (48, 28, True)])
def test_backward(B, T, head):
    d, kw = _inputs(B, T), (dict(dl=1, wo=1) if head else {})
    ref = lnlstm_ref64(d["xh"], d["K"], d["ln"], d["dl"].double() @ d["wo"].double().t() if head else d["dhT"])
    d.update({k: ref[k].float() for k in ("zhat", "chat", "rs")})  # the float64 forward rounded: the backward on its own
    (ok, gpu), (_, cpu) = _run(ops.lnlstm_seq_bwd, BWD, d, DEV, **kw), _run(ops.lnlstm_seq_bwd, BWD, d, "cpu", **kw)
    assert ok
    print("backward", B, T, head, {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in OUT[5:]})
    if (B, T) == (48, 3):  # the slab reduce adds in a fixed order: a second run agrees bit for bit
        again = _run(ops.lnlstm_seq_bwd, BWD, d, DEV, **kw)[1]
        assert torch.equal(again["dln"], gpu["dln"]) and torch.equal(again["dg"], gpu["dg"])


@pytest.mark.parametrize("B,In,Hn", [(24, I, H), (16, I, 64), (16, 30, H)])
def test_declined_shapes_leave_every_output_untouched(B, In, Hn):
    d = _inputs(B, 2, In=In, Hn=Hn)
    for op, names in ((ops.lnlstm_seq_fwd, FWD), (ops.lnlstm_seq_bwd, BWD)):
        ok, got = _run(op, names, d, DEV)
        assert ok is False and all(torch.equal(got[k], d[k]) for k in OUT + ("ws",))


@pytest.mark.parametrize("op,names", [("lnlstm_seq_fwd", FWD), ("lnlstm_seq_bwd", BWD)])
def test_argument_checks(op, names):
    fn, d = getattr(torch.ops.dtfe_rnn, op), {k: v.to(DEV) for k, v in _inputs(16, 2).items()}
    keep = {k: d[k].clone() for k in OUT}
    # a wrong dtype, a short zhat and a CPU tensor raise before anything is written; the valid call is accepted
    for bad in (dict(K=d["K"].double()), dict(zhat=d["zhat"][:1].contiguous()), dict(ln=d["ln"].cpu())):
        with pytest.raises(RuntimeError, match=op):
            fn(*(bad.get(k, d[k]) for k in names))
    assert all(torch.equal(d[k], keep[k]) for k in OUT)
    out = "hT" if op == "lnlstm_seq_fwd" else "dln"
    assert fn(*(d[k] for k in names)) is True and not torch.equal(d[out], keep[out])


def test_whole_step_gradients_and_three_sgd_steps():
    """LnLstmProgram at B = 16 against float64 autograd of the model, the CPU program as e_cpu: all 13 gradients, the loss"""
    B, lr, g = 16, 0.1, torch.Generator().manual_seed(5)
    model = LstmModel(lr=lr, cell="lnlstm")
    x, y = torch.rand(B, 28 * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    progs, opts, loss, (cfg, names, _) = {}, {}, {}, model.opt_groups[0]
    for dev in ("cpu", DEV):
        p = progs[dev] = model.program(dev, B, seed=3)
        p.P.master.copy_(progs["cpu"].P.master)
        opts[dev] = Optimizer(cfg, p.P, var_list=names)
    w = [progs["cpu"].P.view(n).double().clone().requires_grad_() for n in NAMES[:3]]
    w.append(progs["cpu"].ln.double().clone().requires_grad_())
    xh, f64 = torch.zeros(28, B, I + H), dict(dtype=torch.float64)
    xh[:, :, :I] = x.reshape(B, 28, I).transpose(0, 1)
    for k in range(4):  # the 4th loss is the loss after 3 optimizer steps
        for dev, p in progs.items():
            p.load_batch((x.to(dev), y.to(dev)))
            loss[dev] = torch.tensor(float(p.compute_grads()["loss"]), **f64)
        l64 = -(torch.log_softmax(lnlstm_ref64(xh, w[2], w[3])["hT"] @ w[0] + w[1], 1) * y.double()).sum(1).mean()
        grads = torch.autograd.grad(l64, w)
        if k == 0:
            per_var = list(grads[:3]) + list(grads[3])  # the ten gamma / beta rows, in variable order
            print("gradients", {n: _ratio(n, progs[DEV].P.gview(n).cpu(), progs["cpu"].P.gview(n), gr)
                                for n, gr in zip(NAMES, per_var)})
        for v, gr in zip(w, grads):
            v.data -= lr * gr
        for o in opts.values():
            o.step()
    print("loss after 3 steps", loss, l64.item(), _ratio("loss", loss[DEV], loss["cpu"], l64.detach()))
