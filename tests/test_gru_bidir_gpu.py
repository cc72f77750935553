"""The paired-direction GRU kernels (csrc/kernels/gru_bidir.hip) through torch.ops.dtfe_rnn and the GruBidirProgram step.
Reference: the float64 recurrence of tests/test_gru_cpu.py, for direction 1 on the sequence flipped along T with its
outputs flipped back (the flip moves the initial state from step T-1 to step 0, where gru_ref64 expects it).  Bound, as
tests/test_gru_seq_gpu.py: err_gpu <= 16 * max(e_cpu, 2^-23 max|ref|), e_cpu the error of the op's fp32 CPU path.
Largest err_gpu / max(..) measured on an MI355X when this file was added (31 tests, 2.8 s), direction 0 / 1: forward g
1.13 / 1.37, cand 1.19 / 1.68, h of xh 1.48 / 1.62, r*h of xrh 1.53 / 1.74, feat 1.56 / 2.16 (direction 1's mostly at B 16,
T 28, scale 4); backward dgg 1.23 / 1.00, dgc 1.00 / 1.01; step gradients <= 2.41, loss after 3 steps 0.32."""
import pytest
import torch
from test_gru_bidir_cpu import NAMES, bidir_loss64
from test_gru_cpu import gru_ref64
from test_gru_seq_gpu import _inputs, _ratio, _run

from dtfe import ops
from dtfe.models.lstm import H, I, NC, T as T_MODEL, LstmModel
from dtfe.optim import Optimizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
CELL = ("Wg", "bg", "Wc", "bc")
FWD = ("xh", "xrh") + tuple(k + "0" for k in CELL) + tuple(k + "1" for k in CELL) + ("g", "cand", "feat")
BWD = ("xh", "Wg0", "Wc0", "Wg1", "Wc1", "g", "cand", "dhT", "dgg", "dgc")
OUT = ("xh", "xrh", "g", "cand", "feat", "dgg", "dgc")


def _bidir_inputs(B, T, scale=1.0, In=I, Hn=H):
    """_inputs per direction (direction 1's weights, initial state and dhT half from another draw), stacked as the ops
    take them; every element to be written holds 7, the x columns of xh[1] included"""
    a, b = _inputs(B, T, scale, In, Hn), _inputs(B, T + 1, scale, In, Hn)
    d = {k + "0": a[k] for k in CELL}
    d.update({k + "1": b[k] for k in CELL})
    d.update({k: torch.full((2,) + a[k].shape, 7.0) for k in ("xh", "xrh", "g", "cand", "dgg", "dgc")})
    d["xh"][0], d["xh"][1, T - 1, :, In:] = a["xh"], b["xh"][0, :, In:]
    d.update(dhT=torch.cat([a["dhT"], b["dhT"]], 1), dl=a["dl"], wo=torch.cat([a["wo"], b["wo"]]),
             feat=torch.full((B, 2 * Hn), 7.0))
    return d


def _ref64(d, dfeat=None):
    """float64 buffers of both directions, named and laid out like the ops'"""
    Hn = d["Wc0"].shape[1]
    x1 = d["xh"][0].clone()
    x1[-1, :, -Hn:] = d["xh"][1, -1, :, -Hn:]
    half = (None, None) if dfeat is None else dfeat.split(Hn, 1)
    r0 = gru_ref64(d["xh"][0], *(d[k + "0"] for k in CELL), half[0])
    r1 = gru_ref64(x1.flip(0), *(d[k + "1"] for k in CELL), half[1])
    ref = {k: torch.stack([r0[k], r1[k].flip(0)]) for k in r0 if k != "hT"}
    ref["feat"] = torch.cat([r0["hT"], r1["hT"]], 1).detach()
    return ref


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("T", [1, 2, 3, 28])
@pytest.mark.parametrize("B", [16, 48])
def test_forward(B, T, scale):
    """T 1: no write-back, both initial rows are one time step; 2, 3: first reuse of the on-chip tiles in each
    direction; 28: the model's; B 48: three workgroups per direction"""
    d = _bidir_inputs(B, T, scale)
    (ok, gpu), (_, cpu) = _run(ops.gru_bidir_fwd, FWD, d, DEV), _run(ops.gru_bidir_fwd, FWD, d, "cpu")
    ref, x = _ref64(d), d["xh"][0, :, :, :I]
    assert ok and torch.equal(gpu["xh"][0, 0], d["xh"][0, 0]) and torch.equal(gpu["xh"][1, T - 1, :, I:], d["xh"][1, T - 1, :, I:])
    for k in ("xh", "xrh"):  # x columns of both directions: bitwise the input; the written columns: bounded
        assert torch.equal(gpu[k][0, :, :, :I], x) and torch.equal(gpu[k][1, :, :, :I], x), k
        gpu[k], cpu[k], ref[k] = gpu[k][..., I:], cpu[k][..., I:], ref[k][..., I:]
    for k in ("feat0", "feat1"):
        gpu[k], cpu[k], ref[k] = (v["feat"][:, int(k[-1]) * H:][:, :H] for v in (gpu, cpu, ref))
    print("forward", B, T, scale, {"%s[%d]" % (k, dd): _ratio(k, gpu[k][dd], cpu[k][dd], ref[k][dd])
                                   for k in OUT[:4] for dd in (0, 1)},
          {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in ("feat0", "feat1")})


@pytest.mark.parametrize("head", [False, True], ids=["dhT", "dl-wo"])
@pytest.mark.parametrize("T", [1, 3, 28])
@pytest.mark.parametrize("B", [16, 48])
def test_backward(B, T, head):
    d, kw = _bidir_inputs(B, T), (dict(dl=1, wo=1) if head else {})
    ref = _ref64(d, d["dl"].double() @ d["wo"].double().t() if head else d["dhT"])
    d.update({k: ref[k].float() for k in ("xh", "g", "cand")})  # the float64 forward rounded: the backward on its own
    (ok, gpu), (_, cpu) = _run(ops.gru_bidir_bwd, BWD, d, DEV, **kw), _run(ops.gru_bidir_bwd, BWD, d, "cpu", **kw)
    assert ok
    print("backward", B, T, head, {"%s[%d]" % (k, dd): _ratio(k, gpu[k][dd], cpu[k][dd], ref[k][dd])
                                   for k in OUT[5:] for dd in (0, 1)})


@pytest.mark.parametrize("op,names", [("gru_bidir_fwd", FWD), ("gru_bidir_bwd", BWD)])
def test_declined_shapes_and_bad_arguments_write_nothing(op, names):
    for B, In, Hn in ((24, I, H), (16, I, 64), (32, 12, H)):
        d = _bidir_inputs(B, 2, In=In, Hn=Hn)
        ok, got = _run(getattr(ops, op), names, d, DEV)
        assert ok is False and all(torch.equal(got[k], d[k]) for k in OUT), (B, In, Hn)
    fn, d = getattr(torch.ops.dtfe_rnn, op), {k: v.to(DEV) for k, v in _bidir_inputs(16, 2).items()}
    keep = {k: d[k].clone() for k in OUT}
    # a wrong dtype, a short g and a CPU tensor raise before anything is written; the valid call is accepted
    for bad in (dict(Wc1=d["Wc1"].double()), dict(g=d["g"][:, :1].contiguous()), dict(Wg0=d["Wg0"].cpu())):
        with pytest.raises(RuntimeError, match=op):
            fn(*(bad.get(k, d[k]) for k in names))
    assert all(torch.equal(d[k], keep[k]) for k in OUT)
    assert fn(*(d[k] for k in names)) is True and not torch.equal(d[names[-1]], keep[names[-1]])


def test_whole_step_gradients_and_three_sgd_steps():
    """GruBidirProgram at B = 16 against float64 autograd of the model, the CPU program as e_cpu: all ten gradients,
    then the loss after three SGD steps"""
    B, lr, g = 16, 0.1, torch.Generator().manual_seed(5)
    model = LstmModel(lr=lr, cell="gru", bidirectional=True)
    x, y = torch.rand(B, T_MODEL * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    progs, opts, loss, (cfg, names, _) = {}, {}, {}, model.opt_groups[0]
    for dev in ("cpu", DEV):
        p = progs[dev] = model.program(dev, B, seed=3)
        p.P.master.copy_(progs["cpu"].P.master)
        opts[dev] = Optimizer(cfg, p.P, var_list=names)
    w = [progs["cpu"].P.view(n).double().clone().requires_grad_() for n in NAMES]
    for k in range(4):  # the 4th loss is the loss after 3 optimizer steps
        for dev, p in progs.items():
            p.load_batch((x.to(dev), y.to(dev)))
            loss[dev] = torch.tensor(float(p.compute_grads()["loss"]), dtype=torch.float64)
        grads = torch.autograd.grad(l64 := bidir_loss64(x, y, w), w)
        if k == 0:
            print("gradients", {n: _ratio(n, progs[DEV].P.gview(n).cpu(), progs["cpu"].P.gview(n), gr)
                                for n, gr in zip(NAMES, grads)})
        for v, gr in zip(w, grads):
            v.data -= lr * gr
        for o in opts.values():
            o.step()
    print("loss after 3 steps", loss, l64.item(), _ratio("loss", loss[DEV], loss["cpu"], l64.detach()))
