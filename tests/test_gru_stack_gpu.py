"""The stacked-layer GRU kernels (gru_proj_fwd, gru_stack_bwd in csrc/kernels/gru_seq.hip) and the GruStackProgram step
against float64, with the inputs, runner and bound of tests/test_gru_seq_gpu.py: err_gpu <= 16 * max(e_cpu, 2^-23 max|ref|),
e_cpu the error of the op's fp32 CPU path on the same inputs.  Largest err_gpu / max(..) measured on an MI355X when this
file was added (32 tests, under 2 s): projected forward g 1.76, cand 1.63, hT 2.62 (B 48, T 28, scale 1), h of xh 1.63,
r*h of xrh 1.89; backward with dhs dgg 1.00, dgc 1.24; step gradients <= 1.69 (L 2) / 1.76 (L 3), loss after 3 steps 0.32 / 0.62."""
import itertools

import pytest
import torch
from test_gru_cpu import gru_ref64  # (tests/ is on sys.path: rootdir conftest, no package)
from test_gru_seq_gpu import _inputs, _ratio, _run
from test_gru_stack_cpu import stack_ref64

from dtfe import ops
from dtfe.models.lstm import H, I, NC, T as T_MODEL, LstmModel
from dtfe.optim import Optimizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD = ("xh", "xrh", "xpg", "xpc", "Wg", "Wc", "g", "cand", "hT")
BWD = ("xh", "Wg", "Wc", "g", "cand", "dgg", "dgc")
OUT = ("xh", "xrh", "g", "cand", "hT", "dgg", "dgc", "h2")
MODES = (("dhs",), ("dhs", "dhT"), ("dhs", "dl", "wo"))


def _stack_inputs(B, T, scale=1.0, In=H, Hn=H):
    """test_gru_seq_gpu's inputs, plus the float64 projections rounded, a gradient at every step, a second h destination"""
    d = _inputs(B, T, scale, In=In, Hn=Hn)
    proj = lambda W, b: (d["xh"][:, :, :In].double() @ d[W][:In].double() + d[b].double()).float()  # noqa: E731
    d.update(xpg=proj("Wg", "bg"), xpc=proj("Wc", "bc"), h2=torch.full((T, B, In + Hn), 7.0),
             dhs=torch.randn(T, B, Hn, generator=torch.Generator().manual_seed(B + T)))
    return d


@pytest.mark.parametrize("B,T,scale", itertools.product((16, 48), (1, 2, 3, 28), (1.0, 4.0)))
def test_projected_forward(B, T, scale):
    """T 1: no write-back; 2, 3: first reuse of the tiles and of the projection fetched ahead; B 48: three workgroups"""
    d = _stack_inputs(B, T, scale)
    (ok, gpu), (_, cpu) = _run(ops.gru_proj_fwd, FWD, d, DEV, h2=1), _run(ops.gru_proj_fwd, FWD, d, "cpu", h2=1)
    ref = gru_ref64(d["xh"], d["Wg"], d["bg"], d["Wc"], d["bc"])
    assert ok and torch.equal(gpu["xh"][0], d["xh"][0])
    hseq = torch.cat([gpu["xh"][1:, :, H:], gpu["hT"][None]])  # h_0 .. h_{T-1}: the second destination, bit for bit
    assert torch.equal(gpu["h2"][:, :, :H], hseq) and bool((gpu["h2"][:, :, H:] == 7).all())
    for k in ("xh", "xrh"):  # x columns: bitwise the inputs; the written columns: bounded
        assert torch.equal(gpu[k][:, :, :H], d["xh"][:, :, :H]), k
        gpu[k], cpu[k], ref[k] = gpu[k][:, :, H:], cpu[k][:, :, H:], ref[k][:, :, H:]
    print("forward", B, T, scale, {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in OUT[:5]})


def _bptt_ref64(d, mode, In):
    """float64 recurrence from d's xh (x, h_{-1}) and autograd of sum_t h_t . dhs[t] + h_T . dh_T: xh, g, cand, dgg, dgc"""
    Wg, bg, Wc, bc = (d[k].double() for k in ("Wg", "bg", "Wc", "bc"))
    x, h, hs, zg, zc = d["xh"][:, :, :In].double(), d["xh"][0, :, In:].double(), [], [], []
    for t in range(x.shape[0]):
        hs.append(h)
        zg.append((torch.cat([x[t], h], 1) @ Wg + bg).requires_grad_())
        r, u = torch.sigmoid(zg[t]).split(H, 1)
        zc.append((torch.cat([x[t], r * h], 1) @ Wc + bc).requires_grad_())
        h = u * h + (1 - u) * torch.tanh(zc[t])
    dhT = d["dl"].double() @ d["wo"].double().t() if "dl" in mode else d["dhT"].double() if "dhT" in mode else 0.0
    loss = (torch.stack(hs[1:] + [h]) * d["dhs"].double()).sum() + (h * dhT).sum()
    grads, T = torch.autograd.grad(loss, zg + zc), x.shape[0]
    return dict(xh=torch.cat([x, torch.stack(hs).detach()], 2), g=torch.sigmoid(torch.stack(zg)).detach(),
                cand=torch.tanh(torch.stack(zc)).detach(), dgg=torch.stack(grads[:T]), dgc=torch.stack(grads[T:]))


@pytest.mark.parametrize("In,B,T,mode", [c + (MODES[(i + i // 3) % 3],) for i, c in
                                         enumerate(itertools.product((28, H), (16, 48), (1, 3, 28)))])
def test_backward_with_a_gradient_at_every_step(In, B, T, mode):
    d, kw = _stack_inputs(B, T, In=In), dict.fromkeys(mode, 1)
    ref = _bptt_ref64(d, mode, In)
    d.update({k: ref[k].float() for k in ("xh", "g", "cand")})  # the float64 forward rounded: the backward on its own
    (ok, gpu), (_, cpu) = _run(ops.gru_stack_bwd, BWD, d, DEV, **kw), _run(ops.gru_stack_bwd, BWD, d, "cpu", **kw)
    print("backward", In, B, T, mode, ok and {k: _ratio(k, gpu[k], cpu[k], ref[k]) for k in ("dgg", "dgc")})
    assert ok


@pytest.mark.parametrize("op,names,kw,bad", [("gru_proj_fwd", FWD, ("h2",), "xpg"), ("gru_stack_bwd", BWD, ("dhs", "dhT"), "dhs")])
def test_declined_shapes_and_bad_arguments_write_nothing(op, names, kw, bad):
    for B, In, Hn in ((24, H, H), (16, H, 64), (32, 30, H)):
        d = _stack_inputs(B, 2, In=In, Hn=Hn)
        ok, got = _run(getattr(ops, op), names, d, DEV, **dict.fromkeys(kw, 1))
        assert ok is False and all(torch.equal(got[k], d[k]) for k in OUT), (B, In, Hn)
    d = {k: v.to(DEV) for k, v in _stack_inputs(16, 2).items()}
    fn = lambda **o: getattr(torch.ops.dtfe_rnn, op)(*(o.get(k, d[k]) for k in names), **{k: o.get(k, d[k]) for k in kw})  # noqa: E731
    keep = {k: d[k].clone() for k in OUT}
    for wrong in (d[bad].double(), d[bad].cpu()):  # a wrong dtype and a CPU tensor raise before anything is written
        with pytest.raises(RuntimeError, match=op):
            fn(**{bad: wrong})
    assert all(torch.equal(d[k], keep[k]) for k in OUT) and fn() is True and not torch.equal(d[names[-1]], keep[names[-1]])


@pytest.mark.parametrize("L", [2, 3])
def test_whole_step_gradients_and_three_sgd_steps(L):
    """GruStackProgram at B = 16 against float64 autograd of the model, the CPU program as e_cpu; then 3 SGD steps"""
    B, lr, g, model = 16, 0.1, torch.Generator().manual_seed(5), LstmModel(lr=0.1, cell="gru", layers=L)
    x, y = torch.rand(B, T_MODEL * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    progs, opts, loss, (cfg, names, _) = {}, {}, {}, model.opt_groups[0]
    for dev in ("cpu", DEV):
        p = progs[dev] = model.program(dev, B, seed=3)
        p.P.master.copy_(progs["cpu"].P.master)
        opts[dev] = Optimizer(cfg, p.P, var_list=names)
    w = [progs["cpu"].P.view(n).double().clone().requires_grad_() for n in names]  # all 2 + 4 L variables
    for k in range(4):  # the 4th loss is the loss after 3 optimizer steps
        for dev, p in progs.items():
            p.load_batch((x.to(dev), y.to(dev)))
            loss[dev] = torch.tensor(float(p.compute_grads()["loss"]), dtype=torch.float64)
        grads = torch.autograd.grad(l64 := stack_ref64(x.reshape(B, T_MODEL, I).transpose(0, 1), y, w), w)
        if k == 0:
            print("gradients", L, {n: _ratio(n, progs[DEV].P.gview(n).cpu(), progs["cpu"].P.gview(n), gr)
                                   for n, gr in zip(names, grads)})
        for v, gr in zip(w, grads):
            v.data -= lr * gr
        for o in opts.values():
            o.step()
    print("loss after 3 steps", L, loss, l64.item(), _ratio("loss", loss[DEV], loss["cpu"], l64.detach()))
