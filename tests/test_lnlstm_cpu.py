"""The layer-normalised LSTM cell (--cell lnlstm) off the GPU: the model's TF1 variables, the CPU program's gradients
against the float64 autograd recurrence lnlstm_ref64 (also the oracle of tests/test_lnlstm_gpu.py), and the CLI end to
end.  Bound of fp32 against float64 as in tests/test_gru_cpu.py: 4 * 256 * 2^-23 * max|ref|."""
import re

import pytest
import torch

from dtfe import ckpt, train
from dtfe.models.lstm import H, I, LN_SCOPES, NC, LnLstmProgram, LstmModel

PRE = "rnn/layer_norm_basic_lstm_cell/"
NAMES = ["Variable", "Variable_1", PRE + "kernel"] + [PRE + s + "/" + v for s in LN_SCOPES for v in ("gamma", "beta")]


def lnlstm_ref64(xh, K, ln, dhT=None, forget_bias=1.0):
    """float64 autograd LayerNormBasicLSTMCell recurrence over xh [T][B][I+H] (x_t; h_{-1} in step 0's h columns,
    c_{-1} = 0), named like the kernels' buffers; given dh_T also dg = d sum(h_T dh_T) / d z and dln.  float64 K / ln
    that require grad stay in the graph: hT is differentiable, the other buffers are detached."""
    xh, (K, ln) = xh.detach().double(), (v if v.requires_grad else v.detach().double().requires_grad_() for v in (K, ln))
    T, B, Hn = xh.shape[0], xh.shape[1], ln.shape[1]
    x, h, c, hs, zs, zh, chs, rs = xh[:, :, :-Hn], xh[0, :, -Hn:].clone(), 0.0, [], [], [], [], []

    def norm(v):
        d = v - v.mean(-1, keepdim=True)
        r = ((d * d).mean(-1, keepdim=True) + 1e-12) ** -0.5
        return d * r, r.squeeze(-1)

    for t in range(T):
        hs.append(h)
        zs.append(torch.cat([x[t], h], 1) @ K)
        n, r = norm(zs[t].view(B, 4, Hn))
        y = n * ln[0:8:2] + ln[1:8:2]
        ch, rc = norm(c * torch.sigmoid(y[:, 2] + forget_bias) + torch.sigmoid(y[:, 0]) * torch.tanh(y[:, 1]))
        c = ln[8] * ch + ln[9]
        h = torch.tanh(c) * torch.sigmoid(y[:, 3])
        zh.append(n.reshape(B, 4 * Hn)), chs.append(ch), rs.append(torch.cat([r, rc[:, None]], 1))
    out = dict(xh=torch.cat([x, torch.stack(hs)], 2).detach(), zhat=torch.stack(zh).detach(),
               chat=torch.stack(chs).detach(), rs=torch.stack(rs).detach(), hT=h)
    if dhT is not None:
        grads = torch.autograd.grad((h * dhT.double()).sum(), zs + [ln], retain_graph=True)
        out.update(dg=torch.stack(grads[:T]), dln=grads[T])
    return out


def _close(got, ref, name):
    err, bound = (got.double() - ref).abs().max().item(), 4 * 256 * 2.0 ** -23 * ref.abs().max().item()
    assert err <= bound, "%s: err %.3g > bound %.3g" % (name, err, bound)


def test_variables_shapes_and_initial_values():
    m = LstmModel(cell="lnlstm")
    assert m.var_order == NAMES + ["Variable_2"] and [s.name for s in m.specs] == NAMES  # (no bias variable)
    assert [tuple(s.shape) for s in m.specs] == [(H, NC), (NC,), (I + H, 4 * H)] + [(H,)] * 10
    prog = m.program("cpu", 4, seed=0)
    v = [prog.P.view(n) for n in NAMES]
    assert isinstance(prog, LnLstmProgram)
    assert all(bool((g == 1).all()) and bool((b == 0).all()) for g, b in zip(v[3::2], v[4::2]))
    assert 0.9 < v[2].abs().max().item() / (6.0 / sum(v[2].shape)) ** 0.5 <= 1  # glorot-uniform


def test_cpu_program_gradients_against_float64_autograd():
    B, g = 4, torch.Generator().manual_seed(11)
    prog = LstmModel(cell="lnlstm").program("cpu", B, seed=2)
    prog.ln.copy_(torch.stack([1 + torch.rand(H, generator=g) - 0.5 if i % 2 == 0 else torch.rand(H, generator=g) - 0.5
                               for i in range(10)]))  # gamma 1 +- 0.5, beta +- 0.5: a swapped scale or shift shows
    x, y = torch.rand(B, 28 * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    prog.load_batch((x, y))
    loss = float(prog.compute_grads()["loss"])
    w = [prog.P.view(n).double().clone().requires_grad_() for n in NAMES[:3]] + [prog.ln.double().clone().requires_grad_()]
    xh = torch.zeros(28, B, I + H)
    xh[:, :, :I] = x.reshape(B, 28, I).transpose(0, 1)
    l64 = -(torch.log_softmax(lnlstm_ref64(xh, w[2], w[3])["hT"] @ w[0] + w[1], 1) * y.double()).sum(1).mean()
    grads = torch.autograd.grad(l64, w)
    _close(torch.tensor(loss), l64.detach(), "loss")
    for n, gr in zip(NAMES[:3], grads):
        _close(prog.P.gview(n), gr, n)
    for i, n in enumerate(NAMES[3:]):
        _close(prog.P.gview(n), grads[3][i], n)


def test_cli_checkpoint_restore_and_refusals(tmp_path):
    md, logs = str(tmp_path / "ck"), []
    args = ["--mode=local", "--device=cpu", "--synthetic", "--batch_size=4", "--model_dir=" + md, "--cell=lnlstm"]
    assert train.run("lstm", args + ["--save_model_secs=0.01", "--num_steps=2"], log=logs.append) == 0
    t = ckpt.load_bundle(ckpt.latest_checkpoint(md))
    assert set(t) == set(NAMES + ["Variable_2"]) and t[PRE + "kernel"].shape == (I + H, 4 * H)
    t["Variable_2"] = torch.tensor(7, dtype=torch.int32)  # re-saved as step 7: a second run must resume from it
    ckpt.Saver(md).save(t, 7)
    logs.clear()
    assert train.run("lstm", args + ["--save_model_secs=0", "--num_steps=8"], log=logs.append) == 0
    assert [int(m.group(1)) for l in logs for m in [re.match(r"Global step (\d+) ", l)] if m] == [8]
    for extra, msg in ((["--rnn_layers=2"], "needs --cell=gru"), (["--bidirectional"], "--bidirectional needs --cell=gru")):
        with pytest.raises(SystemExit, match=msg):
            train.run("lstm", args + extra + ["--num_steps=1"], log=lambda *_: None)
