"""The GRU cell of the row-sequence model off the GPU: the fp32 CPU paths of ops.gru_seq_fwd / gru_seq_bwd and the
float64 autograd recurrence gru_ref64 (also the oracle of tests/test_gru_seq_gpu.py), the model's TF1
variables, and --cell end to end.  Bound of fp32 against float64: a value is a chain of <= 3 steps of dot products of
<= 256 terms of magnitude <= max|ref|, so 4 * 256 * 2^-23 * max|ref|; a wrong term errs by the order of max|ref|."""
import re

import pytest
import torch

from dtfe import ckpt, ops, train
from dtfe.models.lstm import H, I, NC, GruProgram, LstmModel


def gru_ref64(xh, Wg, bg, Wc, bc, dhT=None):
    """float64 autograd GRUCell recurrence over xh [T][B][I+H] (x_t; h_{-1} in step 0's h columns), named like the
    kernels' buffers; given dh_T also dgg / dgc = d sum(h_T dh_T) / d pre-activations.  float64 weights that require
    grad stay in the graph: hT is differentiable, the other buffers are detached."""
    xh, (Wg, bg, Wc, bc) = xh.detach().double(), (v if v.requires_grad else v.detach().double() for v in (Wg, bg, Wc, bc))
    T, Hn = xh.shape[0], Wc.shape[1]
    x, h, hs, zg, rh, zc = xh[:, :, :-Hn], xh[0, :, -Hn:].clone().requires_grad_(), [], [], [], []
    for t in range(T):
        hs.append(h)
        zg.append(torch.cat([x[t], h], 1) @ Wg + bg)
        r, u = torch.sigmoid(zg[t]).split(Hn, 1)
        rh.append(r * h)
        zc.append(torch.cat([x[t], rh[t]], 1) @ Wc + bc)
        h = u * h + (1 - u) * torch.tanh(zc[t])
    cat = lambda cols: torch.cat([x, torch.stack(cols)], 2).detach()  # noqa: E731
    out = dict(xh=cat(hs), xrh=cat(rh), g=torch.sigmoid(torch.stack(zg)).detach(), cand=torch.tanh(torch.stack(zc)).detach(),
               hT=h)
    if dhT is not None:
        grads = torch.autograd.grad((h * dhT.double()).sum(), zg + zc, retain_graph=True)
        out.update(dgg=torch.stack(grads[:T]), dgc=torch.stack(grads[T:]))
    return out


def _close(got, ref, name):
    err, bound = (got.double() - ref).abs().max().item(), 4 * 256 * 2.0 ** -23 * ref.abs().max().item()
    assert err <= bound, "%s: err %.3g > bound %.3g" % (name, err, bound)


@pytest.mark.parametrize("T", [1, 3])
def test_cpu_path_and_oracle_against_float64_autograd(T):
    B, g = 4, torch.Generator().manual_seed(T)
    xh, dhT = torch.randn(T, B, I + H, generator=g), torch.randn(B, H, generator=g)
    Wg, Wc = torch.randn(I + H, 2 * H, generator=g) * 0.2, torch.randn(I + H, H, generator=g) * 0.2
    bg, bc = torch.randn(2 * H, generator=g), torch.randn(H, generator=g)
    p = [v.double().requires_grad_() for v in (Wg, bg, Wc, bc)]
    ref = gru_ref64(xh, *p, dhT)
    want = torch.autograd.grad((ref.pop("hT") * dhT.double()).sum(), p)
    out = dict(xh=xh.clone(), xrh=torch.zeros(T, B, I + H), g=torch.empty(T, B, 2 * H), cand=torch.empty(T, B, H),
               dgg=torch.empty(T, B, 2 * H), dgc=torch.empty(T, B, H))
    hT = torch.empty(B, H)
    assert ops.gru_seq_fwd(out["xh"], out["xrh"], Wg, bg, Wc, bc, out["g"], out["cand"], hT)
    assert ops.gru_seq_bwd(out["xh"], Wg, Wc, out["g"], out["cand"], dhT, out["dgg"], out["dgc"])
    for k in out:
        _close(out[k], ref[k], k)
    f = {k: v.double().reshape(T * B, -1) for k, v in out.items()}  # the variables' gradients from the path's buffers
    grads = (f["xh"].t() @ f["dgg"], f["dgg"].sum(0), f["xrh"].t() @ f["dgc"], f["dgc"].sum(0))
    for name, got, w in zip(("gWg", "gbg", "gWc", "gbc"), grads, want):
        _close(got, w, name)


def test_variables_and_default_cell():
    m = LstmModel(cell="gru")
    names = ["Variable", "Variable_1", "rnn/gru_cell/gates/kernel", "rnn/gru_cell/gates/bias",
             "rnn/gru_cell/candidate/kernel", "rnn/gru_cell/candidate/bias"]
    assert m.var_order == names + ["Variable_2"] and [s.name for s in m.specs] == names
    assert [tuple(s.shape) for s in m.specs] == [(H, NC), (NC,), (I + H, 2 * H), (2 * H,), (I + H, H), (H,)]
    prog = m.program("cpu", 4, seed=0)
    v = [prog.P.view(n) for n in names]
    assert isinstance(prog, GruProgram) and bool((v[3] == 1).all()) and bool((v[5] == 0).all())
    assert all(0.9 < k.abs().max().item() / (6.0 / sum(k.shape)) ** 0.5 <= 1 for k in (v[2], v[4]))  # glorot-uniform
    m = LstmModel()  # without set_cell: today's model
    assert m.var_order == ["Variable", "Variable_1", "rnn/basic_lstm_cell/kernel", "rnn/basic_lstm_cell/bias",
                           "Variable_2"] and not isinstance(m.program("cpu", 4), GruProgram)


def test_cli_checkpoint_restore_and_refusal(tmp_path):
    md, logs = str(tmp_path / "ck"), []
    args = ["--mode=local", "--device=cpu", "--synthetic", "--batch_size=4", "--model_dir=" + md]
    assert train.run("lstm", args + ["--cell=gru", "--save_model_secs=0.01", "--num_steps=2"], log=logs.append) == 0
    t = ckpt.load_bundle(ckpt.latest_checkpoint(md))  # (the checkpoint thread's latest: step 0, 1 or 2)
    assert set(t) == set(LstmModel(cell="gru").var_order) and t["rnn/gru_cell/gates/kernel"].shape == (I + H, 2 * H)
    t["Variable_2"] = torch.tensor(7, dtype=torch.int32)  # re-saved as step 7: a second run must resume from it
    ckpt.Saver(md).save(t, 7)
    logs.clear()
    assert train.run("lstm", args + ["--cell=gru", "--save_model_secs=0", "--num_steps=8"], log=logs.append) == 0
    assert [int(m.group(1)) for l in logs for m in [re.match(r"Global step (\d+) ", l)] if m] == [8]
    with pytest.raises(SystemExit, match="--cell=gru: only the lstm example"):
        train.run("cnn", args + ["--cell=gru", "--num_steps=1"], log=lambda *_: None)
