"""Stacked GRU cells (--cell gru --rnn_layers L) off the GPU: the TF1 MultiRNNCell variables, the CPU step program
against float64 autograd of stack_ref64 (also the oracle of tests/test_gru_stack_gpu.py), and the flag end to end.
Bound of the fp32 program against float64: a gradient is reached through at most 2 T L cell steps (forward, then
backward), each a dot product of <= 256 terms of magnitude <= max|ref|: 2 T L * 256 * 2^-23 * max|ref|."""
import re

import pytest
import torch

from dtfe import ckpt, train
from dtfe.models.lstm import H, I, NC, T, GruStackProgram, LstmModel


def stack_ref64(x, y, w):
    """float64 loss of the model: x [T][B][I] through the stacked GRUCells w[2:] = (Wg, bg, Wc, bc) per layer from
    h = 0, then the mean softmax cross-entropy of h_T . w[0] + w[1] against one-hot y"""
    seq = x.double()
    for Wg, bg, Wc, bc in zip(*(w[2 + k::4] for k in range(4))):
        h, out = torch.zeros(seq.shape[1], H, dtype=torch.float64), []
        for x_t in seq:
            r, u = torch.sigmoid(torch.cat([x_t, h], 1) @ Wg + bg).split(H, 1)
            h = u * h + (1 - u) * torch.tanh(torch.cat([x_t, r * h], 1) @ Wc + bc)
            out.append(h)
        seq = torch.stack(out)
    return -(torch.log_softmax(seq[-1] @ w[0] + w[1], 1) * y.double()).sum(1).mean()


def test_variables_of_two_layers():
    m = LstmModel(cell="gru", layers=2)
    cells = ["rnn/multi_rnn_cell/cell_%d/gru_cell/%s" % (l, n) for l in range(2)
             for n in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")]
    assert m.var_order == ["Variable", "Variable_1"] + cells + ["Variable_2"] and [s.name for s in m.specs] == m.var_order[:-1]
    assert [tuple(s.shape) for s in m.specs[2:]] == [(I + H, 2 * H), (2 * H,), (I + H, H), (H,),
                                                     (2 * H, 2 * H), (2 * H,), (2 * H, H), (H,)]
    prog = m.program("cpu", 4, seed=0)
    v = [prog.P.view(n) for n in cells]
    assert isinstance(prog, GruStackProgram) and all(bool((v[k] == 1).all()) and bool((v[k + 2] == 0).all()) for k in (1, 5))
    assert all(0.9 < v[k].abs().max().item() / (6.0 / sum(v[k].shape)) ** 0.5 <= 1 for k in (0, 2, 4, 6))  # glorot-uniform


@pytest.mark.parametrize("L", [2, 3])
def test_cpu_program_gradients_against_float64_autograd(L):
    B, g = 4, torch.Generator().manual_seed(L)
    model = LstmModel(cell="gru", layers=L)
    x, y = torch.rand(B, T * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    prog, names = model.program("cpu", B, seed=1), model.var_order[:-1]
    prog.load_batch((x, y))
    loss = torch.tensor(float(prog.compute_grads()["loss"]), dtype=torch.float64)
    w = [prog.P.view(n).double().clone().requires_grad_() for n in names]
    l64 = stack_ref64(x.reshape(B, T, I).transpose(0, 1), y, w)
    got = [prog.P.gview(n).double() for n in names] + [loss]
    for n, a, ref in zip(names + ["loss"], got, torch.autograd.grad(l64, w) + (l64.detach(),)):
        err, bound = (a - ref).abs().max().item(), 2 * T * L * 256 * 2.0 ** -23 * ref.abs().max().item()
        assert err <= bound, "%s: err %.3g > bound %.3g" % (n, err, bound)


def test_cli_checkpoint_restore_and_refusals(tmp_path):
    md, logs = str(tmp_path / "ck"), []
    args = ["--mode=local", "--device=cpu", "--synthetic", "--batch_size=4", "--model_dir=" + md]
    gru2 = args + ["--cell=gru", "--rnn_layers=2"]
    assert train.run("lstm", gru2 + ["--save_model_secs=0.01", "--num_steps=2"], log=logs.append) == 0
    t = ckpt.load_bundle(ckpt.latest_checkpoint(md))
    assert set(t) == set(LstmModel(cell="gru", layers=2).var_order)
    assert t["rnn/multi_rnn_cell/cell_1/gru_cell/gates/kernel"].shape == (2 * H, 2 * H)
    t["Variable_2"] = torch.tensor(7, dtype=torch.int32)  # re-saved as step 7: a second run must resume from it
    ckpt.Saver(md).save(t, 7)
    logs.clear()
    assert train.run("lstm", gru2 + ["--save_model_secs=0", "--num_steps=8"], log=logs.append) == 0
    assert [int(m.group(1)) for l in logs for m in [re.match(r"Global step (\d+) ", l)] if m] == [8]
    for name, msg in (("lstm", "--rnn_layers=2 needs --cell=gru"), ("cnn", "--rnn_layers=2: only the lstm example")):
        with pytest.raises(SystemExit, match=msg):
            train.run(name, args + ["--rnn_layers=2", "--num_steps=1"], log=lambda *_: None)
