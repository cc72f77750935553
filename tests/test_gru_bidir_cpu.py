"""The bidirectional GRU layer of the row-sequence model off the GPU: the model's TF1 variables, the CPU step program
against float64 autograd of the model (bidir_loss64, also the oracle of tests/test_gru_bidir_gpu.py) within the bound
of tests/test_gru_cpu.py, and --bidirectional end to end."""
import re

import pytest
import torch
from test_gru_cpu import _close, gru_ref64

from dtfe import ckpt, train
from dtfe.models.lstm import H, I, NC, T, GruBidirProgram, GruProgram, LstmModel

CELL = ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")
NAMES = ["Variable", "Variable_1"] + ["bidirectional_rnn/%s/gru_cell/%s" % (d, n) for d in ("fw", "bw") for n in CELL]


def bidir_loss64(x, y, w):
    """float64 model: GRU forward in time and GRU over the time-reversed rows, both from h = 0, the two final states
    through the head, mean softmax cross-entropy.  x [B][T * I], y one-hot, w the ten variables in creation order."""
    xh = torch.zeros(T, x.shape[0], I + H)
    xh[:, :, :I] = x.reshape(-1, T, I).transpose(0, 1)
    feat = torch.cat([gru_ref64(xh, *w[2:6])["hT"], gru_ref64(xh.flip(0), *w[6:10])["hT"]], 1)
    return -(torch.log_softmax(feat @ w[0] + w[1], 1) * y.double()).sum(1).mean()


def test_variables_and_unchanged_defaults():
    m = LstmModel(cell="gru", bidirectional=True)
    assert m.var_order == NAMES + ["Variable_2"] and [s.name for s in m.specs] == NAMES
    cell = [(I + H, 2 * H), (2 * H,), (I + H, H), (H,)]
    assert [tuple(s.shape) for s in m.specs] == [(2 * H, NC), (NC,)] + cell + cell
    prog = m.program("cpu", 4, seed=0)
    v = [prog.P.view(n) for n in NAMES]
    assert isinstance(prog, GruBidirProgram) and not torch.equal(v[2], v[6])
    for k in (2, 6):  # per cell: glorot-uniform kernels, gates bias ones, candidate bias zeros
        assert bool((v[k + 1] == 1).all()) and bool((v[k + 3] == 0).all())
        assert all(0.9 < w.abs().max().item() / (6.0 / sum(w.shape)) ** 0.5 <= 1 for w in (v[k], v[k + 2]))
    m.set_cell("gru")  # the defaults: today's single cell
    assert m.var_order[2] == "rnn/gru_cell/gates/kernel" and type(m.program("cpu", 4)) is GruProgram
    assert tuple(m.specs[0].shape) == (H, NC) and LstmModel().var_order[2] == "rnn/basic_lstm_cell/kernel"


def test_cpu_program_gradients_against_float64_autograd():
    B, g = 4, torch.Generator().manual_seed(11)
    x, y = torch.rand(B, T * I, generator=g), torch.eye(NC)[torch.randint(0, NC, (B,), generator=g)]
    prog = LstmModel(cell="gru", bidirectional=True).program("cpu", B, seed=2)
    w = [prog.P.view(n).double().clone().requires_grad_() for n in NAMES]
    prog.load_batch((x, y))
    loss = float(prog.compute_grads()["loss"])
    l64 = bidir_loss64(x, y, w)
    _close(torch.tensor(loss), l64.detach(), "loss")
    for n, gr in zip(NAMES, torch.autograd.grad(l64, w)):
        _close(prog.P.gview(n), gr, n)


def test_cli_checkpoint_restore_and_refusals(tmp_path):
    md, logs, quiet = str(tmp_path / "ck"), [], lambda *_: None
    args = ["--mode=local", "--device=cpu", "--synthetic", "--batch_size=4", "--model_dir=" + md]
    bi = args + ["--cell=gru", "--bidirectional"]
    assert train.run("lstm", bi + ["--save_model_secs=0.01", "--num_steps=2"], log=logs.append) == 0
    t = ckpt.load_bundle(ckpt.latest_checkpoint(md))
    assert set(t) == set(NAMES + ["Variable_2"]) and t["Variable"].shape == (2 * H, NC)
    assert t["bidirectional_rnn/bw/gru_cell/gates/kernel"].shape == (I + H, 2 * H)
    t["Variable_2"] = torch.tensor(7, dtype=torch.int32)  # re-saved as step 7: a second run must resume from it
    ckpt.Saver(md).save(t, 7)
    logs.clear()
    assert train.run("lstm", bi + ["--save_model_secs=0", "--num_steps=8"], log=logs.append) == 0
    assert [int(m.group(1)) for l in logs for m in [re.match(r"Global step (\d+) ", l)] if m] == [8]
    for model, extra, msg in (("lstm", ["--bidirectional"], "--bidirectional needs --cell=gru"),
                              ("lstm", ["--cell=gru", "--bidirectional", "--rnn_layers=2"],
                               "--bidirectional with --rnn_layers=2: a stacked bidirectional GRU is not implemented"),
                              ("cnn", ["--bidirectional"], "--bidirectional: only the lstm example")):
        with pytest.raises(SystemExit, match=msg):
            train.run(model, args + extra + ["--num_steps=1"], log=quiet)
