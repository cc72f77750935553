"""DeviceEvaluator and the --eval_every CLI on the CPU path (the ops' mirrors), flag parsing, the refusals
and two gloo ranks.  The device-parametrised bodies are shared with test_device_eval_gpu.py."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "launch"))

import local_cluster  # noqa: E402

from dtfe import ops, train  # noqa: E402
from dtfe.data import cifar  # noqa: E402
from dtfe.data.mnist import DataSet, DeviceBatcher  # noqa: E402
from dtfe.models.resnet import ResNetModel  # noqa: E402
from dtfe.optim import Optimizer  # noqa: E402
from dtfe.utils import flags as flagmod  # noqa: E402
from dtfe.utils.device_eval import DeviceEvaluator  # noqa: E402

EVAL_KEYS = ("test_accuracy", "test_top5", "test_loss", "test_examples", "eval_ms")


def setup(device, B, n_test, seed=0):
    (tr_x, tr_y), (te_x, te_y) = cifar.synthetic_arrays(n_train=40, n_test=n_test)
    prog = ResNetModel(0.1, "resnet20").program(torch.device(device), B, seed=seed)
    return prog, (tr_x, tr_y), (te_x, te_y)


def norm_of(tr_x, device):
    return cifar.Augment.cifar(tr_x).stats_on(torch.device(device))


def agrees_with_evaluate(device, B, n_test):
    prog, (tr_x, _), (te_x, te_y) = setup(device, B, n_test)
    lab = torch.from_numpy(te_y).view(-1, 1).to(device)
    for norm in (None, norm_of(tr_x, device)):
        prog.input_norm = norm
        images = torch.from_numpy(te_x).to(device) if norm is not None else \
            torch.from_numpy(te_x.astype(np.float32) / 255.0).to(device)
        acc = prog.evaluate(images, lab)
        assert prog.evaluate(images, lab) == acc  # evaluate() itself is reproducible
        ev = DeviceEvaluator(prog, te_x, te_y, topk=5)
        res = ev.run()
        assert res["examples"] == n_test and ev.capture_error is None
        assert res["accuracy"] * n_test == round(acc * n_test)
        assert 0 <= res["accuracy"] <= res["topk_accuracy"] <= 1 and math.isfinite(res["loss"])
        # the first rows only
        part = DeviceEvaluator(prog, te_x, te_y, topk=5, examples=B + 1).run()
        assert part["examples"] == B + 1
        assert part["accuracy"] * (B + 1) == round(prog.evaluate(images[:B + 1], lab[:B + 1]) * (B + 1))


def graph_and_eager_agree(device, B, n_test):
    prog, _, (te_x, te_y) = setup(device, B, n_test)
    states = []
    for graph in (True, False):
        ev = DeviceEvaluator(prog, te_x, te_y, topk=5, graph=graph)
        first = ev.run()
        states.append(ev.state.cpu().clone())
        again = ev.run()  # (graph=True: the first pass ran eager, capturing and replayed chunks; this one replays)
        assert torch.equal(ev.state.cpu(), states[-1]) and again == first
        assert ev.capture_error is None
        if graph and torch.device(device).type == "cuda":
            assert ev.graph is not None
    assert torch.equal(states[0], states[1])  # int64 words: the loss bits too


def nothing_else_moves(device, B, n_test):
    prog, (tr_x, tr_y), (te_x, te_y) = setup(device, B, n_test)
    model = prog.model
    gstep = torch.zeros(1, dtype=torch.int32, device=device)
    cfg, var_list, bp = model.opt_groups[0]
    opt = Optimizer(cfg, prog.P, var_list=var_list, global_step=gstep, beta_power_names=bp)
    batcher = DeviceBatcher(DataSet(tr_x, tr_y, True, 1), device, B, sampling="device")
    for _ in range(2):  # two training steps: moving averages and momentum slots hold something
        prog.load_batch(batcher.next_batch())
        prog.compute_grads()
        Optimizer.step_all([opt], [1], grad16=None, gscale=1.0)
    before = [t.clone() for t in (prog.P.master, opt.s1, gstep, batcher.aug_ctr, batcher.aug_done)]
    bns = prog.batchnorms()
    ev = DeviceEvaluator(prog, te_x, te_y, topk=5)
    ev.run()
    after = (prog.P.master, opt.s1, gstep, batcher.aug_ctr, batcher.aug_done)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert float(prog.loss.item()) == 0.0 and int(prog.correct.item()) == 0
    assert prog.training is True and not any(bn.infer for bn in bns)


def flags_restored_when_forward_raises(device, B, n_test, monkeypatch):
    prog, _, (te_x, te_y) = setup(device, B, n_test)
    ev = DeviceEvaluator(prog, te_x, te_y, topk=5, graph=False)

    def boom():
        assert prog.training is False and all(bn.infer for bn in prog.batchnorms())
        raise RuntimeError("forward failed")

    monkeypatch.setattr(prog, "forward_logits", boom)
    with pytest.raises(RuntimeError, match="forward failed"):
        ev.run()
    assert prog.training is True and not any(bn.infer for bn in prog.batchnorms())
    assert float(prog.loss.item()) == 0.0 and int(prog.correct.item()) == 0


def construction_errors(device, B, n_test):
    prog, _, (te_x, te_y) = setup(device, B, n_test)
    with pytest.raises(ValueError, match="eval_topk"):
        DeviceEvaluator(prog, te_x, te_y, topk=11)
    with pytest.raises(ValueError, match="eval_topk"):
        DeviceEvaluator(prog, te_x, te_y, topk=0)
    bad = te_y.copy()
    bad[n_test - 1] = 10
    with pytest.raises(ValueError, match="labels lie outside"):
        DeviceEvaluator(prog, te_x, bad, topk=5).run()

    class NoProtocol:
        model = prog.model
    with pytest.raises(ValueError, match="forward_logits"):
        DeviceEvaluator(NoProtocol(), te_x, te_y)


def cli_rows(device, B, n_eval, tmp_path, extra=(), name="m"):
    mj = tmp_path / (name + ".jsonl")
    logs = []
    fl = flagmod.parse(["--device=" + device, "--synthetic", "--batch_size", str(B), "--num_steps", "5", "--eval_every",
                        "2", "--eval_examples", str(n_eval), "--save_model_secs=0", "--model_dir=" + str(tmp_path / name),
                        "--metrics_jsonl=" + str(mj)] + list(extra),
                       model_defaults=dict(batch_size=128, num_steps=1000, learning_rate=0.1))
    dev = torch.device("cuda:0" if device == "cuda" else "cpu")
    prog, _opts, gstep = train.run_allreduce(fl, ResNetModel(0.1, "resnet20"), dev, logs.append)
    assert int(gstep.item()) == 5
    return [json.loads(line) for line in mj.read_text().splitlines()], logs, prog


def check_eval_rows(rows, evaluated_gs, n_eval):
    for r in rows:
        if r["gs"] in evaluated_gs:
            assert all(k in r for k in EVAL_KEYS), r
            assert r["test_examples"] == n_eval
            assert 0 <= r["test_accuracy"] <= r["test_top5"] <= 1 and math.isfinite(r["test_loss"])
            assert r["eval_ms"] > 0
        else:
            assert not any(k.startswith("test_") or k == "eval_ms" for k in r), r


def cli_local_mode(device, B, n_eval, tmp_path):
    rows, logs, prog = cli_rows(device, B, n_eval, tmp_path)
    assert [r["gs"] for r in rows] == [1, 2, 3, 4, 5]
    check_eval_rows(rows, (2, 4, 5), n_eval)
    lines = [l for l in logs if "Test-Accuracy" in l]
    assert [l.split(" Test-Accuracy")[0] for l in lines] == ["Global step 2", "Global step 4", "Global step 5"]
    assert all("Test-Loss: " in l for l in lines)
    assert prog.evaluator.capture_error is None
    # several steps per replay: the replays ending at gs 2 and 4 evaluate, and the end of training does
    rows, logs, prog = cli_rows(device, B, n_eval, tmp_path, ["--shuffle", "device", "--steps_per_graph", "2"], "s")
    assert [r["gs"] for r in rows] == [2, 4, 5]
    check_eval_rows(rows, (2, 4, 5), n_eval)
    assert len([l for l in logs if "Test-Accuracy" in l]) == 3
    assert prog.evaluator.capture_error is None and prog.step_runner.capture_error is None
    # an --eval_every that no step reaches: the end of training still evaluates, once
    rows, logs, _ = cli_rows(device, B, n_eval, tmp_path, ["--eval_every", "100"], "e")
    check_eval_rows(rows, (5,), n_eval)
    assert len([l for l in logs if "Test-Accuracy" in l]) == 1


# ----------------------------------------------------------------------------------------- the CPU runs
CPU = ("cpu", 4, 10)


def test_evaluator_agrees_with_evaluate_cpu():
    agrees_with_evaluate(*CPU)


def test_evaluator_runs_repeat_cpu():
    graph_and_eager_agree(*CPU)


def test_evaluator_moves_nothing_else_cpu():
    nothing_else_moves(*CPU)


def test_evaluator_restores_flags_when_forward_raises_cpu(monkeypatch):
    flags_restored_when_forward_raises(*CPU, monkeypatch)


def test_evaluator_construction_errors_cpu():
    construction_errors(*CPU)


def test_cli_eval_every_cpu(tmp_path):
    cli_local_mode(*CPU, tmp_path)


def test_eval_flags_parse():
    d = dict(batch_size=8, num_steps=1, learning_rate=0.1)
    fl = flagmod.parse([], model_defaults=d)
    assert (fl.eval_every, fl.eval_examples, fl.eval_topk) == (0, 0, 5)
    fl = flagmod.parse(["--eval_every=7", "--eval_examples", "30", "--eval_topk=3"], model_defaults=d)
    assert (fl.eval_every, fl.eval_examples, fl.eval_topk) == (7, 30, 3)
    for bad in (["--eval_every=-1"], ["--eval_examples=-2"], ["--eval_topk=0"]):
        with pytest.raises(SystemExit):
            flagmod.parse(bad, model_defaults=d)


BASE = ["--device=cpu", "--synthetic", "--batch_size=4", "--num_steps=1", "--save_model_secs=0"]


def test_eval_every_refused_in_ps_mode(tmp_path):
    with pytest.raises(ValueError, match="--eval_every"):
        train.run("resnet20", BASE + ["--mode=ps", "--ps_hosts=127.0.0.1:1", "--worker_hosts=127.0.0.1:2",
                                      "--job_name=worker", "--eval_every=2", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)


@pytest.mark.parametrize("model", ["gan", "encoder", "softmax", "lstm", "cnn"])
def test_eval_every_refused_without_the_protocol(model, tmp_path):
    with pytest.raises(ValueError, match="--eval_every"):
        train.run(model, BASE + ["--eval_every=2", "--model_dir=" + str(tmp_path)], log=lambda *_: None)


def test_eval_topk_above_the_classes_refused(tmp_path):
    with pytest.raises(ValueError, match="eval_topk"):
        train.run("resnet20", BASE + ["--eval_every=1", "--eval_topk=11", "--eval_examples=4",
                                      "--model_dir=" + str(tmp_path)], log=lambda *_: None)


@pytest.mark.slow
def test_two_gloo_ranks_print_the_same_test_lines(tmp_path):
    codes, out, _ = local_cluster.launch("resnet20", 0, 2, ["--mode=allreduce", "--device=cpu", "--batch_size=4",
                                                             "--num_steps=3", "--data_dir=/nonexistent",
                                                             "--eval_every=2", "--eval_examples=10",
                                                             "--model_dir=" + str(tmp_path / "ck")],
                                         timeout=300, stream=False)
    assert all(c == 0 for c in codes.values()), out
    lines = [[l for l in out[("worker", w)] if "Test-Accuracy" in l] for w in (0, 1)]
    assert len(lines[0]) == 2 and lines[0] == lines[1], lines
    assert lines[0][0].startswith("Global step 2 ") and lines[0][1].startswith("Global step 3 ")
