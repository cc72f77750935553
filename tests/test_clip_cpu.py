"""Global-norm gradient clipping without a GPU: the optimizers' CPU path against hand-written float64
tf.clip_by_global_norm + update, the --clip_norm flag, and the local / ps-worker wiring end to end."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.models.lstm import LstmModel
from dtfe.optim import FlatParams, GlobalNormClip, Optimizer, OptimizerConfig, VarSpec
from dtfe.utils import flags as flagmod

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "launch"))
import local_cluster  # noqa: E402


def _init(shape, g):
    return torch.randn(*shape, generator=g)


SPECS = [VarSpec("a", (7,), _init), VarSpec("skip", (50,), _init), VarSpec("b", (33, 5), _init),
         VarSpec("c", (8192 + 9,), _init)]
VAR_LIST = ["a", "b", "c"]


def _gather(P, t, names=VAR_LIST):
    return torch.cat([t[P.offsets[n]:P.offsets[n] + P.spec(n).numel] for n in names])


def _ref_update(kind, cfg, p, g, s1, s2, b1p, b2p):
    """One TF1 update in float64 (tensorflow/python/training/*.py @ 1.11); returns p, s1, s2."""
    if kind == "sgd":
        return p - cfg.lr * g, s1, s2
    if kind == "momentum":
        s1 = cfg.momentum * s1 + g
        return p - cfg.lr * s1, s1, s2
    if kind == "adam":
        lr_t = cfg.lr * math.sqrt(1 - b2p) / (1 - b1p)
        s1 = cfg.beta1 * s1 + (1 - cfg.beta1) * g
        s2 = cfg.beta2 * s2 + (1 - cfg.beta2) * g * g
        return p - lr_t * s1 / (np.sqrt(s2) + cfg.resolved_eps()), s1, s2
    s1 = cfg.rho * s1 + (1 - cfg.rho) * g * g
    s2 = cfg.momentum * s2 + cfg.lr * g / np.sqrt(s1 + cfg.resolved_eps())
    return p - s2, s1, s2


@pytest.mark.parametrize("clip_norm", [3.0, 1e6])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam", "rmsprop"])
def test_step_cpu_matches_float64_clip_by_global_norm(kind, clip_norm):
    cfg = OptimizerConfig(kind=kind, lr=0.05, momentum=0.9 if kind in ("momentum", "rmsprop") else 0.0,
                          clip_norm=clip_norm)
    P = FlatParams(SPECS, "cpu", seed=5)
    opt = Optimizer(cfg, P, var_list=VAR_LIST)
    init = P.master.clone()
    p = _gather(P, P.master).double().numpy()
    s1 = np.ones_like(p) if kind == "rmsprop" else np.zeros_like(p)
    s2 = np.zeros_like(p)
    b1p, b2p = cfg.beta1, cfg.beta2
    gscale = 0.5
    for step in range(2):
        gen = torch.Generator().manual_seed(100 + step)
        grad = torch.full((P.total,), float("nan"))
        for n in VAR_LIST:
            o, k = P.offsets[n], P.spec(n).numel
            grad[o:o + k] = torch.randn(k, generator=gen)
        opt.step(grad=grad, gscale=gscale)
        # tf.clip_by_global_norm: t * clip_norm / max(global_norm, clip_norm)
        g = _gather(P, grad).double().numpy() * gscale
        norm = math.sqrt(float((g * g).sum()))
        g = g * (clip_norm / max(norm, clip_norm))
        p, s1, s2 = _ref_update(kind, cfg, p, g, s1, s2, b1p, b2p)
        b1p, b2p = b1p * cfg.beta1, b2p * cfg.beta2
        assert abs(float(opt.global_norm.item()) - norm) <= 1e-6 * norm
        assert (float(opt.clip_out[1].item()) < 1.0) == (norm > clip_norm)
        # fp32 arithmetic against float64: a handful of roundings of 2^-24 per element
        np.testing.assert_allclose(_gather(P, P.master).numpy(), p, rtol=2e-5, atol=2e-6)
    o, k = P.offsets["skip"], P.spec("skip").numel
    assert torch.equal(P.master[o:o + k], init[o:o + k])  # outside the var list (its gradient is NaN)


def test_clip_norm_zero_builds_no_plan_and_changes_nothing():
    Pa, Pb = FlatParams(SPECS, "cpu", seed=5), FlatParams(SPECS, "cpu", seed=5)
    a = Optimizer(OptimizerConfig(kind="adam", clip_norm=0.0), Pa, var_list=VAR_LIST)
    b = Optimizer(OptimizerConfig(kind="adam"), Pb, var_list=VAR_LIST)
    assert a.clip is None and a.global_norm is None
    g = torch.randn(Pa.total, generator=torch.Generator().manual_seed(1))
    a.step(grad=g)
    b.step(grad=g)
    assert torch.equal(Pa.master, Pb.master)
    with pytest.raises(ValueError):
        Optimizer(OptimizerConfig(kind="sgd", clip_norm=-1.0), Pa)


def test_ops_cpu_paths():
    P = FlatParams(SPECS, "cpu", seed=5)
    plan = ops.grad_norm_plan([(P.offsets[n], P.spec(n).numel) for n in VAR_LIST], P.master)
    assert plan.dtype == torch.int64 and plan.shape[1] == 2 and int(plan[:, 1].max()) <= 8192
    assert int(plan[:, 1].sum()) == sum(P.spec(n).numel for n in VAR_LIST)
    g = torch.full((P.total,), float("nan"))
    for o, n in plan.tolist():
        g[o:o + n] = 2.0
    out = torch.zeros(2)
    ops.grad_sumsq(g, None, 0.5, 1.0, plan, torch.zeros(len(plan)), torch.zeros(1, dtype=torch.int32), out)
    n = int(plan[:, 1].sum())
    assert abs(float(out[0]) - math.sqrt(n)) < 1e-4 and abs(float(out[1]) - 1 / math.sqrt(n)) < 1e-7
    ops.grad_sumsq(None, g.bfloat16(), 0.5, 1.0, plan, torch.zeros(len(plan)), torch.zeros(1, dtype=torch.int32), out)
    assert abs(float(out[0]) - math.sqrt(n)) < 1e-4
    ops.scale_(g, out[1:], plan)
    clip = GlobalNormClip(P, VAR_LIST, 1.0)
    clip.compute(g)
    assert abs(float(clip.norm.item()) - 2.0) < 1e-5  # 2 * sqrt(n) / sqrt(n)
    with pytest.raises(ValueError):
        ops.grad_norm_plan([(P.total - 1, 2)], P.master)


# ------------------------------------------------------------------ flags
def test_negative_clip_norm_is_an_argument_error(capsys):
    with pytest.raises(SystemExit) as e:
        flagmod.parse(["--clip_norm=-1"])
    assert e.value.code == 2 and "--clip_norm" in capsys.readouterr().err
    assert flagmod.parse([]).clip_norm == 0.0 and flagmod.parse(["--clip_norm", "2.5"]).clip_norm == 2.5


def test_cnn_own_schedule_refuses_clip_norm(tmp_path):
    with pytest.raises(ValueError, match="--bucket_mb"):
        train.run("cnn", ["--mode=local", "--device=cpu", "--synthetic", "--clip_norm=1.0", "--num_steps=1",
                          "--batch_size=4", "--save_model_secs=0", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)


def test_cnn_with_bucket_mb_takes_the_generic_path_and_clips(tmp_path):
    mj = tmp_path / "m.jsonl"
    rc = train.run("cnn", ["--mode=local", "--device=cpu", "--synthetic", "--bucket_mb=4", "--clip_norm=0.5",
                           "--num_steps=2", "--batch_size=4", "--save_model_secs=0", "--metrics_jsonl=" + str(mj),
                           "--model_dir=" + str(tmp_path)], log=lambda *_: None)
    rows = [json.loads(l) for l in mj.read_text().splitlines()]
    assert rc == 0 and [r["gs"] for r in rows] == [1, 2]
    assert all(math.isfinite(r["global_norm"]) and r["global_norm"] > 0.5 for r in rows), rows


# ------------------------------------------------------------------ local
def _lstm_params_after(tmp_path, steps, clip):
    argv = ["--mode=local", "--device=cpu", "--synthetic", "--seed=3", "--batch_size=16", "--num_steps=%d" % steps,
            "--learning_rate=0.1",
            "--save_model_secs=0", "--model_dir=" + str(tmp_path / ("ck%d" % steps)), "--clip_norm=%r" % clip]
    m0 = LstmModel()
    fl = flagmod.parse(argv, model_defaults=dict(batch_size=m0.default_batch, num_steps=m0.default_steps,
                                                 learning_rate=train.MODELS["lstm"][1]))
    flagmod.resolve_mode(fl)
    torch.manual_seed(fl.seed)
    np.random.seed(fl.seed)
    prog, opts, gstep = train.run_allreduce(fl, LstmModel(lr=fl.learning_rate), torch.device("cpu"), lambda *_: None)
    assert int(gstep.item()) == steps and opts[0].clip is not None
    return prog.P.master.clone(), fl.learning_rate


def test_lstm_local_run_logs_global_norm_and_bounds_every_update(tmp_path):
    # lr * C = 0.1: far above the fp32 resolution of the parameters themselves, so the rounding of
    # p' = fl(p - lr g) (about 3e-7 in norm over the LSTM's 0.2 M parameters) does not show in |p' - p|
    clip = 1.0
    mj = tmp_path / "m.jsonl"
    rc = train.run("lstm", ["--mode=local", "--device=cpu", "--synthetic", "--seed=3", "--batch_size=16",
                            "--learning_rate=0.1",
                            "--clip_norm=%r" % clip, "--num_steps=3", "--save_model_secs=0",
                            "--metrics_jsonl=" + str(mj), "--model_dir=" + str(tmp_path / "ck")], log=lambda *_: None)
    assert rc == 0
    rows = [json.loads(l) for l in mj.read_text().splitlines()]
    assert len(rows) == 3
    assert all(r["global_norm"] > clip and math.isfinite(r["global_norm"]) for r in rows), rows  # every step clips
    # the LSTM trains with plain SGD: p' = p - lr * g * scale, so |p' - p| <= lr * C
    ps = [_lstm_params_after(tmp_path, k, clip) for k in (0, 1, 2, 3)]
    lr = ps[0][1]
    for k in range(3):
        d = float((ps[k + 1][0].double() - ps[k][0].double()).norm())
        print("step", k, "|dp|", d, "lr*C", lr * clip)
        assert 0 < d <= lr * clip * (1 + 1e-5), (k, d, lr * clip)


# --------------------------------------------------------------------- ps
def _ps_softmax_first_update_norm(tmp_path, extra):
    tmp_path.mkdir()
    codes, out, _ = local_cluster.launch(
        "softmax", 1, 1, ["--data_dir=/nonexistent", "--device=cpu", "--seed=1", "--workers=1", "--num_steps=1",
                          "--ps_transport=pg", "--save_model_secs=0", "--check_pull",
                          "--model_dir=" + str(tmp_path)] + extra, timeout=240, stream=False)
    assert all(c == 0 for c in codes.values()), (codes, out)
    norms = [float(m.group(1)) for l in out[("worker", 0)] for m in [re.match(r"pull l2norm gs=1: (\S+)$", l)] if m]
    assert len(norms) == 1, out[("worker", 0)]
    return norms[0]  # the variables start at zero: the norm of the first update


@pytest.mark.slow
def test_ps_worker_clips_before_it_pushes(tmp_path):
    lr, clip = 0.01, 1e-3  # (softmax: GradientDescent(0.01); the first gradient's norm is far above 1e-3)
    bound = lr * clip * (1 + 1e-5)
    d = _ps_softmax_first_update_norm(tmp_path / "clip", ["--clip_norm=%r" % clip])
    assert 0 < d <= bound, (d, bound)
    d0 = _ps_softmax_first_update_norm(tmp_path / "noclip", [])
    assert d0 > bound, (d0, bound)  # without the flag the same check fails: the test can see the clip
