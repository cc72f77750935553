"""Learning-rate schedules, L2 weight decay and Nesterov momentum without a GPU: the float32 host mirror
against a float64 evaluation of the TF definitions, the validation errors, the CPU path of the optimizer
against a float64 closed form, the flags' refusals and a CPU command-line run."""
import json

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig, VarSpec
from dtfe.utils import flags as flagmod


# ------------------------------------------------- the TF definitions, float64
def _piecewise64(step, bounds, values):
    """tf.train.piecewise_constant: values[0] for step <= b[0], values[i] for b[i-1] < step <= b[i]."""
    for b, v in zip(bounds, values):
        if step <= b:
            return float(v)
    return float(values[-1])


def _linear64(step, lr, end, n):
    """tf.train.polynomial_decay, power 1, cycle=False."""
    return (lr - end) * (1.0 - min(step, n) / n) + end


def _warm64(v, step, w):
    return v * (step + 1) / w if step < w else v


B, VALS, W, N = (6, 11), (0.1, 0.01, 0.001), 4, 9
STEPS = sorted({0, B[0] - 1, B[0], B[0] + 1, B[1] - 1, B[1], B[1] + 1, W - 1, W, N, N + 1, 10 ** 6})


def test_piecewise_mirror_matches_the_tf_definition():
    spec = ops.lr_schedule_spec(0.1, B, VALS, warmup_steps=W)
    for s in STEPS:
        got, want = ops.lr_schedule_value(spec, s), _warm64(_piecewise64(s, B, VALS), s, W)
        assert isinstance(got, np.float32)
        assert abs(float(got) - want) <= 2 * np.spacing(np.float32(want)), (s, got, want)
    # the <= of tf.train.piecewise_constant: the boundary step itself still has the earlier value
    assert ops.lr_schedule_value(spec, B[0]) == np.float32(0.1)
    assert ops.lr_schedule_value(spec, B[0] + 1) == np.float32(0.01)
    assert ops.lr_schedule_value(spec, B[1] + 1) == np.float32(0.001)
    assert ops.lr_schedule_value(spec, W - 1) == np.float32(0.1)  # (W - 1 + 1) / W = 1


def test_linear_mirror_matches_the_tf_definition():
    for w in (0, W):
        spec = ops.lr_schedule_spec(0.1, decay_steps=N, end=0.002, warmup_steps=w)
        for s in STEPS:
            got, want = ops.lr_schedule_value(spec, s), _warm64(_linear64(s, 0.1, 0.002, N), s, w)
            # in units of ulp(lr): the float32 1 / N and t * (1 / N) are each off by up to 2^-24 relative,
            # about 2 ulp(lr) once multiplied by lr - end; four more roundings of values <= lr (lr - end,
            # the product, the sum, the warm-up) add half an ulp each, the inputs' own rounding one more
            assert abs(float(got) - want) <= 6 * np.spacing(np.float32(0.1)), (s, got, want)
    assert ops.lr_schedule_value(spec, N) == ops.lr_schedule_value(spec, N + 1) == ops.lr_schedule_value(spec, 10 ** 6)
    assert abs(float(ops.lr_schedule_value(spec, N)) - 0.002) <= 6 * np.spacing(np.float32(0.1))


def test_constant_rate_with_warmup_only():
    spec = ops.lr_schedule_spec(0.5, warmup_steps=2)
    assert [float(ops.lr_schedule_value(spec, s)) for s in range(4)] == [0.25, 0.5, 0.5, 0.5]


# --------------------------------------------------------------- validation
def _specs():
    init = lambda shape, g: torch.randn(*shape, generator=g)
    return [VarSpec("w/kernel", (5, 3), init), VarSpec("w/bias", (5,), init), VarSpec("v/kernel", (70,), init)]


def _opt(kind="momentum", gs=True, var_list=None, **kw):
    P = FlatParams(_specs(), "cpu", seed=1)
    g = torch.zeros(1, dtype=torch.int32) if gs else None
    kw.setdefault("lr", 0.1)
    cfg = OptimizerConfig(kind=kind, momentum=0.9 if kind in ("momentum", "rmsprop") else 0.0, **kw)
    return Optimizer(cfg, P, var_list=var_list, global_step=g), P, g


@pytest.mark.parametrize("kw,match", [
    (dict(lr_boundaries=(1, 2), lr_values=(0.1, 0.01)), "values"),
    (dict(lr_boundaries=(1,), lr_values=(0.1, 0.01, 0.001)), "values"),
    (dict(lr_values=(0.1,)), "boundaries"),
    (dict(lr_boundaries=(2, 2), lr_values=(0.1, 0.01, 0.001)), "increasing"),
    (dict(lr_boundaries=(3, 2), lr_values=(0.1, 0.01, 0.001)), "increasing"),
    (dict(lr_boundaries=tuple(range(1, 10)), lr_values=(0.1,) * 10), "boundaries"),
    (dict(lr_boundaries=(1,), lr_values=(0.1, 0.01), lr_decay_steps=5), "mutually exclusive"),
    (dict(lr_decay_steps=-3), "decay_steps"),
    (dict(lr_warmup_steps=-1), "warmup_steps"),
    (dict(weight_decay=-1e-4), "weight_decay"),
    (dict(weight_decay=1e-4, decay_vars=("nope/kernel",)), "decay_vars"),
])
def test_validation_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        _opt(**kw)


def test_a_schedule_needs_a_global_step_and_nesterov_momentum():
    with pytest.raises(ValueError, match="global_step"):
        _opt(gs=False, lr_warmup_steps=3)
    for kind in ("sgd", "adam", "rmsprop"):
        with pytest.raises(ValueError, match="nesterov"):
            _opt(kind=kind, nesterov=True)
    o, _, _ = _opt(lr_boundaries=tuple(range(1, 9)), lr_values=(0.1,) * 9, nesterov=True)  # 8 boundaries are fine
    assert o.lr_spec["kind"] == ops.LR_PIECEWISE and o.nesterov
    o, _, _ = _opt()
    assert o.lr_spec is None and o.current_lr is None and not o.decay and not o.nesterov  # all off by default


# ------------------------------------------------- the CPU path, float64 form
def _ref64(kind, p, g, s1, s2, t, lr, wd, nesterov, m=0.9, b1=0.9, b2=0.999, rho=0.9):
    """One float64 step of the TF1 formulas with the coupled L2 term; t = steps taken so far."""
    g = g + wd * p
    if kind == "sgd":
        return p - lr * g, s1, s2
    if kind == "momentum":
        s1 = s1 * m + g
        return (p - (g * lr + s1 * m * lr) if nesterov else p - lr * s1), s1, s2
    if kind == "adam":
        lr_t = lr * np.sqrt(1 - b2 ** (t + 1)) / (1 - b1 ** (t + 1))
        s1 = b1 * s1 + (1 - b1) * g
        s2 = b2 * s2 + (1 - b2) * g * g
        return p - lr_t * s1 / (np.sqrt(s2) + 1e-8), s1, s2
    s1 = rho * s1 + (1 - rho) * g * g
    s2 = m * s2 + lr * g / np.sqrt(s1 + 1e-10)
    return p - s2, s1, s2


@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam", "rmsprop"])
def test_step_cpu_with_schedule_decay_and_nesterov_matches_float64(kind):
    nesterov = kind == "momentum"
    sched = dict(lr_boundaries=(1, 3), lr_values=(0.1, 0.03, 0.004), lr_warmup_steps=2)
    o, P, gs = _opt(kind, weight_decay=0.01, decay_vars=("w/kernel", "v/kernel"), nesterov=nesterov, **sched)
    p = P.master.double().numpy().copy()
    s1 = np.ones_like(p) if kind == "rmsprop" else np.zeros_like(p)
    s2 = np.zeros_like(p)
    wd = np.zeros_like(p)
    for n in ("w/kernel", "v/kernel"):
        wd[P.offsets[n]:P.offsets[n] + P.spec(n).numel] = 0.01
    gen = torch.Generator().manual_seed(5)
    for t in range(6):
        g = torch.randn(P.total, generator=gen)
        lr = _warm64(_piecewise64(t, (1, 3), (0.1, 0.03, 0.004)), t, 2)
        o.step(grad=g)
        assert abs(float(o.current_lr.item()) - lr) <= 1e-7 and int(gs.item()) == t + 1
        p, s1, s2 = _ref64(kind, p, g.double().numpy(), s1, s2, t, lr, wd, nesterov)
        for n in o.var_list:  # (the padding between variables is not updated)
            sl = slice(P.offsets[n], P.offsets[n] + P.spec(n).numel)
            np.testing.assert_allclose(P.master.numpy()[sl], p[sl], rtol=1e-5, atol=1e-5)
    # the features are not no-ops: the plain optimizer ends elsewhere
    o2, P2, _ = _opt(kind)
    gen = torch.Generator().manual_seed(5)
    for t in range(6):
        o2.step(grad=torch.randn(P2.total, generator=gen))
    assert not torch.allclose(P2.master, P.master, rtol=1e-3, atol=1e-3)


def test_an_optimizer_with_a_preset_global_step_applies_that_steps_rate():
    """What a restore relies on: the rate is a function of the checkpointed global_step alone."""
    o, P, gs = _opt("sgd", lr_boundaries=(4, 9), lr_values=(0.1, 0.01, 0.001))
    gs.fill_(7)
    before = P.master.clone()
    g = torch.ones(P.total)
    o.step(grad=g)
    assert float(o.current_lr.item()) == float(np.float32(0.01)) and int(gs.item()) == 8
    sl = slice(P.offsets["v/kernel"], P.offsets["v/kernel"] + 70)
    torch.testing.assert_close(P.master[sl], before[sl] - 0.01, rtol=1e-6, atol=1e-7)
    gs.fill_(10)
    o.step(grad=g)
    assert float(o.current_lr.item()) == float(np.float32(0.001))


def test_step_all_with_a_schedule_takes_the_sequential_path_on_the_cpu_too():
    P = FlatParams(_specs(), "cpu", seed=1)
    gs = torch.zeros(1, dtype=torch.int32)
    mk = lambda vl: Optimizer(OptimizerConfig(kind="adam", lr=0.1, lr_warmup_steps=4), P, var_list=vl, global_step=gs)
    opts = [mk(["w/kernel", "w/bias"]), mk(["v/kernel"])]
    P.grad.fill_(1.0)
    for step in range(3):
        Optimizer.step_all(opts, [0, 1])
        want = float(ops.lr_schedule_value(opts[0].lr_spec, step))
        assert [float(o.current_lr.item()) for o in opts] == [want, want]


# -------------------------------------------------------------------- flags
def test_flags_parse_and_default_to_off(capsys):
    f = flagmod.parse([])
    assert (f.lr_boundaries, f.lr_values, f.lr_decay_steps, f.lr_end, f.lr_warmup_steps, f.weight_decay, f.nesterov) \
        == ((), (), 0, 0.0, 0, 0.0, False)
    assert flagmod.recipe_flags(f) == []
    f = flagmod.parse(["--lr_boundaries", "32000,48000", "--lr_values=0.1,0.01,0.001", "--lr_warmup_steps", "5",
                       "--weight_decay", "1e-4", "--nesterov"])
    assert f.lr_boundaries == (32000, 48000) and f.lr_values == (0.1, 0.01, 0.001)
    assert f.lr_warmup_steps == 5 and f.weight_decay == 1e-4 and f.nesterov is True
    f = flagmod.parse(["--lr_decay_steps=64000", "--lr_end", "0.0001"])
    assert (f.lr_decay_steps, f.lr_end) == (64000, 0.0001) and flagmod.recipe_flags(f) == ["--lr_decay_steps"]
    for bad in (["--weight_decay=-1"], ["--lr_end=0.1"]):
        with pytest.raises(SystemExit):
            flagmod.parse(bad)
    assert "--lr_decay_steps" in capsys.readouterr().err


def _run(model, extra, tmp_path):
    return train.run(model, ["--device=cpu", "--synthetic", "--num_steps=1", "--batch_size=4", "--save_model_secs=0",
                             "--model_dir=" + str(tmp_path)] + extra, log=lambda *_: None)


@pytest.mark.parametrize("extra", [["--lr_warmup_steps=5"], ["--weight_decay=1e-4"], ["--nesterov"],
                                   ["--lr_boundaries=1", "--lr_values=0.1,0.01"]])
def test_ps_mode_refuses_the_recipe_flags(extra, tmp_path):
    with pytest.raises(ValueError, match="--mode=ps") as e:
        _run("resnet20", ["--mode=ps", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", "--job_name=worker"]
             + extra, tmp_path)
    assert extra[0].split("=")[0] in str(e.value)


def test_cnn_own_schedule_refuses_a_schedule_without_bucket_mb(tmp_path):
    with pytest.raises(ValueError, match="--bucket_mb"):
        _run("cnn", ["--mode=local", "--lr_warmup_steps=3"], tmp_path)


def test_cnn_with_bucket_mb_takes_the_generic_path_and_the_schedule(tmp_path):
    mj = tmp_path / "m.jsonl"
    rc = _run("cnn", ["--mode=local", "--bucket_mb=4", "--lr_warmup_steps=4", "--num_steps=2",
                      "--metrics_jsonl=" + str(mj)], tmp_path)
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    lr = train.MODELS["cnn"][1]
    spec = ops.lr_schedule_spec(lr, warmup_steps=4)
    assert rc == 0 and [r["lr"] for r in rows] == [float(ops.lr_schedule_value(spec, s)) for s in (0, 1)]


@pytest.mark.parametrize("flag", ["--weight_decay=1e-4", "--nesterov"])
def test_models_without_decay_vars_refuse_weight_decay_and_nesterov(flag, tmp_path):
    with pytest.raises(ValueError, match=flag.split("=")[0]):
        _run("gan", ["--mode=local", flag], tmp_path)


# ---------------------------------------------------------------------- CLI
def test_cli_resnet20_logs_the_scheduled_rate(tmp_path):
    mj = tmp_path / "m.jsonl"
    rc = _run("resnet20", ["--mode=local", "--num_steps=5", "--lr_boundaries=1,3", "--lr_values=0.1,0.01,0.001",
                           "--lr_warmup_steps=2", "--weight_decay=1e-4", "--nesterov", "--log_every=1",
                           "--metrics_jsonl=" + str(mj)], tmp_path)
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    spec = ops.lr_schedule_spec(0.1, (1, 3), (0.1, 0.01, 0.001), warmup_steps=2)
    assert rc == 0 and [r["gs"] for r in rows] == [1, 2, 3, 4, 5]
    assert [r["lr"] for r in rows] == [float(ops.lr_schedule_value(spec, s)) for s in range(5)]
    assert len({r["lr"] for r in rows}) == 4 and all(np.isfinite(r["loss"]) for r in rows)


def test_resnet20_declares_its_kernels_as_decaying():
    from dtfe.models.resnet import ResNetModel

    m = ResNetModel()
    names = m.opt_groups[0][1]
    assert m.decay_vars and set(m.decay_vars) < set(names)
    assert all(n.endswith("/kernel") for n in m.decay_vars)
    rest = [n for n in names if n not in m.decay_vars]
    assert rest and all(n.endswith(("/gamma", "/beta", "/bias")) for n in rest)
