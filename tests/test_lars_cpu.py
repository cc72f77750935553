"""Layer-wise adaptive rate scaling off the GPU: the numpy-float32 mirror of the trust ratio, the CPU path of
Optimizer.step against a float64 transcription of tf.contrib.opt.LARSOptimizer, the flags and their refusals,
and the ResNet-20 CLI's metrics row with and without --lars_eeta."""
import json

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.optim import FlatParams, LayerTrust, Optimizer, OptimizerConfig, VarSpec
from dtfe.utils import flags as flagmod


def _init(shape, g):
    return torch.randn(*shape, generator=g)


# the GPU tests' variable set (tests/test_lars_gpu.py)
SPECS = [
    VarSpec("a1", (1,), _init),
    VarSpec("out0", (100,), _init, bf16=True),            # not in the var list
    VarSpec("a3", (3,), _init),
    VarSpec("a64", (64,), _init, bf16=True),
    VarSpec("a1027", (1027,), _init),
    VarSpec("skip", (300,), _init, bf16=True),            # in the var list, not adaptive
    VarSpec("a8197", (8192 + 5,), _init, bf16=True),
    VarSpec("zw", (1500,), lambda shape, g: torch.zeros(*shape)),   # adaptive, master all zeros
    VarSpec("a3x8192", (3 * 8192,), _init),
    VarSpec("tr", (70, 130), _init, bf16=True, transpose=(70, 1, 130)),
    VarSpec("zg", (2000,), _init, bf16=True),             # adaptive, gradient all zeros
    VarSpec("out1", (5000,), _init),                       # not in the var list
    # 67 chunks of 1024: the fold's second strip of 64 partials, a strip that ends inside a quad
    VarSpec("a67591", (66 * 1024 + 7,), _init),
]
VAR_LIST = ["a1", "a3", "a64", "a1027", "skip", "a8197", "zw", "a3x8192", "tr", "zg", "a67591"]
ADAPTIVE = [n for n in VAR_LIST if n != "skip"]
DECAY = ["a64", "a8197", "tr", "zw", "skip"]
WD, EETA, EPS, LR, MOM = 0.01, 0.02, 1e-6, 0.05, 0.9


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _sl(P, n):
    return slice(P.offsets[n], P.offsets[n] + P.spec(n).numel)


def _grad(P, seed):
    g = torch.full((P.total,), float("nan"))
    gen = torch.Generator().manual_seed(seed)
    for n in VAR_LIST:
        g[_sl(P, n)] = 0.0 if n == "zg" else torch.randn(P.spec(n).numel, generator=gen)
    return g


# ------------------------------------------------------------------ the mirror
def test_trust_mirror_edge_cases():
    f = np.float32
    one = _bits(f(1))
    assert ops.lars_trust_ref(4.0, 9.0, 0.5, 0.0, 0.0).dtype == np.float32
    # a zero (or non-finite-compare) norm: exactly 1, whatever the rest
    for sw, sg in ((0.0, 9.0), (4.0, 0.0), (0.0, 0.0), (float("nan"), 1.0), (1.0, float("nan"))):
        assert _bits(ops.lars_trust_ref(sw, sg, 0.5, 0.1, 0.3)) == one, (sw, sg)
    assert _bits(ops.lars_trust_ref(4.0, 9.0, 0.5, 0.1, 0.3, clip_scale=0.0)) == one  # a clip to nothing
    # exact cases: |w| = 2, |g| = 3
    assert _bits(ops.lars_trust_ref(4.0, 9.0, 0.5, 0.0, 0.0)) == _bits(f(1) / f(3))
    assert _bits(ops.lars_trust_ref(4.0, 9.0, 0.5, 0.5, 0.0)) == _bits(f(0.25))       # 1 / (3 + 1)
    assert _bits(ops.lars_trust_ref(4.0, 9.0, 0.5, 0.5, 4.0)) == _bits(f(0.125))      # 1 / (3 + 1 + 4)
    assert _bits(ops.lars_trust_ref(4.0, 9.0, 0.5, 0.5, 0.0, clip_scale=0.5)) == _bits(f(0.4))  # 1 / (1.5 + 1)
    # operation for operation in float32, and within a few roundings of float64
    rng = np.random.RandomState(7)
    for _ in range(200):
        sw, sg = f(rng.uniform(1e-3, 1e4)), f(rng.uniform(1e-6, 1e4))
        eeta, wd, eps, clip = rng.uniform(1e-4, 1.0), rng.uniform(0, 0.1), rng.uniform(0, 1e-3), f(rng.uniform(0.1, 1))
        got = ops.lars_trust_ref(sw, sg, eeta, wd, eps, clip)
        wn, gn = np.sqrt(sw), f(np.sqrt(sg) * clip)
        assert _bits(got) == _bits(f(f(eeta) * wn) / f(f(gn + f(f(wd) * wn)) + f(eps)))
        ref = float(f(eeta)) * np.sqrt(float(sw)) / (np.sqrt(float(sg)) * float(clip) + float(f(wd)) * np.sqrt(float(sw))
                                                     + float(f(eps)))
        assert abs(float(got) - ref) <= 4 * np.spacing(f(ref))


# ---------------------------------------------------------------- the CPU path
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("clip_norm", [0.0, 7.0])
def test_cpu_step_matches_a_float64_transcription_of_lars(nesterov, clip_norm):
    P = FlatParams(SPECS, "cpu", seed=3)
    init = P.master.clone()
    cfg = OptimizerConfig(kind="momentum", lr=LR, momentum=MOM, nesterov=nesterov, clip_norm=clip_norm, weight_decay=WD,
                          decay_vars=tuple(DECAY), lars_eeta=EETA, lars_epsilon=EPS, lars_vars=tuple(ADAPTIVE))
    o = Optimizer(cfg, P, var_list=VAR_LIST)
    assert o.layer_trust.tolist() == [1.0] * len(VAR_LIST)
    var = {n: P.master[_sl(P, n)].double().clone() for n in VAR_LIST}
    acc = {n: torch.zeros_like(v) for n, v in var.items()}
    gscale = 1.0 / 3.0
    for step in range(2):
        g = _grad(P, 20 + step)
        o.step(grad=g, gscale=gscale)
        grads = {n: g[_sl(P, n)].double() * float(np.float32(gscale)) for n in VAR_LIST}
        if clip_norm:  # tf.clip_by_global_norm over the var list, before the optimizer sees the gradient
            norm = float(torch.cat(list(grads.values())).norm())
            assert norm > clip_norm
            grads = {n: x * (clip_norm / norm) for n, x in grads.items()}
        for i, n in enumerate(VAR_LIST):
            # LARSOptimizer.compute_lr, then ApplyMomentum
            w_norm, g_norm, wd = float(var[n].norm()), float(grads[n].norm()), WD if n in DECAY else 0.0
            trust = 1.0
            if n in ADAPTIVE and w_norm > 0 and g_norm > 0:
                trust = EETA * w_norm / (g_norm + wd * w_norm + EPS)
            assert abs(float(o.layer_trust[i]) - trust) <= 3e-5 * trust, (n, float(o.layer_trust[i]), trust)
            if n in ("skip", "zg") or (n == "zw" and step == 0):
                assert float(o.layer_trust[i]) == 1.0
            gr = grads[n] + wd * var[n]
            acc[n] = acc[n] * MOM + gr
            lr = LR * trust
            var[n] = var[n] - (gr * lr + acc[n] * MOM * lr if nesterov else lr * acc[n])
    for n in VAR_LIST:
        assert torch.allclose(P.master[_sl(P, n)].double(), var[n], rtol=1e-5, atol=1e-6), n
        assert torch.allclose(o.s1[_sl(P, n)].double(), acc[n], rtol=1e-5, atol=1e-6), n
    for n in ("out0", "out1"):
        assert torch.equal(P.master[_sl(P, n)], init[_sl(P, n)])
    assert torch.isfinite(P.master).all()


def test_cpu_trust_is_the_mirror_of_its_own_sums_and_zero_eeta_is_off():
    P, Q = FlatParams(SPECS, "cpu", seed=3), FlatParams(SPECS, "cpu", seed=3)
    wd = [WD if n in DECAY else 0.0 for n in VAR_LIST]
    lt = LayerTrust(P, VAR_LIST, ADAPTIVE, wd, EETA, EPS)
    clip = torch.tensor([0.37])
    lt.compute(_grad(P, 5), gscale=0.5, clip_scale=clip)
    for i, n in enumerate(VAR_LIST):
        want = np.float32(1) if n == "skip" else \
            ops.lars_trust_ref(lt.sums[i, 0].item(), lt.sums[i, 1].item(), EETA, wd[i], EPS, 0.37)
        assert _bits(lt.trust[i].item()) == _bits(want), n
    a = Optimizer(OptimizerConfig(kind="momentum", lr=LR, momentum=MOM, lars_eeta=0.0, lars_vars=tuple(ADAPTIVE)), P,
                  var_list=VAR_LIST)
    b = Optimizer(OptimizerConfig(kind="momentum", lr=LR, momentum=MOM), Q, var_list=VAR_LIST)
    assert a.lars is None and a.layer_trust is None
    for s in range(2):
        a.step(grad=_grad(P, s))
        b.step(grad=_grad(P, s))
    assert torch.equal(P.master, Q.master) and torch.equal(a.s1, b.s1)


def test_optimizer_config_validation():
    P = FlatParams(SPECS, "cpu", seed=3)
    for kind in ("sgd", "adam", "rmsprop"):
        with pytest.raises(ValueError, match="momentum optimizer"):
            Optimizer(OptimizerConfig(kind=kind, lars_eeta=0.01), P, var_list=VAR_LIST)
    m = dict(kind="momentum", momentum=MOM)
    with pytest.raises(ValueError, match="lars_vars"):
        Optimizer(OptimizerConfig(lars_eeta=0.01, lars_vars=("out0",), **m), P, var_list=VAR_LIST)
    with pytest.raises(ValueError, match="lars_eeta"):
        Optimizer(OptimizerConfig(lars_eeta=-1.0, **m), P, var_list=VAR_LIST)
    with pytest.raises(ValueError, match="epsilon"):
        Optimizer(OptimizerConfig(lars_eeta=0.01, lars_epsilon=-1.0, **m), P, var_list=VAR_LIST)
    o = Optimizer(OptimizerConfig(lars_eeta=0.01, **m), P, var_list=VAR_LIST)  # lars_vars None: the whole var list
    assert o.lars.adaptive == VAR_LIST
    with pytest.raises(ValueError, match="wait="):
        o.step(grad=_grad(P, 1), wait=(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), ["a1"]))


# ------------------------------------------------------------------------ flags
D = dict(batch_size=8, num_steps=1, learning_rate=0.1)


def test_flags_parse_and_validate():
    fl = flagmod.parse([], model_defaults=D)
    assert fl.lars_eeta == 0.0 and fl.lars_epsilon == 0.0 and flagmod.lars_flags(fl) == []
    fl = flagmod.parse(["--lars_eeta=0.001", "--lars_epsilon", "1e-9"], model_defaults=D)
    assert fl.lars_eeta == 0.001 and fl.lars_epsilon == 1e-9
    assert flagmod.lars_flags(fl) == ["--lars_eeta", "--lars_epsilon"]
    assert flagmod.recipe_flags(fl) == [] and flagmod.ema_flags(fl) == []
    for bad in (["--lars_eeta=-0.1"], ["--lars_eeta=nan"], ["--lars_eeta=inf"], ["--lars_epsilon=1e-9"],
                ["--lars_eeta=0.1", "--lars_epsilon=-1"]):
        with pytest.raises(SystemExit):
            flagmod.parse(bad, model_defaults=D)


BASE = ["--device=cpu", "--synthetic", "--batch_size=4", "--num_steps=1", "--save_model_secs=0"]


def test_ps_mode_refuses_the_flag(tmp_path):
    with pytest.raises(ValueError, match="--mode=ps") as e:
        train.run("resnet20", BASE + ["--mode=ps", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2",
                                      "--job_name=worker", "--lars_eeta=0.001", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)
    assert str(e.value) == train.PS_LARS_ERROR % "--lars_eeta"


def test_a_model_without_decay_vars_refuses_the_flag(tmp_path):
    with pytest.raises(ValueError, match="decaying variables") as e:
        train.run("lstm", BASE + ["--mode=local", "--lars_eeta=0.001", "--lars_epsilon=1e-9",
                                  "--model_dir=" + str(tmp_path)], log=lambda *_: None)
    assert str(e.value) == train.MODEL_LARS_ERROR % ("--lars_eeta --lars_epsilon", "lstm")


def test_cnn_own_schedule_refuses_the_flag_without_bucket_mb(tmp_path):
    with pytest.raises(ValueError, match="--bucket_mb") as e:
        train.run("cnn", BASE + ["--mode=local", "--lars_eeta=0.001", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)
    assert str(e.value) == train.CNN_LARS_ERROR % "--lars_eeta"
    # on the generic path the CNN is an Adam model without decaying variables: refused as such
    with pytest.raises(ValueError, match="decaying variables"):
        train.run("cnn", BASE + ["--mode=local", "--bucket_mb=4", "--lars_eeta=0.001", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)


# -------------------------------------------------------------------------- CLI
def _resnet20(tmp_path, name, extra):
    mj = tmp_path / (name + ".jsonl")
    logs = []
    # one example: the smallest batch the CPU model accepts
    rc = train.run("resnet20", ["--device=cpu", "--synthetic", "--batch_size=1", "--num_steps=2", "--save_model_secs=0",
                                "--mode=local", "--seed=3", "--model_dir=" + str(tmp_path / name),
                                "--metrics_jsonl=" + str(mj)] + extra, log=logs.append)
    assert rc == 0
    return [json.loads(r) for r in mj.read_text().splitlines()]


def test_resnet20_cli_reports_the_trust_range_only_with_the_flag(tmp_path):
    rows = _resnet20(tmp_path, "lars", ["--lars_eeta=0.001", "--weight_decay=1e-4"])
    assert [r["gs"] for r in rows] == [1, 2]
    for r in rows:
        assert 0 < r["trust_min"] <= r["trust_max"] <= 10.0 and np.isfinite(r["loss"]), r  # eeta / wd bounds it
    plain = _resnet20(tmp_path, "plain", ["--weight_decay=1e-4"])
    assert [r["gs"] for r in plain] == [1, 2]
    assert not any(k.startswith("trust") for r in plain for k in r), plain
    # the same first batch and weights: the first step's loss agrees, the flag changed the update only
    assert rows[0]["loss"] == plain[0]["loss"] and rows[1]["loss"] != plain[1]["loss"]
