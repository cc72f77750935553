"""The exponential moving average of the weights off the GPU: the numpy-float32 host mirrors against a
float64 recurrence, the CPU optimizer path against the mirrors (bitwise: it goes through them), the
checkpoint round trip of the shadow, the flags and their refusals, and the lstm CLI's two accuracy lines."""
import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.models.lstm import LstmModel
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig, VarSpec
from dtfe.utils import flags as flagmod


def _init(shape, g):
    return torch.randn(*shape, generator=g)


SPECS = [
    VarSpec("a3", (3,), _init),
    VarSpec("out0", (10,), _init, bf16=True),                 # not in the var list
    VarSpec("a70", (70,), _init, bf16=True),
    VarSpec("tr", (5, 2, 3), _init, bf16=True, transpose=(5, 2, 3)),
]
VAR_LIST = ["a3", "a70", "tr"]
KINDS = ["sgd", "momentum", "adam", "rmsprop"]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _opt(P, kind, gs=None, **kw):
    cfg = OptimizerConfig(kind=kind, lr=0.05, momentum=0.9 if kind in ("momentum", "rmsprop") else 0.0, **kw)
    return Optimizer(cfg, P, var_list=VAR_LIST, global_step=gs)


def _slices(P, names=VAR_LIST):
    return [slice(P.offsets[n], P.offsets[n] + P.spec(n).numel) for n in names]


# ------------------------------------------------------------------ the mirrors
def test_decay_value_mirror():
    f = np.float32
    assert _bits(ops.ema_decay_value(0.999, False, 123)) == _bits(f(0.999))
    for n in range(40):
        want = min(f(0.6), f(f(1 + n) / f(10 + n)))
        got = ops.ema_decay_value(0.6, True, n)
        assert got.dtype == np.float32 and _bits(got) == _bits(want)
        # the float32 quotient is the correctly rounded one
        assert _bits(f(f(1 + n) / f(10 + n))) == _bits(f((1 + n) / (10 + n)))
    assert _bits(ops.ema_decay_value(0.6, True, 13)) == _bits(f(0.6))  # (1 + 13) / (10 + 13) > 0.6
    assert float(ops.ema_decay_value(0.6, True, 12)) < float(f(0.6))


def test_update_mirror_within_one_ulp_of_float64_per_step():
    """Every step of the mirror's recurrence against the same step in float64 (from the mirror's own float32
    shadow): at most 1 ulp of the result.  The inputs, drawn once: per element a sign and a binade
    [m, 2m), m = 2^-20 .. 2^20, that shadow and values share - the case of a weight and its average - and a
    decay per step in [0.5, 1).  There 1 - d and shadow - value are exact (Sterbenz), the product is below
    m / 2 and rounds with at most 1/8 ulp of a result in [m, 2m), the last subtraction with 1/2: 0.625 ulp
    in all.  (Operands of opposite sign can cancel in the last subtraction; an error counted in ulps of
    the result has no bound then, for the mirror as for any float32 evaluation of the formula.)"""
    rng = np.random.RandomState(1234)
    f = np.float32
    n = 4096
    scale = (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 2.0 ** rng.randint(-20, 21, n)).astype(f)
    shadow = (scale * rng.uniform(1.0, 2.0, n).astype(f)).astype(f)
    worst = 0.0
    for step in range(50):
        d = f(rng.uniform(0.5, 1.0))
        assert f(0.5) <= d < f(1)
        value = (scale * np.minimum(rng.uniform(1.0, 2.0, n).astype(f), np.nextafter(f(2), f(0)))).astype(f)
        got = ops.ema_update_ref(shadow, value, d)
        assert got.dtype == np.float32
        s64, v64 = shadow.astype(np.float64), value.astype(np.float64)
        want = s64 - (s64 - v64) * (1.0 - float(d))
        ulp = np.spacing(np.abs(want).astype(f)).astype(np.float64)
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / ulp).max()))
        shadow = got
    print("worst error of a step: %.3f ulp" % worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- the CPU path
@pytest.mark.parametrize("num_updates", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_optimizer_shadow_equals_the_mirror(kind, num_updates):
    Pa, Pb = FlatParams(SPECS, "cpu", seed=3), FlatParams(SPECS, "cpu", seed=3)
    gsa, gsb = (torch.zeros(1, dtype=torch.int32) for _ in range(2))
    a = _opt(Pa, kind, gsa, ema_decay=0.6, ema_num_updates=num_updates)
    b = _opt(Pb, kind, gsb)
    assert b.ema is None and b.current_ema_decay is None
    init = Pa.master.clone()
    assert torch.equal(a.ema, init) and a.ema.data_ptr() != Pa.master.data_ptr()
    shadow = init.numpy().copy()
    gen = torch.Generator().manual_seed(5)
    for step in range(16):  # (1 + n) / (10 + n) reaches 0.6 at n = 13
        g = torch.randn(Pa.total, generator=gen)
        a.step(grad=g)
        b.step(grad=g)
        d = ops.ema_decay_value(0.6, num_updates, step + 1)  # the step after the advance
        assert _bits(a.current_ema_decay.item()) == _bits(d)
        for sl in _slices(Pa):
            shadow[sl] = ops.ema_update_ref(shadow[sl], Pa.master.numpy()[sl], d)
        assert np.array_equal(_bits(a.ema.numpy()), _bits(shadow))
        # the trained state is the one of an optimizer without EMA
        assert torch.equal(Pa.master, Pb.master)
        for x, y in ((a.s1, b.s1), (a.s2, b.s2), (a.beta_pow, b.beta_pow)):
            assert (x is None and y is None) or torch.equal(x, y)
    out = slice(Pa.offsets["out0"], Pa.offsets["out0"] + 10)
    assert torch.equal(a.ema[out], init[out])  # outside the var list: never written
    if num_updates:
        assert float(a.current_ema_decay.item()) == float(np.float32(0.6))


def test_cpu_swap_and_averaged():
    P = FlatParams(SPECS, "cpu", seed=3)
    o = _opt(P, "momentum", ema_decay=0.5)
    gen = torch.Generator().manual_seed(6)
    for _ in range(3):
        o.step(grad=torch.randn(P.total, generator=gen))
    P.refresh_copies()  # (the CPU step leaves the copies to its caller; on the GPU the apply writes them)
    m0, e0 = P.master.clone(), o.ema.clone()
    w0 ={k: v.clone() for k, v in list(P.w16.items()) + [("t/" + k, v) for k, v in P.wt16.items()]}
    assert not torch.equal(m0, e0)
    o.swap_ema()
    out = slice(P.offsets["out0"], P.offsets["out0"] + 10)
    for sl in _slices(P):
        assert torch.equal(P.master[sl], e0[sl]) and torch.equal(o.ema[sl], m0[sl])
    assert torch.equal(P.master[out], m0[out]) and torch.equal(o.ema[out], e0[out])
    assert torch.equal(P.w16["a70"], P.view("a70").to(torch.bfloat16))
    assert torch.equal(P.wt16["tr"], P.view("tr").permute(2, 1, 0).reshape(-1).to(torch.bfloat16))
    assert torch.equal(P.w16["out0"], w0["out0"])
    o.swap_ema()

    def same():
        assert torch.equal(P.master, m0) and torch.equal(o.ema, e0)
        for k, v in w0.items():
            assert torch.equal(P.wt16[k[2:]] if k.startswith("t/") else P.w16[k], v)
    same()
    with pytest.raises(RuntimeError, match="body"):
        with o.averaged():
            assert torch.equal(P.view("a3"), e0[_slices(P, ["a3"])[0]])
            raise RuntimeError("body")
    same()
    with pytest.raises(ValueError, match="moving average"):
        _opt(P, "sgd").swap_ema()


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_of_the_shadow():
    model = LstmModel()
    cpu = torch.device("cpu")

    def make(ema, seed):
        prog = model.program(cpu, 4, seed=seed)
        gs = torch.zeros(1, dtype=torch.int32)
        opts = []
        for cfg, vl, bp in model.opt_groups:
            cfg = OptimizerConfig(**dict(cfg.__dict__, ema_decay=0.5 if ema else 0.0))
            opts.append(Optimizer(cfg, prog.P, var_list=vl, global_step=gs, beta_power_names=bp))
        return prog, opts, gs

    prog, opts, gs = make(True, 0)
    gen = torch.Generator().manual_seed(7)
    for _ in range(2):
        for o in opts:
            o.step(grad=torch.randn(prog.P.total, generator=gen))
    t = train.tensors_from_flat(model, prog.P, opts, int(gs.item()))
    trained = [n for _c, vl, _b in model.opt_groups for n in vl]
    ema_keys = sorted(k for k in t if k.endswith("/ExponentialMovingAverage"))
    assert ema_keys == sorted(n + "/ExponentialMovingAverage" for n in trained)
    # with the key: the shadow comes back, and it is not the variable
    prog2, opts2, _ = make(True, 1)
    train.load_flat_from_tensors(model, prog2.P, opts2, t)
    assert torch.equal(prog2.P.master, prog.P.master)
    for o, o2 in zip(opts, opts2):
        assert torch.equal(o2.ema, o.ema) and not torch.equal(o2.ema, prog2.P.master)
    # without it (a run without EMA wrote the checkpoint): the shadow starts at the restored variable
    t_plain = {k: v for k, v in t.items() if not k.endswith("/ExponentialMovingAverage")}
    prog3, opts3, _ = make(True, 2)
    train.load_flat_from_tensors(model, prog3.P, opts3, t_plain)
    for o3 in opts3:
        for sl in [slice(prog3.P.offsets[n], prog3.P.offsets[n] + prog3.P.spec(n).numel) for n in o3.var_list]:
            assert torch.equal(o3.ema[sl], prog.P.master[sl])
    # and an optimizer without EMA writes no such key and reads a checkpoint that has them
    prog4, opts4, gs4 = make(False, 3)
    assert not any("ExponentialMovingAverage" in k for k in train.tensors_from_flat(model, prog4.P, opts4, 0))
    train.load_flat_from_tensors(model, prog4.P, opts4, t)
    assert torch.equal(prog4.P.master, prog.P.master)


# ------------------------------------------------------------------------ flags
D = dict(batch_size=8, num_steps=1, learning_rate=0.1)


def test_flags_parse_and_validate():
    fl = flagmod.parse([], model_defaults=D)
    assert fl.ema_decay == 0.0 and fl.ema_num_updates is False and flagmod.ema_flags(fl) == []
    fl = flagmod.parse(["--ema_decay=0.999", "--ema_num_updates"], model_defaults=D)
    assert fl.ema_decay == 0.999 and fl.ema_num_updates is True
    assert flagmod.ema_flags(fl) == ["--ema_decay", "--ema_num_updates"]
    assert flagmod.recipe_flags(fl) == []
    for bad in (["--ema_decay=1.0"], ["--ema_decay=-0.1"], ["--ema_decay=nan"], ["--ema_num_updates"]):
        with pytest.raises(SystemExit):
            flagmod.parse(bad, model_defaults=D)


def test_optimizer_config_validation():
    P = FlatParams(SPECS, "cpu", seed=3)
    for bad in (1.0, -0.1, float("nan"), 1.0 - 1e-12):  # the last rounds to 1 in float32
        with pytest.raises(ValueError, match="ema_decay"):
            _opt(P, "sgd", ema_decay=bad)
    with pytest.raises(ValueError, match="global_step"):
        _opt(P, "sgd", ema_decay=0.5, ema_num_updates=True)
    with pytest.raises(ValueError, match="ema_decay"):
        _opt(P, "sgd", torch.zeros(1, dtype=torch.int32), ema_num_updates=True)
    assert _opt(P, "sgd").ema is None


BASE = ["--device=cpu", "--synthetic", "--batch_size=4", "--num_steps=1", "--save_model_secs=0"]


@pytest.mark.parametrize("extra", [["--ema_decay=0.9"], ["--ema_decay=0.9", "--ema_num_updates"]])
def test_ps_mode_refuses_ema(extra, tmp_path):
    with pytest.raises(ValueError, match="--mode=ps") as e:
        train.run("resnet20", BASE + ["--mode=ps", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2",
                                      "--job_name=worker", "--model_dir=" + str(tmp_path)] + extra, log=lambda *_: None)
    assert "--ema_decay" in str(e.value) and "moving average" in str(e.value)
    assert str(e.value) == train.PS_EMA_ERROR % " ".join(x.split("=")[0] for x in extra)


def test_cnn_own_schedule_refuses_ema_without_bucket_mb(tmp_path):
    with pytest.raises(ValueError, match="--bucket_mb") as e:
        train.run("cnn", BASE + ["--mode=local", "--ema_decay=0.9", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)
    assert str(e.value) == train.CNN_EMA_ERROR % "--ema_decay"


# -------------------------------------------------------------------------- CLI
def _lstm(tmp_path, extra):
    logs = []
    mj = tmp_path / "m.jsonl"
    rc = train.run("lstm", BASE + ["--num_steps=3", "--model_dir=" + str(tmp_path / "ck"),
                                   "--metrics_jsonl=" + str(mj)] + extra, log=logs.append)
    assert rc == 0
    return logs, mj.read_text()


def test_lstm_cli_prints_both_accuracy_lines(tmp_path):
    import json

    logs, rows = _lstm(tmp_path, ["--ema_decay=0.9", "--ema_num_updates"])
    acc = [l for l in logs if "Test-Accuracy" in l]
    assert len(acc) == 2 and acc[0].startswith("Test-Accuracy: ") and acc[1].startswith("EMA Test-Accuracy: ")
    rows = [json.loads(r) for r in rows.splitlines()]
    assert [_bits(r["ema_decay"]).item() for r in rows] == \
        [_bits(ops.ema_decay_value(0.9, True, n)).item() for n in (1, 2, 3)]


def test_lstm_cli_without_the_flag_says_nothing_of_ema(tmp_path):
    logs, rows = _lstm(tmp_path, [])
    assert len([l for l in logs if "Test-Accuracy" in l]) == 1
    assert "EMA" not in "\n".join(logs) and "ema" not in rows
