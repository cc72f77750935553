"""The exponential moving average of the weights inside the fused apply, and the swap that puts it to use,
on the device.  Every comparison is bitwise: the shadow against the numpy-float32 host mirror fed with the
masters read back after each step, everything else against a twin optimizer without EMA, the swap against
what it exchanged, a captured replay against eager launches.  Each case runs with the plan's default chunk
for this small var list (2048: update_vec4, scalar tails, tiles) and with 8192 (the 4-in-flight body)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dtfe import ckpt, ops, train  # noqa: E402
from dtfe.data import cifar  # noqa: E402
from dtfe.models.resnet import ResNetModel  # noqa: E402
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig, VarSpec  # noqa: E402
from dtfe.utils import flags as flagmod  # noqa: E402
from dtfe.utils.device_eval import DeviceEvaluator  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _init(shape, g):
    return torch.randn(*shape, generator=g)


# every path of the kernel: single elements, a vector body with a tail, a second chunk of 5 elements, exact
# chunks, the transposed-tile path with both bf16 copies (partial tiles in both directions, 3 taps) - and two
# variables NOT in the var list
SPECS = [
    VarSpec("a1", (1,), _init),
    VarSpec("out0", (100,), _init, bf16=True),            # not in the var list
    VarSpec("a3", (3,), _init),
    VarSpec("a64", (64,), _init, bf16=True),
    VarSpec("a1027", (1027,), _init),
    VarSpec("a8197", (8192 + 5,), _init, bf16=True),
    VarSpec("a3x8192", (3 * 8192,), _init),
    VarSpec("tr", (70, 3, 65), _init, bf16=True, transpose=(70, 3, 65)),
    VarSpec("out1", (5000,), _init),                       # not in the var list
]
VAR_LIST = ["a1", "a3", "a64", "a1027", "a8197", "a3x8192", "tr"]
OUTSIDE = ["out0", "out1"]
KINDS = ["sgd", "momentum", "adam", "rmsprop"]
CHUNKS = [2048, 8192]
D = 0.6


def _params(seed=3):
    return FlatParams(SPECS, DEV, seed=seed)


def _fill_grad(P, seed, names=VAR_LIST, dtype=torch.float32):
    """A full-size gradient: NaN everywhere (padding and foreign variables included), seeded normal
    values in the given variables only."""
    g = torch.full((P.total,), float("nan"), dtype=torch.float32)
    gen = torch.Generator().manual_seed(seed)
    for n in names:
        o, k = P.offsets[n], P.spec(n).numel
        g[o:o + k] = torch.randn(k, generator=gen)
    return g.to(dtype).to(DEV)


def _gs():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _opt(P, kind, gs=None, var_list=VAR_LIST, chunk=0, **kw):
    kw.setdefault("lr", 0.05)
    cfg = OptimizerConfig(kind=kind, momentum=0.9 if kind in ("momentum", "rmsprop") else 0.0, **kw)
    o = Optimizer(cfg, P, var_list=var_list, global_step=gs)
    if chunk:
        o._build_plan(chunk)
    return o


def _state(P, opt):
    t = {"master": P.master, "s1": opt.s1, "s2": opt.s2, "beta_pow": opt.beta_pow}
    t.update({"w16/" + k: v for k, v in P.w16.items()})
    t.update({"wt16/" + k: v for k, v in P.wt16.items()})
    return {k: v.clone() for k, v in t.items() if v is not None}


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:  # bits: -0 is not +0
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _slices(P, names):
    return [slice(P.offsets[n], P.offsets[n] + P.spec(n).numel) for n in names]


def _mirror_step(P, shadow, d, names=VAR_LIST):
    """shadow (numpy, full size) after one EMA update from the masters as they are now."""
    m = P.master.cpu().numpy()
    for sl in _slices(P, names):
        shadow[sl] = ops.ema_update_ref(shadow[sl], m[sl], d)


def _untouched_mask(P, names=VAR_LIST):
    mask = np.ones(P.total, dtype=bool)
    for sl in _slices(P, names):
        mask[sl] = False
    return mask  # variables outside the list, and the padding between variables


def _copies_follow_the_masters(P):
    for n, w in P.w16.items():
        assert torch.equal(w, P.view(n).to(torch.bfloat16)), n
    for n, w in P.wt16.items():
        R, T, C = P.spec(n).transpose
        assert torch.equal(w, P.view(n).reshape(R, T, C).permute(2, 1, 0).reshape(-1).to(torch.bfloat16)), n


# ------------------------------------------------------- shadow against the mirror
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_shadow_equals_the_mirror_and_the_rest_equals_an_optimizer_without_ema(kind, g16, chunk):
    Pa, Pb = _params(), _params()
    a = _opt(Pa, kind, chunk=chunk, ema_decay=D)
    b = _opt(Pb, kind, chunk=chunk)
    assert b.ema is None and b.current_ema_decay is None
    init = Pa.master.clone()
    assert torch.equal(a.ema, init) and a.ema.data_ptr() != Pa.master.data_ptr()
    shadow = init.cpu().numpy().copy()
    d = ops.ema_decay_value(D, False, 0)
    for step in range(6):
        g = _fill_grad(Pa, 20 + step, dtype=torch.bfloat16 if g16 else torch.float32)
        kw = dict(grad16=g) if g16 else dict(grad=g)
        a.step(gscale=1.0 / 3.0, **kw)
        b.step(gscale=1.0 / 3.0, **kw)
        _assert_same(_state(Pa, a), _state(Pb, b))
        _mirror_step(Pa, shadow, d)
        assert np.array_equal(_bits(a.ema.cpu().numpy()), _bits(shadow)), step
        assert _bits(a.current_ema_decay.item()) == _bits(d)
    mask = _untouched_mask(Pa)
    assert np.array_equal(_bits(a.ema.cpu().numpy())[mask], _bits(init.cpu().numpy())[mask])
    assert torch.isfinite(a.ema).all() and not torch.equal(a.ema, Pa.master)
    _copies_follow_the_masters(Pa)


# ------------------------------------------------------------------ num_updates
@pytest.mark.parametrize("gs_inc", [1, 2])
def test_num_updates_decay_equals_the_host_mirror_bitwise_at_every_step(gs_inc):
    P, gs = _params(), _gs()
    opt = _opt(P, "sgd", gs, ema_decay=D, ema_num_updates=True)
    g = _fill_grad(P, 5)
    shadow = P.master.cpu().numpy().copy()
    got, want = [], []
    for step in range(16):
        opt.step(grad=g, gs_inc=gs_inc)
        n = gs_inc * (step + 1)  # the step after this launch's advance
        assert int(gs.item()) == n
        dv = ops.ema_decay_value(D, True, n)
        got.append(int(_bits(opt.current_ema_decay.item())))
        want.append(int(_bits(dv)))
        _mirror_step(P, shadow, dv)
        assert np.array_equal(_bits(opt.ema.cpu().numpy()), _bits(shadow)), step
    print([float(ops.ema_decay_value(D, True, gs_inc * (s + 1))) for s in range(16)])
    assert got == want
    # both regimes: (1 + n) / (10 + n) reaches 0.6 at n = 13.  With increments of 2 the steps below 13 are
    # n = 2, 4 .. 12, so only 7 distinct values can occur in 16 steps: every one of them is compared above
    assert len(set(want)) >= (10 if gs_inc == 1 else 7)
    assert want[-1] == int(_bits(np.float32(D)))


# ------------------------------------------------------------------ composition
@pytest.mark.parametrize("chunk", CHUNKS)
def test_ema_composes_with_schedule_weight_decay_nesterov_and_clip(chunk):
    recipe = dict(lr_boundaries=(2, 5), lr_values=(0.05, 0.02, 0.003), lr_warmup_steps=3, weight_decay=0.03125 + 1e-4,
                  decay_vars=("a3", "a1027", "a8197", "tr"), nesterov=True, clip_norm=7.0)
    Pa, Pb = _params(), _params()
    gsa, gsb = _gs(), _gs()
    a = _opt(Pa, "momentum", gsa, chunk=chunk, ema_decay=D, ema_num_updates=True, **recipe)
    b = _opt(Pb, "momentum", gsb, chunk=chunk, **recipe)
    shadow = Pa.master.cpu().numpy().copy()
    for step in range(7):
        g = _fill_grad(Pa, 40 + step)
        a.step(grad=g)
        b.step(grad=g)
        assert float(a.clip_out[1].item()) < 1.0 and torch.equal(a.clip_out, b.clip_out)
        assert torch.equal(a.current_lr, b.current_lr)
        _assert_same(_state(Pa, a), _state(Pb, b))
        _mirror_step(Pa, shadow, ops.ema_decay_value(D, True, step + 1))
        assert np.array_equal(_bits(a.ema.cpu().numpy()), _bits(shadow)), step
    assert int(gsa.item()) == int(gsb.item()) == 7


# --------------------------------------------------------------------- step_all
def test_step_all_over_two_ema_optimizers_equals_the_two_steps_in_order():
    la, lb = ["a1", "a64", "a8197", "tr"], ["a3", "a1027", "a3x8192", "out1"]
    Pa, Pb = _params(), _params()
    g = _fill_grad(Pa, 80, names=la + lb)
    gsa, gsb = _gs(), _gs()
    mk = lambda P, gs: [_opt(P, "adam", gs, var_list=vl, lr=lr, ema_decay=D, ema_num_updates=True)
                        for vl, lr in ((la, 0.05), (lb, 0.01))]
    oa, ob = mk(Pa, gsa), mk(Pb, gsb)
    shadows = [Pa.master.cpu().numpy().copy() for _ in range(2)]
    for step in range(4):
        Optimizer.step_all(oa, [0, 2], grad=g)
        for o, inc in zip(ob, [0, 2]):
            o.step(grad=g, gs_inc=inc)
        for i, (x, y, inc) in enumerate(zip(oa, ob, [0, 2])):
            _assert_same(_state(Pa, x), _state(Pb, y))
            assert torch.equal(x.ema.view(torch.int32), y.ema.view(torch.int32))
            # each saw the step its own launch began with, plus its own increment
            dv = ops.ema_decay_value(D, True, 2 * step + inc)
            assert _bits(x.current_ema_decay.item()) == _bits(y.current_ema_decay.item()) == _bits(dv)
            _mirror_step(Pa, shadows[i], dv, names=x.var_list)
            assert np.array_equal(_bits(x.ema.cpu().numpy()), _bits(shadows[i]))
    assert int(gsa.item()) == int(gsb.item()) == 8


# ------------------------------------------------------------------------- swap
@pytest.mark.parametrize("chunk", CHUNKS)
def test_swap_exchanges_masters_and_shadow_and_a_second_swap_restores_everything(chunk):
    P = _params()
    o = _opt(P, "momentum", chunk=chunk, ema_decay=D)
    for step in range(3):
        o.step(grad=_fill_grad(P, 60 + step))
    before = _state(P, o)
    m0, e0 = P.master.clone(), o.ema.clone()
    done0 = o.done.clone()
    o.swap_ema()
    mask = torch.from_numpy(_untouched_mask(P)).to(DEV)
    mi, ei = P.master.view(torch.int32), o.ema.view(torch.int32)
    assert torch.equal(mi[~mask], e0.view(torch.int32)[~mask]) and torch.equal(ei[~mask], m0.view(torch.int32)[~mask])
    assert not torch.equal(mi[~mask], m0.view(torch.int32)[~mask])
    # outside variables and the padding: neither buffer is written
    assert torch.equal(mi[mask], m0.view(torch.int32)[mask]) and torch.equal(ei[mask], e0.view(torch.int32)[mask])
    assert torch.equal(P.w16["out0"], before["w16/out0"])
    _copies_follow_the_masters(P)  # natural and transposed copies follow the new masters
    assert not torch.equal(P.wt16["tr"], before["wt16/tr"])
    assert torch.equal(o.s1, before["s1"]) and torch.equal(o.done, done0)  # no slot, no counter
    o.swap_ema()
    _assert_same(_state(P, o), before)
    assert torch.equal(o.ema.view(torch.int32), e0.view(torch.int32))


def test_averaged_restores_when_its_body_raises():
    P = _params()
    o = _opt(P, "adam", ema_decay=D)
    for step in range(2):
        o.step(grad=_fill_grad(P, 65 + step))
    before, e0 = _state(P, o), o.ema.clone()
    with pytest.raises(RuntimeError, match="body"):
        with o.averaged() as got:
            assert got is o
            sl = _slices(P, ["a1027"])[0]
            assert torch.equal(P.master[sl], e0[sl])
            raise RuntimeError("body")
    _assert_same(_state(P, o), before)
    assert torch.equal(o.ema.view(torch.int32), e0.view(torch.int32))
    with pytest.raises(ValueError, match="moving average"):
        _opt(P, "sgd").swap_ema()


# ---------------------------------------------------------------------- capture
def test_a_graph_of_step_swap_swap_replayed_three_times_equals_eager():
    Pa, Pb = _params(), _params()
    gsa, gsb = _gs(), _gs()
    a = _opt(Pa, "adam", gsa, ema_decay=D, ema_num_updates=True)
    b = _opt(Pb, "adam", gsb, ema_decay=D, ema_num_updates=True)
    g = _fill_grad(Pa, 70)
    Pa.grad.copy_(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture; undone below
        a.step()
        a.swap_ema()
        a.swap_ema()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.step()
        a.swap_ema()
        a.swap_ema()
    # back to b's (fresh) state: the warm-up and the capture itself must not count
    Pa.master.copy_(Pb.master); a.s1.copy_(b.s1); a.s2.copy_(b.s2); a.beta_pow.copy_(b.beta_pow); gsa.copy_(gsb)
    a.ema.copy_(b.ema); a.current_ema_decay.copy_(b.current_ema_decay)
    Pa.refresh_copies()
    for rep in range(3):
        graph.replay()
        b.step(grad=g)
        b.swap_ema()
        b.swap_ema()
        _assert_same(_state(Pa, a), _state(Pb, b))
        assert torch.equal(a.ema.view(torch.int32), b.ema.view(torch.int32))
        assert _bits(a.current_ema_decay.item()) == _bits(ops.ema_decay_value(D, True, rep + 1))
        assert int(gsa.item()) == int(gsb.item()) == rep + 1
    assert not torch.equal(a.ema, Pa.master)


# --------------------------------------------------------------------- refusals
def test_refusals():
    la, lb = ["a1", "a64", "a8197", "tr"], ["a3", "a1027", "a3x8192"]
    P = _params()
    g = _fill_grad(P, 81)
    oa = [_opt(P, "adam", var_list=la, ema_decay=D), _opt(P, "adam", var_list=lb, ema_decay=D)]
    with pytest.raises(RuntimeError, match="EMA"):  # the op itself refuses an EMA in a group of two
        ops.apply_gradients_group([o._state for o in oa], g, None, 1.0, [o.cfg.lr for o in oa], [0, 1])
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="ema_decay"):
            _opt(P, "sgd", ema_decay=bad)
    plain = _opt(P, "sgd")
    with pytest.raises(RuntimeError, match="no EMA"):
        ops.ema_swap(plain._state)
    segs, work = plain._tables
    with pytest.raises(RuntimeError, match="ema_decay"):
        ops.opt_state(plain.kind, P.master, segs, work, plain.done, ema=torch.zeros_like(P.master), ema_decay=1.0)
    with pytest.raises(RuntimeError, match="ema"):
        ops.opt_state(plain.kind, P.master, segs, work, plain.done, ema=torch.zeros(P.total - 1, device=DEV),
                      ema_decay=0.5)
    with pytest.raises(RuntimeError, match="global_step"):
        ops.opt_state(plain.kind, P.master, segs, work, plain.done, ema=torch.zeros_like(P.master), ema_decay=0.5,
                      ema_num_updates=True)


# -------------------------------------------------------------------- evaluator
B, N_TEST = 8, 20  # the smallest batch tests/test_device_eval_gpu.py uses


def test_evaluator_inside_averaged_equals_a_program_holding_the_shadow():
    (tr_x, tr_y), (te_x, te_y) = cifar.synthetic_arrays(n_train=40, n_test=N_TEST)
    from dtfe.data.mnist import DataSet, DeviceBatcher

    dev = torch.device("cuda:0")
    prog = ResNetModel(0.1, "resnet20").program(dev, B, seed=0)
    model = prog.model
    gstep = torch.zeros(1, dtype=torch.int32, device=dev)
    cfg, var_list, bp = model.opt_groups[0]
    cfg.ema_decay = 0.5
    opt = Optimizer(cfg, prog.P, var_list=var_list, global_step=gstep, beta_power_names=bp)
    batcher = DeviceBatcher(DataSet(tr_x, tr_y, True, 1), dev, B, sampling="device")
    for _ in range(3):
        prog.load_batch(batcher.next_batch())
        prog.compute_grads()
        Optimizer.step_all([opt], [1], grad16=None, gscale=1.0)
    # a second program whose masters are the first one's, the trained variables overwritten with the shadow
    prog2 = ResNetModel(0.1, "resnet20").program(dev, B, seed=1)
    prog2.P.master.copy_(prog.P.master)
    for sl in _slices(prog.P, var_list):
        prog2.P.master[sl] = opt.ema[sl]
    prog2.P.refresh_copies()
    assert not torch.equal(prog2.P.master, prog.P.master)
    before = _state(prog.P, opt)
    e0 = opt.ema.clone()
    ev, ev2 = (DeviceEvaluator(p, te_x, te_y, topk=5, graph=False) for p in (prog, prog2))
    raw = ev.run()
    with opt.averaged():
        assert torch.equal(prog.P.master, prog2.P.master)
        for n, w in prog.P.w16.items():
            assert torch.equal(w, prog2.P.w16[n]), n
        for n, w in prog.P.wt16.items():
            assert torch.equal(w, prog2.P.wt16[n]), n
        avg = ev.run()
    want = ev2.run()
    assert avg == want and avg["examples"] == N_TEST
    print(raw, avg)
    _assert_same(_state(prog.P, opt), before)
    assert torch.equal(opt.ema, e0)
    assert ev.run() == raw


# -------------------------------------------------------------------------- CLI
def _cli(tmp_path, name, num_steps):
    mj = tmp_path / (name + ".jsonl")
    logs = []
    fl = flagmod.parse(["--device=cuda", "--synthetic", "--batch_size", str(B), "--num_steps", str(num_steps),
                        "--eval_every", "2", "--eval_examples", "64", "--ema_decay", "0.9", "--shuffle", "device",
                        "--save_model_secs=0", "--model_dir=" + str(tmp_path / "ck"), "--metrics_jsonl=" + str(mj)],
                       model_defaults=dict(batch_size=128, num_steps=1000, learning_rate=0.1))
    model = ResNetModel(0.1, "resnet20")
    prog, opts, gstep = train.run_allreduce(fl, model, torch.device("cuda:0"), logs.append)
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    return model, prog, opts, gstep, rows, logs


def test_cli_evaluates_and_checkpoints_the_average_and_a_restart_keeps_it(tmp_path):
    model, prog, opts, gstep, rows, logs = _cli(tmp_path, "a", 4)
    assert [r["gs"] for r in rows] == [1, 2, 3, 4]
    assert all(_bits(r["ema_decay"]) == _bits(np.float32(0.9)) for r in rows)
    for r in rows:
        assert (r.get("eval_weights") == "ema") == (r["gs"] in (2, 4)) == ("test_accuracy" in r)
    lines = [l for l in logs if "Test-Accuracy" in l]
    assert [l.split(":")[0] for l in lines] == ["Global step 2 Test-Accuracy(EMA)", "Global step 4 Test-Accuracy(EMA)"]
    assert prog.evaluator.capture_error is None and prog.step_runner.capture_error is None
    # the state as the chief checkpoints it, through a real bundle
    t = train.tensors_from_flat(model, prog.P, opts, int(gstep.item()))
    ckpt.Saver(str(tmp_path / "ck")).save(t, int(gstep.item()))
    saved = ckpt.load_bundle(ckpt.latest_checkpoint(str(tmp_path / "ck")))
    trained = sorted({n for _c, vl, _b in model.opt_groups for n in vl})
    ema_keys = {k for k in saved if k.endswith("/ExponentialMovingAverage")}
    assert ema_keys == {n + "/ExponentialMovingAverage" for n in trained}
    assert not any("moving_mean" in k or "moving_variance" in k for k in ema_keys)
    assert any("moving_mean" in x.name or "moving_variance" in x.name for x in model.specs)
    shadow4 = opts[0].ema.cpu().numpy().copy()
    assert not np.array_equal(shadow4, prog.P.master.cpu().numpy())
    # a second run restores it and trains one more step: its shadow continues the saved one (one mirror
    # update from the masters of step 5) - re-initialised it would have started from the masters of step 4
    _m2, prog2, opts2, gstep2, rows2, _ = _cli(tmp_path, "b", 5)
    assert int(gstep2.item()) == 5 and [r["gs"] for r in rows2] == [5] and rows2[0]["eval_weights"] == "ema"
    d = ops.ema_decay_value(0.9, False, 0)
    got, m5 = opts2[0].ema.cpu().numpy(), prog2.P.master.cpu().numpy()
    for sl in _slices(prog2.P, trained):
        assert np.array_equal(_bits(got[sl]), _bits(ops.ema_update_ref(shadow4[sl], m5[sl], d)))
        assert not np.array_equal(got[sl], m5[sl])
