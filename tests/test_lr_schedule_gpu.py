"""Learning-rate schedules, L2 weight decay and Nesterov momentum inside the fused apply, on the device.
Every comparison is bitwise: the schedule against its numpy-float32 host mirror, the scheduled / decayed
apply against the plain apply given the same rate / the same precomputed gradient, Nesterov against a
numpy-float32 mirror (only + and *, contraction off), a captured replay against eager steps."""
import numpy as np
import pytest
import torch

from dtfe import ops
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig, VarSpec

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
DECAY = ("a3", "a1027", "a8197", "tr")   # a1, a64, a3x8192 do not decay
WD = 0.03125 + 1e-4
KINDS = ["sgd", "momentum", "adam", "rmsprop"]
# warm-up 3, boundaries (2, 5): the rate changes at steps 1, 2, 3 (warm-up, first boundary) and 6
PIECEWISE = dict(lr_boundaries=(2, 5), lr_values=(0.05, 0.02, 0.003), lr_warmup_steps=3)
LINEAR = dict(lr_decay_steps=7, lr_end=0.001)


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


def _cfg(kind, **kw):
    kw.setdefault("lr", 0.05)
    return OptimizerConfig(kind=kind, momentum=0.9 if kind in ("momentum", "rmsprop") else 0.0, **kw)


def _gs():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _opt(P, kind, gs=None, var_list=VAR_LIST, **kw):
    return Optimizer(_cfg(kind, **kw), P, var_list=var_list, global_step=gs)


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


def _assert_outside_untouched(P, init, w16_out0):
    for n in OUTSIDE:  # their gradient is NaN
        o, k = P.offsets[n], P.spec(n).numel
        assert torch.equal(P.master[o:o + k], init[o:o + k])
    assert torch.equal(P.w16["out0"], w16_out0)
    assert torch.isfinite(P.master).all()


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _copies_follow_the_masters(P):
    for n, w in P.w16.items():
        assert torch.equal(w, P.view(n).to(torch.bfloat16)), n
    for n, w in P.wt16.items():
        R, T, C = P.spec(n).transpose
        assert torch.equal(w, P.view(n).reshape(R, T, C).permute(2, 1, 0).reshape(-1).to(torch.bfloat16)), n


# ------------------------------------------------------------- the schedule
@pytest.mark.parametrize("sched", [PIECEWISE, LINEAR, dict(LINEAR, lr_warmup_steps=4)], ids=["piecewise", "linear",
                                                                                             "linear+warmup"])
def test_lr_out_equals_the_host_mirror_bitwise_at_every_step(sched):
    P, gs = _params(), _gs()
    opt = _opt(P, "sgd", gs, **sched)
    g = _fill_grad(P, 5)
    got, want = [], []
    for step in range(13):
        opt.step(grad=g)
        got.append(_bits(opt.current_lr.item()))
        want.append(_bits(ops.lr_schedule_value(opt.lr_spec, step)))
        assert int(gs.item()) == step + 1
    print([float(ops.lr_schedule_value(opt.lr_spec, s)) for s in range(13)])
    assert got == want
    assert len(set(want)) >= 4  # the schedule moves inside these steps


@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_scheduled_apply_equals_unscheduled_apply_with_the_mirror_value_as_host_lr(kind, g16):
    Pa, Pb = _params(), _params()
    init, w16_out0 = Pa.master.clone(), Pa.w16["out0"].clone()
    gsa, gsb = _gs(), _gs()
    a = _opt(Pa, kind, gsa, **PIECEWISE)
    b = _opt(Pb, kind, gsb)
    assert b.lr_spec is None and b.current_lr is None
    for step in range(8):
        g = _fill_grad(Pa, 20 + step, dtype=torch.bfloat16 if g16 else torch.float32)
        kw = dict(grad16=g) if g16 else dict(grad=g)
        a.step(gscale=1.0 / 3.0, **kw)
        b.cfg.lr = float(ops.lr_schedule_value(a.lr_spec, step))
        b.step(gscale=1.0 / 3.0, **kw)
        _assert_same(_state(Pa, a), _state(Pb, b))
    assert int(gsa.item()) == int(gsb.item()) == 8
    _assert_outside_untouched(Pa, init, w16_out0)


def test_a_preset_global_step_applies_that_steps_rate():
    Pa, Pb = _params(), _params()
    gs = torch.full((1,), 6, dtype=torch.int32, device=DEV)  # as a restored checkpoint leaves it
    a = _opt(Pa, "momentum", gs, **PIECEWISE)
    want = ops.lr_schedule_value(a.lr_spec, 6)
    b = _opt(Pb, "momentum", lr=float(want))
    g = _fill_grad(Pa, 7)
    a.step(grad=g)
    b.step(grad=g)
    assert _bits(a.current_lr.item()) == _bits(want) == _bits(np.float32(0.003))
    _assert_same(_state(Pa, a), _state(Pb, b))


# -------------------------------------------------------------- weight decay
def _decayed_grad(P, g, scale=None):
    """g (times the device scalar ``scale``) + (p * wd) on the decaying variables, as two separate
    float32 torch ops (no add(alpha=), which may fuse)."""
    wd = torch.tensor(WD, dtype=torch.float32, device=DEV)
    out = g.clone() if scale is None else g * scale
    for n in DECAY:
        o, k = P.offsets[n], P.spec(n).numel
        t = P.master[o:o + k] * wd
        out[o:o + k] = out[o:o + k] + t
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_decayed_apply_equals_plain_apply_of_the_precomputed_gradient(kind):
    Pa, Pb, Pc = _params(), _params(), _params()
    init, w16_out0 = Pa.master.clone(), Pa.w16["out0"].clone()
    a = _opt(Pa, kind, weight_decay=WD, decay_vars=DECAY)   # fp32 gradient
    b = _opt(Pb, kind)                                      # plain, fed g + p * wd
    c = _opt(Pc, kind, weight_decay=WD, decay_vars=DECAY)   # bf16 gradient
    assert a.decay and not b.decay and [w != 0 for w in a.wd] == [n in DECAY for n in VAR_LIST]
    for step in range(3):
        g16 = _fill_grad(Pa, 30 + step, dtype=torch.bfloat16)
        g = g16.float()
        gb = _decayed_grad(Pb, g)
        a.step(grad=g)
        b.step(grad=gb)
        c.step(grad16=g16)
        _assert_same(_state(Pa, a), _state(Pb, b))
        _assert_same(_state(Pa, a), _state(Pc, c))
    _assert_outside_untouched(Pa, init, w16_out0)
    _copies_follow_the_masters(Pa)


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_the_decay_is_added_after_the_clip_scale(kind):
    Pa, Pb = _params(), _params()
    a = _opt(Pa, kind, weight_decay=WD, decay_vars=DECAY, clip_norm=7.0)
    b = _opt(Pb, kind)
    for step in range(2):
        g = _fill_grad(Pa, 40 + step)
        a.step(grad=g)
        norm, scale = a.clip_out.cpu().tolist()
        assert norm > 7.0 and scale < 1.0  # this test clips; the norm is the gradient's alone
        b.step(grad=_decayed_grad(Pb, g, a.clip_out[1:].clone()))
        _assert_same(_state(Pa, a), _state(Pb, b))


def _raw_state(o, **kw):
    """ops.opt_state over an Optimizer's own tables and tensors, ``kw`` on top."""
    c = o.cfg
    segs, work = o._tables
    args = dict(s1=o.s1, s2=o.s2, beta1=c.beta1, beta2=c.beta2, eps=c.resolved_eps(), momentum=c.momentum, rho=c.rho,
                beta_pow=o.beta_pow, global_step=o.global_step)
    args.update(kw)
    return ops.opt_state(o.kind, o.P.master, segs, work, o.done, **args)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_a_plan_without_decay_is_the_old_plan(kind):
    g = None
    states = []
    for mode in ("optimizer", "no wd", "wd zeros", "wd zeros, decay kernel"):
        P = _params()
        o = _opt(P, kind)
        assert not o.decay and o.lr_spec is None
        g = _fill_grad(P, 50) if g is None else g
        g[P.offsets["a3"]] = -0.0  # a + 0 * p would lose the sign
        if mode == "optimizer":
            o.step(grad=g, gscale=0.5)
        else:
            segs, work = o._tables
            extra = {} if mode == "no wd" else dict(wd=[0.0] * len(segs), decay=mode.endswith("decay kernel"))
            # a state of the optimizer's own tables and tensors, built without the recipe arguments
            ops.apply_gradients(_raw_state(o, **extra), g, None, 0.5, o.cfg.lr, 1)
        states.append(_state(P, o))
    for s in states[1:]:
        _assert_same(states[0], s)


# ------------------------------------------------------------------ Nesterov
def test_nesterov_equals_the_numpy_float32_mirror():
    P = _params()
    lr, m = np.float32(0.05), np.float32(0.9)
    opt = _opt(P, "momentum", nesterov=True)
    v = P.master.cpu().numpy().copy()
    acc = np.zeros_like(v)
    for step in range(3):
        g = _fill_grad(P, 60 + step)
        opt.step(grad=g)
        gh = g.cpu().numpy()
        for n in VAR_LIST:
            sl = slice(P.offsets[n], P.offsets[n] + P.spec(n).numel)
            acc[sl] = acc[sl] * m + gh[sl]                              # a = a m + g
            v[sl] = v[sl] - (gh[sl] * lr + (acc[sl] * m) * lr)          # v -= g lr + (a m) lr
        assert acc.dtype == v.dtype == np.float32
        assert np.array_equal(P.master.cpu().numpy().view(np.int32), v.view(np.int32))
        assert np.array_equal(opt.s1.cpu().numpy().view(np.int32), acc.view(np.int32))
    _copies_follow_the_masters(P)
    # and it is not the plain momentum update
    Pb = _params()
    b = _opt(Pb, "momentum")
    b.step(grad=_fill_grad(Pb, 60))
    assert not torch.equal(Pb.master, P.master)


def test_nesterov_is_refused_for_other_kinds():
    with pytest.raises(ValueError, match="nesterov"):
        _opt(_params(), "adam", nesterov=True)
    P = _params()
    o = _opt(P, "sgd")
    with pytest.raises(RuntimeError, match="nesterov"):
        _raw_state(o, nesterov=True)


# ------------------------------------------------------------ captured replay
RECIPE = dict(weight_decay=WD, decay_vars=DECAY, **PIECEWISE)


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_a_graph_of_four_steps_replayed_three_times_equals_twelve_eager_steps(kind):
    extra = dict(nesterov=True) if kind == "momentum" else {}
    Pa, Pb = _params(), _params()
    gsa, gsb = _gs(), _gs()
    a = _opt(Pa, kind, gsa, **RECIPE, **extra)
    b = _opt(Pb, kind, gsb, **RECIPE, **extra)
    g = _fill_grad(Pa, 70)
    Pa.grad.copy_(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture; its update is undone below
        a.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(4):
            a.step()
    # back to b's (fresh) state: the warm-up and the capture itself must not count
    Pa.master.copy_(Pb.master); a.s1.copy_(b.s1); gsa.copy_(gsb); a.current_lr.copy_(b.current_lr)
    if a.s2 is not None:
        a.s2.copy_(b.s2); a.beta_pow.copy_(b.beta_pow)
    Pa.refresh_copies()
    for rep in range(3):
        graph.replay()
        for _ in range(4):
            b.step(grad=g)
        _assert_same(_state(Pa, a), _state(Pb, b))
        assert int(gsa.item()) == int(gsb.item()) == 4 * (rep + 1)
        # the rate of the replay's last step: the boundaries (steps 2 and 5) lie inside replays 1 and 2
        want = ops.lr_schedule_value(a.lr_spec, 4 * rep + 3)
        assert _bits(a.current_lr.item()) == _bits(b.current_lr.item()) == _bits(want)
    assert _bits(a.current_lr.item()) == _bits(np.float32(0.003))


# ------------------------------------------------------------------- grouped
def test_step_all_over_two_scheduled_optimizers_equals_the_two_steps_in_order():
    la, lb = ["a1", "a64", "a8197", "tr"], ["a3", "a1027", "a3x8192", "out1"]
    Pa, Pb = _params(), _params()
    g = _fill_grad(Pa, 80, names=la + lb)
    gsa, gsb = _gs(), _gs()
    mk = lambda P, gs: [_opt(P, "adam", gs, var_list=vl, lr=lr, weight_decay=WD, decay_vars=dv, **PIECEWISE)
                        for vl, lr, dv in ((la, 0.05, ("tr",)), (lb, 0.01, ("a1027",)))]
    oa, ob = mk(Pa, gsa), mk(Pb, gsb)
    for step in range(4):
        Optimizer.step_all(oa, [0, 2], grad=g)
        for o, inc in zip(ob, [0, 2]):
            o.step(grad=g, gs_inc=inc)
        for x, y in zip(oa, ob):
            _assert_same(_state(Pa, x), _state(Pb, y))
            # both optimizers of a step saw the step it began with: the second did not run ahead
            assert _bits(x.current_lr.item()) == _bits(y.current_lr.item()) \
                == _bits(ops.lr_schedule_value(x.lr_spec, 2 * step))
    assert int(gsa.item()) == int(gsb.item()) == 8


def test_the_grouped_launch_decays_each_optimizers_own_segments():
    la, lb = ["a1", "a64", "a8197", "tr"], ["a3", "a1027", "a3x8192", "out1"]
    Pa, Pb = _params(), _params()
    g = _fill_grad(Pa, 81, names=la + lb)
    mk = lambda P: [_opt(P, "adam", var_list=la, weight_decay=WD, decay_vars=("tr", "a64")),
                    _opt(P, "adam", var_list=lb)]  # one launch, the second optimizer without decay
    oa, ob = mk(Pa), mk(Pb)
    for _ in range(2):
        Optimizer.step_all(oa, [0, 0], grad=g)
        for o in ob:
            o.step(grad=g, gs_inc=0)
        for x, y in zip(oa, ob):
            _assert_same(_state(Pa, x), _state(Pb, y))
    with pytest.raises(RuntimeError, match="schedule"):  # the op itself refuses a schedule in a group
        sched = ops.lr_schedule_pack(ops.lr_schedule_spec(0.1, warmup_steps=2), Pa.master)
        gs = _gs()
        ops.require().apply_gradients_group(
            [_raw_state(oa[0], global_step=gs, sched=sched), _raw_state(oa[1], global_step=gs)], g, None, 1.0,
            [o.cfg.lr for o in oa], [0, 1])


# ------------------------------------------------- next to --clip_norm / wait=
def test_clip_norm_keeps_working_next_to_a_schedule():
    Pa, Pb = _params(), _params()
    gsa, gsb = _gs(), _gs()
    a = _opt(Pa, "adam", gsa, clip_norm=7.0, **PIECEWISE)
    b = _opt(Pb, "adam", gsb, clip_norm=7.0)
    for step in range(4):
        g = _fill_grad(Pa, 90 + step)
        a.step(grad=g)
        b.cfg.lr = float(ops.lr_schedule_value(a.lr_spec, step))
        b.step(grad=g)
        assert float(a.clip_out[1].item()) < 1.0
        assert torch.equal(a.clip_out, b.clip_out)
        _assert_same(_state(Pa, a), _state(Pb, b))


def test_wait_keeps_working_next_to_a_schedule():
    Pa, Pb = _params(), _params()
    gsa, gsb = _gs(), _gs()
    a = _opt(Pa, "momentum", gsa, **RECIPE)
    b = _opt(Pb, "momentum", gsb, **RECIPE)
    done, seen = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    for step in range(3):
        g = _fill_grad(Pa, 95 + step)
        ops.epoch_signal(done)  # the producer has finished: the waiting items go ahead at once
        a.step(grad=g, wait=(done, seen, ["a3", "tr"]))
        b.step(grad=g)
        _assert_same(_state(Pa, a), _state(Pb, b))
        assert _bits(a.current_lr.item()) == _bits(ops.lr_schedule_value(a.lr_spec, step))
    assert int(seen.item()) == int(done.item()) == 3
