"""Global-norm gradient clipping on the device: the norm kernel (grad_sumsq), its scale, and the fused
apply reading that scale - against float64 host arithmetic and, bitwise, against the unclipped apply
given the same scale as a host float."""
import dataclasses
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dtfe import ops
from dtfe.models.gan import GanModel
from dtfe.models.lstm import LstmModel
from dtfe.optim import FlatParams, GlobalNormClip, Optimizer, OptimizerConfig, VarSpec

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _init(shape, g):
    return torch.randn(*shape, generator=g)


# every path of both kernels: single elements, a vector body with a tail, a second chunk of 5 elements,
# exact chunks, the transposed-tile path with both bf16 copies - and two variables NOT in the var list
SPECS = [
    VarSpec("a1", (1,), _init),
    VarSpec("out0", (100,), _init, bf16=True),            # not in the var list
    VarSpec("a3", (3,), _init),
    VarSpec("a64", (64,), _init, bf16=True),
    VarSpec("a1027", (1027,), _init),
    VarSpec("a8197", (8192 + 5,), _init, bf16=True),
    VarSpec("a3x8192", (3 * 8192,), _init),
    VarSpec("tr", (70, 130), _init, bf16=True, transpose=(70, 1, 130)),
    VarSpec("out1", (5000,), _init),                       # not in the var list
]
VAR_LIST = ["a1", "a3", "a64", "a1027", "a8197", "a3x8192", "tr"]
OUTSIDE = ["out0", "out1"]


def _params(seed=3):
    return FlatParams(SPECS, DEV, seed=seed)


def _fill_grad(P, seed, names=VAR_LIST, std=1.0, dtype=torch.float32):
    """A full-size gradient: NaN everywhere (padding and foreign variables included), seeded normal
    values in the given variables only."""
    g = torch.full((P.total,), float("nan"), dtype=torch.float32)
    gen = torch.Generator().manual_seed(seed)
    for n in names:
        o, k = P.offsets[n], P.spec(n).numel
        g[o:o + k] = torch.randn(k, generator=gen) * std
    return g.to(dtype).to(DEV)


def _host_norm(P, g, gscale, names=VAR_LIST):
    x = torch.cat([g[P.offsets[n]:P.offsets[n] + P.spec(n).numel] for n in names]).cpu().double()
    return math.sqrt(float(((x * float(np.float32(gscale))) ** 2).sum()))


def _clip(P, c=1.0, names=VAR_LIST):
    return GlobalNormClip(P, names, c)


# ------------------------------------------------------------------- norm
@pytest.mark.parametrize("g16,gscale", [(False, 1.0), (True, 0.125)])
def test_norm_matches_float64_and_reads_only_the_var_list(g16, gscale):
    P = _params()
    g = _fill_grad(P, 11, dtype=torch.bfloat16 if g16 else torch.float32)
    clip = _clip(P, 1.0)
    clip.compute(None if g16 else g, g if g16 else None, gscale)
    out = clip.out.cpu()
    ref = _host_norm(P, g, gscale)
    print("norm", float(out[0]), "ref", ref, "rel", abs(float(out[0]) - ref) / ref)
    assert torch.isfinite(out).all(), out  # neither padding nor a foreign variable was read
    assert abs(float(out[0]) - ref) <= 1e-5 * ref


def test_plan_covers_exactly_the_var_list():
    P = _params()
    plan = ops.grad_norm_plan([(P.offsets[n], P.spec(n).numel) for n in VAR_LIST], P.master).cpu()
    assert int(plan[:, 1].max()) <= 8192
    seen = torch.zeros(P.total, dtype=torch.int32)
    for o, n in plan.tolist():
        seen[o:o + n] += 1
    want = torch.zeros(P.total, dtype=torch.int32)
    for n in VAR_LIST:
        want[P.offsets[n]:P.offsets[n] + P.spec(n).numel] = 1
    assert torch.equal(seen, want)


def test_norm_is_bitwise_reproducible_whatever_the_grid():
    P = _params()
    g = _fill_grad(P, 12)
    clip = _clip(P, 0.5)
    outs = []
    for _ in range(3):
        clip.compute(g)
        outs.append(clip.out.clone())
    clip.compute(g, max_blocks=1)
    outs.append(clip.out.clone())
    clip.compute(g, max_blocks=3)
    outs.append(clip.out.clone())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), (outs[0], o)
    assert int(clip.ticket.item()) == 0  # the ticket reset itself


def test_scale_values():
    P = _params()
    g = _fill_grad(P, 13)
    probe = _clip(P, 1.0)
    probe.compute(g)
    norm = np.float32(probe.out[0].item())
    c = np.float32(norm / np.float32(3))
    clip = _clip(P, float(c))
    clip.compute(g)
    got = np.float32(clip.out[1].item())
    want = c / norm  # the fp32 division
    assert abs(got - want) <= np.spacing(want), (got, want)
    assert np.float32(clip.out[0].item()) == norm
    clip = _clip(P, float(2 * norm))
    clip.compute(g)
    assert float(clip.out[1].item()) == 1.0
    z = torch.zeros(P.total, device=DEV)
    clip.compute(z)
    assert clip.out.cpu().tolist() == [0.0, 1.0]


def test_scale_multiplies_exactly_the_var_list_in_place():
    P = _params()
    g = _fill_grad(P, 14)
    clip = _clip(P, 2.0)
    clip.compute(g)
    scale = clip.out[1:].clone()
    want = g.clone()
    for n in VAR_LIST:
        o, k = P.offsets[n], P.spec(n).numel
        want[o:o + k] *= scale
    clip.scale_grad(g)
    assert torch.equal(torch.nan_to_num(g, nan=-7.0), torch.nan_to_num(want, nan=-7.0))  # the rest still NaN
    clip.compute(g)  # the clipped gradient's norm is clip_norm
    assert abs(float(clip.norm.item()) - 2.0) <= 1e-5 * 2.0 and float(scale) < 1.0


# ------------------------------------------------------------------ apply
def _cfg(kind, **kw):
    return OptimizerConfig(kind=kind, lr=0.05, momentum=0.9 if kind in ("momentum", "rmsprop") else 0.0, **kw)


def _state(P, opt):
    t = {"master": P.master, "s1": opt.s1, "s2": opt.s2}
    t.update({"w16/" + k: v for k, v in P.w16.items()})
    t.update({"wt16/" + k: v for k, v in P.wt16.items()})
    return {k: v.clone() for k, v in t.items() if v is not None}


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam", "rmsprop"])
def test_clipped_apply_equals_unclipped_apply_with_the_scale_as_host_float(kind, g16):
    gscale = 1.0 / 3.0
    Pa, Pb = _params(), _params()
    init = Pa.master.clone()
    w16_out0 = Pa.w16["out0"].clone()
    gsa = torch.zeros(1, dtype=torch.int32, device=DEV)
    gsb = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = Optimizer(_cfg(kind, clip_norm=7.0), Pa, var_list=VAR_LIST, global_step=gsa)
    b = Optimizer(_cfg(kind), Pb, var_list=VAR_LIST, global_step=gsb)
    assert b.clip is None
    for step in range(2):  # the second step runs on non-trivial slots
        g = _fill_grad(Pa, 20 + step, dtype=torch.bfloat16 if g16 else torch.float32)
        kw = dict(grad16=g) if g16 else dict(grad=g)
        a.step(gscale=gscale, **kw)
        norm, scale = a.clip_out.cpu().tolist()
        assert norm > 7.0 and scale < 1.0  # this test clips
        b.step(gscale=float(np.float32(gscale) * np.float32(scale)), **kw)
        _assert_same(_state(Pa, a), _state(Pb, b))
    assert int(gsa.item()) == int(gsb.item()) == 2
    for n in OUTSIDE:  # untouched (their gradient is NaN)
        o, k = Pa.offsets[n], Pa.spec(n).numel
        assert torch.equal(Pa.master[o:o + k], init[o:o + k])
    assert torch.equal(Pa.w16["out0"], w16_out0)
    assert torch.isfinite(Pa.master).all()


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_clip_norm_zero_is_the_unclipped_optimizer(kind):
    Pa, Pb, Pc = _params(), _params(), _params()
    a = Optimizer(_cfg(kind, clip_norm=0.0), Pa, var_list=VAR_LIST)
    b = Optimizer(_cfg(kind), Pb, var_list=VAR_LIST)
    c = Optimizer(_cfg(kind), Pc, var_list=VAR_LIST)
    assert a.clip is None and a.global_norm is None and a.clip_out is None  # no plan, no norm launch
    g = _fill_grad(Pa, 30)
    a.step(grad=g, gscale=0.5)
    b.step(grad=g, gscale=0.5)
    # the op called without a clip_scale argument
    ops.apply_gradients(c._state, g, None, 0.5, c.cfg.lr, 1)
    _assert_same(_state(Pa, a), _state(Pb, b))
    _assert_same(_state(Pa, a), _state(Pc, c))


def test_grouped_apply_clips_each_var_list_by_its_own_norm():
    la, lb = ["a1", "a64", "a8197", "tr"], ["a3", "a1027", "a3x8192", "out1"]
    Pa, Pb = _params(), _params()
    g = _fill_grad(Pa, 40, names=la + lb)
    gsa = torch.zeros(1, dtype=torch.int32, device=DEV)
    gsb = torch.zeros(1, dtype=torch.int32, device=DEV)
    oa = [Optimizer(_cfg("adam", clip_norm=c), Pa, var_list=vl, global_step=gsa) for c, vl in ((5.0, la), (1e6, lb))]
    ob = [Optimizer(_cfg("adam", clip_norm=c), Pb, var_list=vl, global_step=gsb) for c, vl in ((5.0, la), (1e6, lb))]
    Optimizer.step_all(oa, [0, 2], grad=g, gscale=0.5)
    for o, inc in zip(ob, [0, 2]):
        o.step(grad=g, gscale=0.5, gs_inc=inc)
    for x, y in zip(oa, ob):
        _assert_same(_state(Pa, x), _state(Pb, y))
        assert torch.equal(x.clip_out, y.clip_out)
    assert int(gsa.item()) == int(gsb.item()) == 2
    for o, vl in zip(oa, (la, lb)):
        ref = _host_norm(Pa, g, 0.5, vl)
        assert abs(float(o.global_norm.item()) - ref) <= 1e-5 * ref
    assert float(oa[0].clip_out[1].item()) < 1.0 and float(oa[1].clip_out[1].item()) == 1.0


def test_norm_and_apply_replay_in_one_graph():
    Pa, Pb = _params(), _params()
    c = 60.0
    a = Optimizer(_cfg("adam", clip_norm=c), Pa, var_list=VAR_LIST)
    b = Optimizer(_cfg("adam", clip_norm=c), Pb, var_list=VAR_LIST)
    grads = [_fill_grad(Pa, 50, std=1.0), _fill_grad(Pa, 51, std=0.01), _fill_grad(Pa, 52, std=0.0)]
    Pa.grad.copy_(grads[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture; its update is undone below
        a.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.step()
    # back to b's (fresh) state: the warm-up and the capture itself must not count
    Pa.master.copy_(Pb.master); a.s1.copy_(b.s1); a.s2.copy_(b.s2); a.beta_pow.copy_(b.beta_pow)
    Pa.refresh_copies()
    clipped = []
    for g in grads:
        Pa.grad.copy_(g)
        graph.replay()
        b.step(grad=g)
        _assert_same(_state(Pa, a), _state(Pb, b))
        ref = _host_norm(Pa, g, 1.0)
        norm, scale = a.clip_out.cpu().tolist()
        assert abs(norm - ref) <= 1e-5 * ref
        if ref <= 0.99 * c:
            assert scale == 1.0
        else:
            assert abs(scale - c / ref) <= 1e-5 * c / ref
        clipped.append(scale < 1.0)
    assert clipped == [True, False, False] and float(a.global_norm.item()) == 0.0  # clipped, not clipped, zero


# ----------------------------------------------------------------- models
def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_lstm_program_clipped_gpu_matches_cpu():
    torch.manual_seed(0)
    B = 8
    model = LstmModel()
    cpu, gpu = model.program("cpu", B, seed=7), model.program(DEV, B, seed=7)
    batches = [(torch.rand(B, 784), F.one_hot(torch.randint(0, 10, (B,)), 10).float()) for _ in range(3)]
    cpu.load_batch(batches[0])
    cpu.compute_grads()
    names = model.opt_groups[0][1]
    c = 0.5 * _host_norm(cpu.P, cpu.P.grad, 1.0, names)  # half the first step's unclipped norm
    cfg = dataclasses.replace(model.opt_groups[0][0], clip_norm=c)
    oc, og = Optimizer(cfg, cpu.P, var_list=names), Optimizer(cfg, gpu.P, var_list=names)
    for i, batch in enumerate(batches):
        cpu.load_batch(batch)
        gpu.load_batch(tuple(t.cuda() for t in batch))
        cpu.compute_grads()
        gpu.compute_grads()
        ref_gpu = _host_norm(gpu.P, gpu.P.grad, 1.0, names)
        oc.step()
        og.step()
        if i == 0:
            ng, nc = float(og.global_norm.item()), float(oc.global_norm.item())
            print("global_norm gpu", ng, "f64 of the gpu gradient", ref_gpu, "cpu program", nc)
            # the kernel against float64 over the very same gradient: the norm kernel's own bound
            assert abs(ng - ref_gpu) <= 1e-5 * ref_gpu
            # and against the CPU path of the same program
            assert abs(ng - nc) <= 1e-5 * nc
            assert abs(float(og.clip_out[1].item()) - 0.5) < 1e-3 and float(oc.clip_out[1].item()) < 1.0
    for s in model.specs:  # the tolerance tests/test_models_gpu.py uses for this model
        rel = _rel(gpu.P.view(s.name).cpu(), cpu.P.view(s.name))
        print(s.name, "param rel", rel)
        assert rel < 1e-4, (s.name, rel)


def test_gan_program_two_clips_gpu_matches_cpu():
    torch.manual_seed(1)
    B = 64
    model = GanModel()
    cpu, gpu = model.program("cpu", B, seed=7), model.program(DEV, B, seed=7)
    x = torch.rand(B, 784)
    gpu.load_batch(x.cuda())
    cpu.load_batch(x)
    cpu.z.copy_(gpu.z.cpu())  # same noise (device RNG vs host RNG)
    cpu.compute_grads()
    gpu.compute_grads()
    gsc, gsg = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32, device=DEV)
    oc, og = [], []
    for cfg, names, bp in model.opt_groups:
        c = 0.5 * _host_norm(cpu.P, cpu.P.grad, 1.0, names)
        cfg = dataclasses.replace(cfg, clip_norm=c)
        oc.append(Optimizer(cfg, cpu.P, var_list=names, global_step=gsc, beta_power_names=bp))
        og.append(Optimizer(cfg, gpu.P, var_list=names, global_step=gsg, beta_power_names=bp))
    refs = [_host_norm(gpu.P, gpu.P.grad, 1.0, names) for _cfg_, names, _bp in model.opt_groups]
    incs = [0, model.gs_increments]
    Optimizer.step_all(oc, incs)
    Optimizer.step_all(og, incs)
    assert int(gsg.item()) == 2 and int(gsc.item()) == 2
    for o_c, o_g, ref in zip(oc, og, refs):
        ng, nc = float(o_g.global_norm.item()), float(o_c.global_norm.item())
        print("global_norm gpu", ng, "f64 of the gpu gradient", ref, "cpu program", nc)
        assert abs(ng - ref) <= 1e-5 * ref
        assert abs(ng - nc) <= 1e-5 * nc
        assert float(o_g.clip_out[1].item()) < 1.0
    for s in model.specs:
        rel = _rel(gpu.P.view(s.name).cpu(), cpu.P.view(s.name))
        print(s.name, "param rel", rel)
        assert rel < 1e-4, (s.name, rel)
