"""Layer-wise adaptive rate scaling on the device: the per-variable norm kernel (layer_trust) against float64
host arithmetic, its trust ratios bit for bit against the numpy-float32 mirror, and the fused apply reading
them - bitwise against a plain momentum apply per variable that is given lr * trust as a host float."""
import json

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.models.resnet import ResNetModel
from dtfe.optim import FlatParams, LayerTrust, Optimizer, OptimizerConfig, VarSpec
from dtfe.utils import flags as flagmod

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _init(shape, g):
    return torch.randn(*shape, generator=g)


# the clip tests' variable set (every path of both kernels: single elements, a vector body with a tail, a
# second chunk of 5 elements, exact chunks, the transposed-tile path with both bf16 copies, two variables NOT
# in the var list) plus one in-list variable LARS skips, one adaptive variable whose master is all zeros and
# one whose gradient is, and one long enough for every path of the fold
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
ONES = ["skip", "zw", "zg"]                                # a trust of exactly 1 at the first step
DECAY = ["a64", "a8197", "tr", "zw", "skip"]
OUTSIDE = ["out0", "out1"]
WD = 0.01
# 0: the plan's own choice (8192: the kernel's eight loads per thread in flight); 1024: one load, many chunks to fold
CHUNKS = [0, 1024]


def _params(seed=3):
    return FlatParams(SPECS, DEV, seed=seed)


def _fill_grad(P, seed, std=1.0, dtype=torch.float32):
    """A full-size gradient: NaN everywhere (padding and foreign variables included), seeded normal values
    in the var list's variables only, zeros in zg."""
    g = torch.full((P.total,), float("nan"), dtype=torch.float32)
    gen = torch.Generator().manual_seed(seed)
    for n in VAR_LIST:
        o, k = P.offsets[n], P.spec(n).numel
        g[o:o + k] = 0.0 if n == "zg" else torch.randn(k, generator=gen) * std
    return g.to(dtype).to(DEV)


def _sl(P, n):
    return slice(P.offsets[n], P.offsets[n] + P.spec(n).numel)


def _wd(names=DECAY, wd=WD):
    return [wd if n in names else 0.0 for n in VAR_LIST]


def _lt(P, wd=None, eeta=0.02, eps=0.0, chunk=0):
    return LayerTrust(P, VAR_LIST, ADAPTIVE, wd if wd is not None else [0.0] * len(VAR_LIST), eeta, eps, chunk)


def _host_norms(P, g, gscale, n):
    w = P.master[_sl(P, n)].cpu().double()
    x = g[_sl(P, n)].cpu().double() * float(np.float32(gscale))
    return float((w * w).sum().sqrt()), float((x * x).sum().sqrt())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("chunk", CHUNKS)
def test_plan_covers_exactly_the_adaptive_variables(chunk):
    P = _params()
    lt = _lt(P, chunk=chunk)
    plan, ranges = lt.plan.cpu().tolist(), lt.ranges.cpu().tolist()
    assert max(c for _s, _o, c in plan) == (chunk or 8192)
    seen = torch.zeros(P.total, dtype=torch.int32)
    for seg, o, c in plan:
        assert _sl(P, VAR_LIST[seg]).start <= o and o + c <= _sl(P, VAR_LIST[seg]).stop
        seen[o:o + c] += 1
    want = torch.zeros(P.total, dtype=torch.int32)
    for n in ADAPTIVE:
        want[_sl(P, n)] = 1
    assert torch.equal(seen, want)
    assert [s for s, _f, _n in ranges] == [VAR_LIST.index(n) for n in ADAPTIVE]
    for seg, first, n in ranges:  # a variable's chunks are consecutive, in element order
        rows = plan[first:first + n]
        assert all(r[0] == seg for r in rows) and sum(r[2] for r in rows) == P.spec(VAR_LIST[seg]).numel
        assert [r[1] for r in rows] == sorted(r[1] for r in rows)
    assert lt.limit == max(o + c for _s, o, c in plan)


# ----------------------------------------------------------------- norms
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("g16,gscale", [(False, 1.0), (True, 0.125)])
def test_norms_match_float64_and_read_only_the_adaptive_variables(g16, gscale, chunk):
    P = _params()
    g = _fill_grad(P, 11, dtype=torch.bfloat16 if g16 else torch.float32)
    g[_sl(P, "skip")] = float("nan")  # a variable LARS skips is not read either
    lt = _lt(P, chunk=chunk)
    lt.compute(None if g16 else g, g if g16 else None, gscale)
    sums, trust = lt.sums.cpu(), lt.trust.cpu()
    assert torch.isfinite(sums).all() and torch.isfinite(trust).all(), (sums, trust)
    for i, n in enumerate(VAR_LIST):
        if n == "skip":
            assert sums[i].tolist() == [0.0, 0.0]
            continue
        wn, gn = _host_norms(P, g, gscale, n)
        got_w, got_g = float(sums[i, 0].sqrt()), float(sums[i, 1].sqrt())
        print(n, "w", got_w, wn, "g", got_g, gn)
        assert abs(got_w - wn) <= 1e-5 * wn and abs(got_g - gn) <= 1e-5 * gn
    assert float(sums[VAR_LIST.index("zw"), 0]) == 0.0 and float(sums[VAR_LIST.index("zg"), 1]) == 0.0


# ----------------------------------------------------------------- trust
@pytest.mark.parametrize("clip,wd,eps", [(None, 0.0, 0.0), (0.37, WD, 0.0), (None, 0.0, 1e-3), (0.37, WD, 1e-3),
                                         (None, WD, 0.0)])
def test_trust_equals_the_mirror_of_the_device_sums(clip, wd, eps):
    P = _params()
    g = _fill_grad(P, 12)
    eeta, gscale = 0.02, 1.0 / 3.0
    wds = _wd(wd=wd)
    lt = _lt(P, wds, eeta, eps)
    cs = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=DEV)
    lt.compute(g, None, gscale, clip_scale=cs)
    sums, trust = lt.sums.cpu().numpy(), lt.trust.cpu().numpy()
    for i, n in enumerate(VAR_LIST):
        if n in ONES:
            assert trust[i].view(np.int32) == np.float32(1).view(np.int32), (n, trust[i])
            continue
        want = ops.lars_trust_ref(sums[i, 0], sums[i, 1], eeta, np.float32(wds[i]), eps,
                                  None if clip is None else np.float32(clip))
        assert trust[i].view(np.int32) == want.view(np.int32), (n, trust[i], want)
        # and against float64 from the raw arrays: two norms at 1e-5 each plus the quotient's roundings
        wn, gn = _host_norms(P, g, gscale, n)
        if clip is not None:
            gn *= float(np.float32(clip))
        ref = float(np.float32(eeta)) * wn / (gn + float(np.float32(wds[i])) * wn + float(np.float32(eps)))
        print(n, "trust", float(trust[i]), "f64", ref, "rel", abs(float(trust[i]) - ref) / ref)
        assert abs(float(trust[i]) - ref) <= 3e-5 * ref


# ------------------------------------------------------ grid independence
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("g16", [False, True])
def test_sums_and_trust_are_bitwise_reproducible_whatever_the_grid(g16, chunk):
    P = _params()
    g = _fill_grad(P, 13, dtype=torch.bfloat16 if g16 else torch.float32)
    lt = _lt(P, _wd(), 0.02, 1e-6, chunk)
    kw = dict(grad16=g) if g16 else dict(grad=g)
    outs = []
    for mb in (0, 0, 0, 1, 3):
        lt.sums.fill_(-1.0)
        lt.trust[lt.index] = -1.0
        lt.compute(gscale=0.5, max_blocks=mb, **kw)
        outs.append((lt.sums.clone(), lt.trust.clone()))
        assert int(lt.ticket.item()) == 0  # the ticket reset itself
    for s, t in outs[1:]:
        assert torch.equal(_bits(s), _bits(outs[0][0])) and torch.equal(_bits(t), _bits(outs[0][1]))
    assert float(outs[0][1][VAR_LIST.index("skip")]) == 1.0  # written at setup, never by a launch


# ------------------------------------------------------------------ apply
LR = 0.05


def _cfg(**kw):
    return OptimizerConfig(kind="momentum", lr=LR, momentum=0.9, **kw)


def _lars_cfg(**kw):
    return _cfg(weight_decay=WD, decay_vars=tuple(DECAY), lars_eeta=0.02, lars_epsilon=1e-6, lars_vars=tuple(ADAPTIVE),
                **kw)


def _var_state(P, opt, n):
    t = {"master": P.master[_sl(P, n)], "s1": opt.s1[_sl(P, n)], "w16": P.w16.get(n), "wt16": P.wt16.get(n),
         "ema": None if opt.ema is None else opt.ema[_sl(P, n)]}
    return {k: v.clone() for k, v in t.items() if v is not None}


@pytest.mark.parametrize("case", ["momentum", "nesterov", "schedule", "ema", "clip_g16"])
def test_lars_apply_equals_plain_apply_per_variable_with_lr_times_trust(case):
    f = np.float32
    extra = {"nesterov": dict(nesterov=True), "schedule": dict(lr_boundaries=(0,), lr_values=(LR, 0.02)),
             "ema": dict(ema_decay=0.9), "clip_g16": dict(clip_norm=7.0)}.get(case, {})
    g16 = case == "clip_g16"
    gscale = 1.0 / 3.0
    P = _params()
    init, w16_out0 = P.master.clone(), P.w16["out0"].clone()
    gs = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = Optimizer(_lars_cfg(**extra), P, var_list=VAR_LIST, global_step=gs)
    assert a.layer_trust is a.lars.trust and a.layer_trust.shape == (len(VAR_LIST),)
    grads = [_fill_grad(P, 20 + s, dtype=torch.bfloat16 if g16 else torch.float32) for s in range(2)]
    trusts, scales = [], []
    for s, g in enumerate(grads):
        a.step(gscale=gscale, **(dict(grad16=g) if g16 else dict(grad=g)))
        trusts.append(a.layer_trust.cpu().numpy().copy())
        scales.append(f(a.clip_out[1].item()) if a.clip is not None else None)
        if case == "schedule":  # lr_out reports the schedule's rate, not a variable's
            assert f(a.current_lr.item()) == f(extra["lr_values"][s])
    assert int(gs.item()) == 2 and a.lars.launches == 2
    assert trusts[0][VAR_LIST.index("zw")] == 1.0 and trusts[1][VAR_LIST.index("zw")] != 1.0  # zeros, then not
    assert all(t[VAR_LIST.index(n)] == 1.0 for t in trusts for n in ("skip", "zg"))
    if case == "clip_g16":
        assert scales[0] < 1.0  # this case clips
    for i, n in enumerate(VAR_LIST):
        Pv = _params()
        gsv = torch.zeros(1, dtype=torch.int32, device=DEV)
        plain = {k: v for k, v in extra.items() if k in ("nesterov", "ema_decay")}
        b = Optimizer(_cfg(weight_decay=WD if n in DECAY else 0.0, **plain), Pv, var_list=[n], global_step=gsv)
        assert b.lars is None
        for s, g in enumerate(grads):
            rate = f(extra["lr_values"][s]) if case == "schedule" else f(LR)
            b.cfg.lr = float(rate * f(trusts[s][i]))
            # the clip's scale as a host float in gscale: the unclipped apply the clip tests compare with
            gsc = gscale if scales[s] is None else float(f(gscale) * scales[s])
            b.step(gscale=gsc, **(dict(grad16=g) if g16 else dict(grad=g)))
        sa, sb = _var_state(P, a, n), _var_state(Pv, b, n)
        assert sa.keys() == sb.keys()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (case, n, k)
    for n in OUTSIDE:  # untouched (their gradient is NaN)
        assert torch.equal(P.master[_sl(P, n)], init[_sl(P, n)])
    assert torch.equal(P.w16["out0"], w16_out0)
    assert torch.isfinite(P.master).all()


def test_off_is_off(monkeypatch):
    Pa, Pb = _params(), _params()
    a = Optimizer(_cfg(weight_decay=WD, decay_vars=tuple(DECAY), lars_eeta=0.0, lars_epsilon=0.0, lars_vars=tuple(ADAPTIVE)),
                  Pa, var_list=VAR_LIST)
    b = Optimizer(_cfg(weight_decay=WD, decay_vars=tuple(DECAY)), Pb, var_list=VAR_LIST)
    assert a.lars is None and a.layer_trust is None and b.layer_trust is None

    def no_launch(*_a, **_k):
        raise AssertionError("a trust launch without lars_eeta")
    monkeypatch.setattr(ops, "layer_trust", no_launch)
    for s in range(2):
        g = _fill_grad(Pa, 30 + s)
        a.step(grad=g, gscale=0.5)
        b.step(grad=g, gscale=0.5)
    assert torch.equal(_bits(Pa.master), _bits(Pb.master)) and torch.equal(a.s1, b.s1)
    for k in Pa.w16:
        assert torch.equal(Pa.w16[k], Pb.w16[k])
    assert torch.equal(Pa.wt16["tr"], Pb.wt16["tr"])


def test_refusals():
    P = _params()
    with pytest.raises(ValueError, match="momentum"):
        Optimizer(OptimizerConfig(kind="adam", lars_eeta=0.01), P, var_list=VAR_LIST)
    with pytest.raises(ValueError, match="lars_vars"):
        Optimizer(_cfg(lars_eeta=0.01, lars_vars=("out0",)), P, var_list=VAR_LIST)
    a = Optimizer(_lars_cfg(), P, var_list=VAR_LIST)
    done, seen = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    with pytest.raises(ValueError, match="wait="):
        a.step(grad=_fill_grad(P, 1), wait=(done, seen, ["a1"]))
    # the native side: a per-segment rate is the momentum optimizer's
    segs, work = a._tables
    with pytest.raises(RuntimeError, match="seg_lr"):
        ops.opt_state(ops.OPT_SGD, P.master, segs, work, torch.zeros(1, dtype=torch.int32, device=DEV),
                      seg_lr=a.layer_trust)
    with pytest.raises(RuntimeError, match="seg_lr"):
        ops.opt_state(ops.OPT_MOMENTUM, P.master, segs, work, torch.zeros(1, dtype=torch.int32, device=DEV), s1=a.s1,
                      momentum=0.9, seg_lr=a.layer_trust[:-1].clone())


def test_step_all_sends_lars_down_the_sequential_path():
    la, lb = ["a1", "a64", "a8197", "tr"], ["a3", "a1027", "a3x8192", "skip", "zw", "zg"]
    Pa, Pb = _params(), _params()
    g = _fill_grad(Pa, 40)

    def pair(P, gs):
        return [Optimizer(_cfg(lars_eeta=0.02, lars_vars=tuple(n for n in vl if n != "skip")), P, var_list=vl, global_step=gs)
                for vl in (la, lb)]
    gsa, gsb = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    oa, ob = pair(Pa, gsa), pair(Pb, gsb)
    Optimizer.step_all(oa, [0, 1], grad=g, gscale=0.5)
    for o, inc in zip(ob, [0, 1]):
        o.step(grad=g, gscale=0.5, gs_inc=inc)
    assert torch.equal(_bits(Pa.master), _bits(Pb.master)) and int(gsa.item()) == int(gsb.item()) == 1
    for x, y in zip(oa, ob):
        assert torch.equal(_bits(x.layer_trust), _bits(y.layer_trust)) and torch.equal(x.s1, y.s1)
        assert bool((x.layer_trust != 1).any())


# ---------------------------------------------------------------- capture
def test_two_steps_in_one_graph_equal_two_eager_steps():
    Pa, Pb = _params(), _params()
    a = Optimizer(_lars_cfg(clip_norm=7.0, nesterov=True), Pa, var_list=VAR_LIST)
    b = Optimizer(_lars_cfg(clip_norm=7.0, nesterov=True), Pb, var_list=VAR_LIST)
    grads = [_fill_grad(Pa, 50), _fill_grad(Pa, 51, std=0.01)]

    def two_steps():
        for g in grads:
            Pa.grad.copy_(g)
            a.step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture; its update is undone below
        two_steps()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        two_steps()
    # back to b's (fresh) state: the warm-up and the capture itself must not count
    Pa.master.copy_(Pb.master)
    a.s1.copy_(b.s1)
    Pa.refresh_copies()
    graph.replay()
    trust_eager = []
    for g in grads:
        b.step(grad=g)
        trust_eager.append(b.layer_trust.clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(Pa.master), _bits(Pb.master)) and torch.equal(_bits(a.s1), _bits(b.s1))
    for k in Pa.w16:
        assert torch.equal(Pa.w16[k], Pb.w16[k])
    assert torch.equal(Pa.wt16["tr"], Pb.wt16["tr"])
    assert torch.equal(_bits(a.layer_trust), _bits(trust_eager[1])) and torch.equal(a.clip_out, b.clip_out)
    assert not torch.equal(_bits(trust_eager[0]), _bits(trust_eager[1]))
    assert int(a.lars.ticket.item()) == 0


# ------------------------------------------------------------------ model
def test_resnet20_step_with_the_flag(tmp_path):
    mj = tmp_path / "m.jsonl"
    fl = flagmod.parse(["--device=cuda", "--synthetic", "--batch_size=8", "--num_steps=1", "--save_model_secs=0",
                        "--lars_eeta", "0.001", "--weight_decay", "1e-4", "--metrics_jsonl=" + str(mj),
                        "--model_dir=" + str(tmp_path / "ck")],
                       model_defaults=dict(batch_size=128, num_steps=1000, learning_rate=0.1))
    model = ResNetModel(0.1, "resnet20")
    logs = []
    prog, opts, gstep = train.run_allreduce(fl, model, torch.device("cuda", 0), logs.append)
    torch.cuda.synchronize()
    assert int(gstep.item()) == 1 and len(opts) == 1 and not any("capture_error" in l for l in logs), logs
    o = opts[0]
    sums, trust = o.lars.sums.cpu().numpy(), o.layer_trust.cpu().numpy()
    adaptive = set(model.decay_vars)
    assert adaptive and set(o.lars.adaptive) == adaptive & set(o.var_list)
    seen = []
    for i, n in enumerate(o.var_list):
        if n in adaptive:  # conv and dense kernels
            assert n.endswith("/kernel") and o.wd[i] == 1e-4
            want = ops.lars_trust_ref(sums[i, 0], sums[i, 1], 0.001, np.float32(1e-4), 0.0)
            assert trust[i].view(np.int32) == want.view(np.int32), (n, trust[i], want)
            assert sums[i, 0] > 0 and sums[i, 1] > 0 and 0 < trust[i] <= 10  # eeta / wd bounds the ratio
            seen.append(float(trust[i]))
        else:  # BatchNorm scales and offsets, biases
            assert trust[i].view(np.int32) == np.float32(1).view(np.int32), (n, trust[i])
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    assert len(rows) == 1 and rows[0]["trust_min"] <= rows[0]["trust_max"]
    assert rows[0]["trust_min"] == min(seen) and rows[0]["trust_max"] == max(seen)
    assert torch.isfinite(prog.P.master).all()
