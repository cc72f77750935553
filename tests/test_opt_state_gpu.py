"""The bound optimizer state (ops.opt_state / torch.classes.dtfe.OptState): what it refuses at construction
and at a launch - always before anything is launched - and what a launch reads from it."""
import numpy as np
import pytest
import torch

import dtfe.ops as ops
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig, VarSpec

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 5000
R, T, C = 70, 3, 50  # the transposed segment of test_kernels_gpu.test_optimizer_transposed_copies


def _plan(n):  # one segment, one flat work item
    return [[0, n, 1, 1, 0, 0]], [[0, 0, 0, 0, 0, 0, n]]


def _zeros(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device=DEV)


class _Untouched:
    """A parameter buffer and a done counter; ``check()``: both are as they were made."""

    def __init__(self, n=N):
        torch.manual_seed(3)
        self.p = torch.randn(n, device=DEV)
        self.p0 = self.p.clone()
        self.done = _zeros(1, torch.int32)

    def check(self):
        torch.cuda.synchronize()
        assert torch.equal(self.p.view(torch.int32), self.p0.view(torch.int32))
        assert int(self.done.item()) == 0


# ------------------------------------------------------------ gradient arguments
GRADS = {
    "g is bf16": lambda: (_zeros(N, torch.bfloat16), None),
    "g16 is float32": lambda: (None, _zeros(N)),
    "g is one short": lambda: (_zeros(N - 1), None),
    "g is on the CPU": lambda: (torch.zeros(N), None),
    "g is not contiguous": lambda: (_zeros(2 * N)[::2], None),
    "both": lambda: (_zeros(N), _zeros(N, torch.bfloat16)),
    "neither": lambda: (None, None),
}


@pytest.mark.parametrize("case", list(GRADS))
def test_a_launch_refuses_a_gradient_it_cannot_read(case):
    u = _Untouched()
    st = ops.opt_state(ops.OPT_SGD, u.p, *_plan(N), u.done)
    g, g16 = GRADS[case]()
    with pytest.raises(RuntimeError, match="apply_gradients"):
        ops.apply_gradients(st, g, g16, 1.0, 0.1, 0)
    u.check()


# -------------------------------------------------- state arguments at construction
def _bp(n=2):
    return torch.tensor([0.9, 0.999][:n], device=DEV)


STATES = {
    "momentum, s1 one short": (dict(kind=ops.OPT_MOMENTUM, s1=lambda: _zeros(N - 1)), "s1"),
    "adam without beta_pow": (dict(kind=ops.OPT_ADAM, s1=lambda: _zeros(N), s2=lambda: _zeros(N)), "adam"),
    "beta_pow with one element": (dict(kind=ops.OPT_ADAM, s1=lambda: _zeros(N), s2=lambda: _zeros(N),
                                       beta_pow=lambda: _bp(1)), "beta_pow"),
    "global_step is int64": (dict(kind=ops.OPT_SGD, global_step=lambda: _zeros(1, torch.int64)), "global_step"),
    "sched without global_step": (dict(kind=ops.OPT_SGD, sched=lambda: ops.lr_schedule_pack(
        ops.lr_schedule_spec(0.1, warmup_steps=2), _zeros(1))), "schedule"),
    "nesterov with sgd": (dict(kind=ops.OPT_SGD, nesterov=lambda: True), "nesterov"),
}


@pytest.mark.parametrize("case", list(STATES))
def test_the_state_refuses_tensors_a_launch_could_not_use(case):
    kw, match = STATES[case]
    kw = {k: v() if callable(v) else v for k, v in kw.items()}
    u = _Untouched()
    with pytest.raises(RuntimeError, match=match):
        ops.opt_state(kw.pop("kind"), u.p, *_plan(N), u.done, **kw)
    u.check()


# ----------------------------------------------------- plan tables at construction
PLANS = {  # name: (numel of p, segs, work, wd, match); WT16 stands for the address of a [C][T][R] bf16 copy
    "a segment longer than p": (N, [[0, N + 1, 1, 1, 0, 0]], [[0, 0, 0, 0, 0, 0, N]], None, "segs"),
    "a second segment past the end of p": (N, [[0, 4000, 1, 1, 0, 0], [4000, 1001, 1, 1, 0, 0]],
                                           [[0, 0, 0, 0, 0, 0, 4000], [0, 1, 0, 0, 0, 0, 1000]], None, "segs"),
    "a work item of segment 1 of 1": (N, [[0, N, 1, 1, 0, 0]], [[0, 1, 0, 0, 0, 0, N]], None, "work"),
    "a flat item past its segment": (N, [[0, N, 1, 1, 0, 0]], [[0, 0, 0, 0, 0, 4096, 1000]], None, "work"),
    "a tile item with r0 past R": (R * T * C, [[0, R, T, C, 0, "WT16"]], [[1, 0, 0, 128, 0, 0, 0]], None, "work"),
    "a tile item without a wt16": (N, [[0, 50, 2, 50, 0, 0]], [[1, 0, 0, 0, 0, 0, 0]], None, "work"),
    "wd of two entries for one segment": (N, *_plan(N), [0.0, 0.0], "wd"),
    "a negative wd": (N, *_plan(N), [-1.0], "wd"),
}


@pytest.mark.parametrize("case", list(PLANS))
def test_the_state_refuses_a_plan_that_leaves_its_buffers(case):
    n, segs, work, wd, match = PLANS[case]
    wt16 = _zeros(R * T * C, torch.bfloat16)
    segs = [[wt16.data_ptr() if x == "WT16" else x for x in row] for row in segs]
    u = _Untouched(n)
    with pytest.raises(RuntimeError, match=match):
        ops.opt_state(ops.OPT_SGD, u.p, segs, work, u.done, wd=wd, decay=wd is not None)
    u.check()
    assert int(wt16.view(torch.int16).abs().max().item()) == 0


# ---------------------------------------------------- one bound state, many launches
LRS = (0.1, 0.2, 0.3)


def _sgd_mirror(p0, g):
    """numpy float32: v -= lr * g for each rate of LRS, each product and difference rounded once."""
    v = p0.cpu().numpy().copy()
    for lr in LRS:
        v = v - np.float32(lr) * g.cpu().numpy()
        assert v.dtype == np.float32
    return v.view(np.int32)


def test_the_rate_is_read_at_every_launch():
    torch.manual_seed(4)
    p0, g = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    p = p0.clone()
    st = ops.opt_state(ops.OPT_SGD, p, *_plan(N), _zeros(1, torch.int32))
    for lr in LRS:
        ops.apply_gradients(st, g, None, 1.0, lr, 0)
    assert np.array_equal(p.cpu().numpy().view(np.int32), _sgd_mirror(p0, g))


def test_the_op_and_the_states_method_are_the_same_launch():
    torch.manual_seed(8)
    p0, g = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
    res = []
    for launch in (lambda st, *a: ops.require().apply_gradients(st, *a), lambda st, *a: st.apply(*a, None, None, 0, None)):
        p, acc = p0.clone(), _zeros(N)
        st = ops.opt_state(ops.OPT_MOMENTUM, p, *_plan(N), _zeros(1, torch.int32), s1=acc, momentum=0.9)
        for lr in LRS:
            launch(st, g, None, 0.5, lr, 0)
        res.append((p, acc))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], p0)


def test_the_optimizer_reads_cfg_lr_at_every_step():
    P = FlatParams([VarSpec("v", (N,), lambda shape, gen: torch.randn(shape, generator=gen))], DEV, seed=5)
    p0 = P.master.clone()
    torch.manual_seed(6)
    P.gview("v").copy_(torch.randn(N))
    opt = Optimizer(OptimizerConfig(kind="sgd", lr=LRS[0]), P)
    for lr in LRS:
        opt.cfg.lr = lr
        opt.step()
    assert np.array_equal(P.master[:N].cpu().numpy().view(np.int32), _sgd_mirror(p0[:N], P.grad[:N]))


# ------------------------------------------------- the group takes each state's own
def test_a_grouped_launch_uses_each_states_own_fields():
    n, h = 6000, 3000
    torch.manual_seed(7)
    p0, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    res = []
    for grouped in (True, False):
        p, s1, s2, gs = p0.clone(), _zeros(n), _zeros(n), _zeros(1, torch.int32)
        bps = [torch.tensor([b1, 0.999], device=DEV) for b1 in (0.9, 0.5)]
        sts = [ops.opt_state(ops.OPT_ADAM, p, [[lo, h, 1, 1, 0, 0]], [[0, 0, 0, 0, 0, 0, h]], _zeros(1, torch.int32),
                             s1=s1, s2=s2, beta1=b1, beta2=0.999, eps=1e-8, beta_pow=bp, global_step=gs)
               for lo, b1, bp in zip((0, h), (0.9, 0.5), bps)]
        lrs, incs = [0.01, 0.02], [0, 2]
        for _ in range(2):
            if grouped:
                ops.require().apply_gradients_group(sts, g, None, 1.0, lrs, incs)
            else:
                for st, lr, inc in zip(sts, lrs, incs):
                    ops.apply_gradients(st, g, None, 1.0, lr, inc)
        torch.cuda.synchronize()
        res.append([p, s1, s2, *bps, gs])
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert int(res[0][-1].item()) == 4
    assert not torch.equal(res[0][3], res[0][4])  # each advanced its own beta1 power
