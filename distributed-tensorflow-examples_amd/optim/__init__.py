"""TF1-exact optimizers over a flat fp32 master buffer.

``FlatParams`` owns every trainable variable of a model as one contiguous fp32
buffer (plus the matching fp32 gradient buffer and optional bf16 working
copies for the MFMA kernels).  ``Optimizer`` applies TF1 ``GradientDescent``,
``Momentum``, ``Adam`` or ``RMSProp`` to a *subset* of those variables (the
reference's ``var_list``) in one fused HIP launch, advancing ``global_step``
(and Adam's ``beta1_power``/``beta2_power``) on device.  CPU tensors take an
exact PyTorch path with the same formulas.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import ops


# fused apply: the transposed-tile work items ahead of the flat ranges (test hook / A/B switch)
TILES_FIRST = True


@dataclass
class VarSpec:
    """One trainable variable.

    name:  TF checkpoint key (e.g. "Variable_3", "rnn/basic_lstm_cell/kernel")
    shape: shape in *this framework's* storage layout
    init:  callable(shape, generator) -> fp32 CPU tensor
    bf16:  keep a natural-layout bf16 working copy
    transpose: (R, T, C) view -> also keep a [C][T][R] bf16 copy (backward GEMM operand)
    tf_shape / to_tf / from_tf: layout conversion for TF-compatible checkpoints
    """
    name: str
    shape: tuple
    init: object
    bf16: bool = False
    transpose: tuple | None = None
    tf_shape: tuple | None = None
    to_tf: object = None
    from_tf: object = None

    @property
    def numel(self) -> int:
        return int(math.prod(self.shape)) if self.shape else 1


class FlatParams:
    """Contiguous fp32 master weights + grads (+ bf16 copies) for a list of VarSpecs."""

    ALIGN = 64  # elements: keep every variable 256-byte aligned for 16 B vector loads

    def __init__(self, specs, device, seed: int = 0, init: bool = True):
        self.specs = list(specs)
        self.device = torch.device(device)
        self.offsets = {}
        off = 0
        for s in self.specs:
            self.offsets[s.name] = off
            off += (s.numel + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.total = off
        self.master = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.w16 = {}
        self.wt16 = {}
        for s in self.specs:
            if s.bf16:
                self.w16[s.name] = torch.zeros(s.shape, dtype=torch.bfloat16, device=self.device)
            if s.transpose is not None:
                self.wt16[s.name] = torch.zeros(s.numel, dtype=torch.bfloat16, device=self.device)
        if init:
            self.initialize(seed)

    # views ------------------------------------------------------------
    def view(self, name):
        s = self.spec(name)
        o = self.offsets[name]
        return self.master[o:o + s.numel].view(s.shape)

    def gview(self, name):
        s = self.spec(name)
        o = self.offsets[name]
        return self.grad[o:o + s.numel].view(s.shape)

    def spec(self, name) -> VarSpec:
        for s in self.specs:
            if s.name == name:
                return s
        a = getattr(self, "aliases", {}).get(name)
        if a is not None:
            return a
        raise KeyError(name)

    def add_alias(self, spec: VarSpec, parent: str, elem_off: int):
        """Register ``spec`` as a view of elements [elem_off, elem_off + numel) of variable ``parent``
        (a partition of it, parallel/partition.py): ``offsets`` / ``view`` / ``gview`` / ``w16`` then
        address it like a variable; layout, initialisation and copies stay the parent's."""
        ps = self.spec(parent)
        assert spec.transpose is None and elem_off + spec.numel <= ps.numel, spec.name
        if not hasattr(self, "aliases"):
            self.aliases = {}
        self.aliases[spec.name] = spec
        self.offsets[spec.name] = self.offsets[parent] + elem_off
        if parent in self.w16:
            self.w16[spec.name] = self.w16[parent].view(-1)[elem_off:elem_off + spec.numel].view(spec.shape)

    def range_of(self, names):
        """[lo, hi) element range covering the given variables (must be contiguous)."""
        los = [self.offsets[n] for n in names]
        his = [self.offsets[n] + self.spec(n).numel for n in names]
        return min(los), max(his)

    # init / copies -------------------------------------------------------
    def initialize(self, seed: int):
        g = torch.Generator().manual_seed(seed)
        for s in self.specs:
            v = s.init(s.shape, g).to(torch.float32)
            self.view(s.name).copy_(v.view(s.shape).to(self.device))
        self.refresh_copies()

    def refresh_copies(self):
        """Recompute bf16 working copies from the masters (after init/restore)."""
        for s in self.specs:
            if s.name in self.w16:
                self.w16[s.name].copy_(self.view(s.name).to(torch.bfloat16))
            if s.name in self.wt16:
                R, T, C = s.transpose
                self.wt16[s.name].copy_(self.view(s.name).reshape(R, T, C).permute(2, 1, 0).reshape(-1)
                                        .to(torch.bfloat16))

    def state_dict(self):
        return {s.name: self.view(s.name).detach().cpu().clone() for s in self.specs}

    def load_state_dict(self, sd):
        for s in self.specs:
            self.view(s.name).copy_(sd[s.name].view(s.shape).to(self.device))
        self.refresh_copies()


KINDS = {"sgd": ops.OPT_SGD, "momentum": ops.OPT_MOMENTUM, "adam": ops.OPT_ADAM, "rmsprop": ops.OPT_RMSPROP}


@dataclass
class OptimizerConfig:
    kind: str = "sgd"
    lr: float = 0.01
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = None  # default per kind: adam 1e-8, rmsprop 1e-10 (TF1 defaults)
    momentum: float = 0.0
    rho: float = 0.9
    name: str = field(default="")
    # tf.clip_by_global_norm over the optimizer's var list before the update; 0 = off (the reference)
    clip_norm: float = 0.0
    # learning-rate schedule, a function of global_step evaluated inside the fused apply (all off = the
    # constant lr): tf.train.piecewise_constant (lr_boundaries / lr_values) or linear decay from lr to
    # lr_end over lr_decay_steps (tf.train.polynomial_decay, power 1), either under a linear warm-up
    lr_boundaries: tuple = ()
    lr_values: tuple = ()
    lr_decay_steps: int = 0
    lr_end: float = 0.0
    lr_warmup_steps: int = 0
    # coupled L2 weight decay (g += weight_decay * p, after the clip scale) on the variables decay_vars
    # (None: every variable of the var list)
    weight_decay: float = 0.0
    decay_vars: tuple | None = None
    # momentum only: TF1 ApplyMomentum's use_nesterov
    nesterov: bool = False
    # tf.train.ExponentialMovingAverage of the var list, updated inside the fused apply: 0 = off, else in
    # [0, 1).  ema_num_updates: the decay is min(ema_decay, (1 + n) / (10 + n)) at the global step n after
    # the apply (TF's num_updates=global_step)
    ema_decay: float = 0.0
    ema_num_updates: bool = False
    # momentum only: layer-wise adaptive rate scaling (tf.contrib.opt.LARSOptimizer).  lars_eeta > 0 turns it
    # on: every variable of lars_vars (None: the whole var list) takes the rate times its trust ratio
    # lars_eeta * |w| / (|g| + wd * |w| + lars_epsilon), wd being that variable's weight decay; the other
    # variables of the var list (the skip list: BatchNorm, biases) keep the rate
    lars_eeta: float = 0.0
    lars_epsilon: float = 0.0
    lars_vars: tuple | None = None

    def has_schedule(self):
        return bool(self.lr_boundaries or self.lr_values or self.lr_decay_steps or self.lr_warmup_steps)

    def resolved_eps(self):
        if self.eps is not None:
            return self.eps
        return 1e-10 if self.kind == "rmsprop" else 1e-8


class GlobalNormClip:
    """``tf.clip_by_global_norm`` over a var list of a FlatParams, on the device: ``compute`` launches
    the norm of ``gscale * grad`` over exactly the var list's elements into ``out = [norm, scale]``
    with ``scale = clip_norm / max(norm, clip_norm)``.  An ``Optimizer`` with ``clip_norm`` owns one
    and hands ``out[1:]`` to its fused apply; a ps worker owns one per optimizer group and scales its
    gradient in place (``scale_grad``) before the push.  Stateless: nothing to checkpoint."""

    def __init__(self, params: FlatParams, var_list, clip_norm: float):
        if not clip_norm > 0:
            raise ValueError("GlobalNormClip: clip_norm must be > 0, got %r" % (clip_norm,))
        self.P = params
        self.clip_norm = float(clip_norm)
        dev = params.device
        self.plan = ops.grad_norm_plan([(params.offsets[n], params.spec(n).numel) for n in var_list], params.master)
        self.partials = torch.zeros(max(1, self.plan.shape[0]), dtype=torch.float32, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)

    def compute(self, grad=None, grad16=None, gscale: float = 1.0, max_blocks: int = 0):
        """Launch the norm on the current stream; returns the scale as a 1-element device tensor.
        (``max_blocks``: test hook, caps the grid.)"""
        if grad is None and grad16 is None:
            grad = self.P.grad
        if (grad if grad is not None else grad16).numel() < self.P.total:
            raise ValueError("GlobalNormClip: the gradient is shorter than the flat parameter buffer")
        ops.grad_sumsq(grad, grad16, gscale, self.clip_norm, self.plan, self.partials, self.ticket, self.out,
                       max_blocks)
        return self.out[1:]

    def scale_grad(self, grad=None):
        """grad[var list] *= scale, in place (after ``compute``)."""
        ops.scale_(self.P.grad if grad is None else grad, self.out[1:], self.plan)

    @property
    def norm(self):
        return self.out[:1]


class LayerTrust:
    """The trust ratios of LARS (``tf.contrib.opt.LARSOptimizer``) over a var list of a FlatParams, on the
    device: ``compute`` launches the norms of master and ``gscale * grad`` of every adaptive variable into
    ``sums[i] = (sum w^2, sum g^2)`` and ``trust[i] = eeta * |w| / (|g| + wd[i] * |w| + eps)`` (1 where a norm is
    zero), ``i`` the variable's index in the var list.  The variables outside ``adaptive`` hold a trust of
    exactly 1, written here once.  An ``Optimizer`` with ``lars_eeta`` owns one and binds ``trust`` into its
    fused apply as the per-segment factor of the rate.  Stateless: nothing to checkpoint."""

    def __init__(self, params: FlatParams, var_list, adaptive, wd, eeta: float, eps: float = 0.0, chunk: int = 0):
        if not (eeta > 0 and math.isfinite(eeta)) or not (eps >= 0 and math.isfinite(eps)):
            raise ValueError("LayerTrust: eeta must be > 0 and epsilon >= 0, got %r and %r" % (eeta, eps))
        var_list = list(var_list)
        unknown = [n for n in adaptive if n not in var_list]
        if unknown:
            raise ValueError("LayerTrust: the adaptive variables %r are not in the var list" % (unknown,))
        if len(wd) != len(var_list):
            raise ValueError("LayerTrust: one weight decay per variable of the var list")
        self.P = params
        self.eeta, self.eps = float(eeta), float(eps)
        self.adaptive = [n for n in var_list if n in set(adaptive)]
        self.index = [var_list.index(n) for n in self.adaptive]
        dev, nseg = params.device, len(var_list)
        self.plan, self.ranges, self.limit = ops.layer_trust_plan(
            [(i, params.offsets[n], params.spec(n).numel) for i, n in zip(self.index, self.adaptive)], params.master,
            chunk)
        self.wd = torch.tensor([float(w) for w in wd], dtype=torch.float32).reshape(nseg).to(dev)
        self.partials = torch.zeros(max(1, 2 * self.plan.shape[0]), dtype=torch.float32, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sums = torch.zeros(nseg, 2, dtype=torch.float32, device=dev)
        self.trust = torch.ones(nseg, dtype=torch.float32, device=dev)
        self.launches = 0  # how often compute ran (tests: an optimizer without LARS never launches)

    def compute(self, grad=None, grad16=None, gscale: float = 1.0, clip_scale=None, max_blocks: int = 0):
        """Launch on the current stream; returns ``trust``.  ``clip_scale``: the 1-element device tensor of a
        global-norm clip computed before (the clip scales the gradient the optimizer sees).
        (``max_blocks``: test hook, caps the grid.)"""
        if grad is None and grad16 is None:
            grad = self.P.grad
        if (grad if grad is not None else grad16).numel() < self.P.total:
            raise ValueError("LayerTrust: the gradient is shorter than the flat parameter buffer")
        self.launches += 1
        ops.layer_trust(self.P.master, grad, grad16, gscale, self.plan, self.ranges, self.limit, self.wd, self.eeta,
                        self.eps, clip_scale, self.partials, self.ticket, self.sums, self.trust, max_blocks)
        return self.trust


class Optimizer:
    """Fused TF1 optimizer over a subset (var_list) of a FlatParams.

    Slot variables follow TF1 naming: ``<var>/Adam``, ``<var>/Adam_1``;
    ``<var>/RMSProp`` (initialised to ones), ``<var>/RMSProp_1``;
    ``<var>/Momentum``.  Adam's non-slot ``beta1_power``/``beta2_power`` are a
    2-element device tensor advanced by the kernel itself.  With ``cfg.ema_decay`` the optimizer also keeps
    ``tf.train.ExponentialMovingAverage`` shadows of its variables (``ema``, checkpointed as
    ``<var>/ExponentialMovingAverage``), updated by the same launch; ``swap_ema`` / ``averaged`` put them in the
    variables' place.  On the CPU the update goes through the numpy-float32 mirror: the same bits as the kernel's.

    On the GPU the optimizer is bound to the native side once (``ops.opt_state``): plan, slots, counters
    and the recipe are checked and fixed at construction, and of the config only ``cfg.lr`` is read at
    every step - changing ``cfg.beta1``, ``beta2``, ``eps``, ``momentum`` or ``rho`` afterwards has no
    effect there (the CPU path still reads them).  Likewise the tensors (``s1``, ``s2``, ``beta_pow``,
    ``global_step``, ``done``) are bound as they are at construction: write into them, do not replace them.
    """

    SLOT_NAMES = {"adam": ("Adam", "Adam_1"), "rmsprop": ("RMSProp", "RMSProp_1"), "momentum": ("Momentum",),
                  "sgd": ()}
    EMA_NAME = "ExponentialMovingAverage"

    def __init__(self, cfg: OptimizerConfig, params: FlatParams, var_list=None, global_step=None,
                 beta_power_names=("beta1_power", "beta2_power"), slots_of=None, beta_pow=None):
        """``slots_of``: another Optimizer over the same FlatParams whose slot buffers this one uses (disjoint
        var lists) in place of its own; ``beta_pow``: Adam's beta powers to advance in place of an own pair."""
        self.cfg = cfg
        self.P = params
        self.kind = KINDS[cfg.kind]
        self.var_list = [s.name for s in params.specs] if var_list is None else list(var_list)
        self.device = params.device
        self.global_step = global_step  # int32 [1] device tensor or None
        self.beta_power_names = beta_power_names
        nslots = len(self.SLOT_NAMES[cfg.kind])
        # slots live in full-size flat buffers (same offsets as the masters)
        self.s1 = self.s2 = None
        if slots_of is not None:
            self.s1, self.s2 = slots_of.s1, slots_of.s2
        elif nslots >= 1:
            fill = 1.0 if cfg.kind == "rmsprop" else 0.0
            self.s1 = torch.full((params.total,), fill, dtype=torch.float32, device=self.device)
            if nslots >= 2:
                self.s2 = torch.zeros(params.total, dtype=torch.float32, device=self.device)
        if cfg.kind != "adam":
            self.beta_pow = None
        elif beta_pow is not None:
            self.beta_pow = beta_pow
        else:
            self.beta_pow = torch.tensor([cfg.beta1, cfg.beta2], dtype=torch.float32, device=self.device)
        self.done = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._state = None
        self._init_recipe()
        if self.device.type == "cuda":
            self._build_plan()
        # global-norm clipping (cfg.clip_norm > 0): the norm kernel's chunk plan, scratch and its two
        # results clip_out = [norm, scale]; the apply reads the scale from the device.  No state to save.
        self.clip_norm = float(getattr(cfg, "clip_norm", 0.0) or 0.0)
        if self.clip_norm < 0:
            raise ValueError("clip_norm must be >= 0 (0 = no clipping), got %r" % (cfg.clip_norm,))
        self.clip = GlobalNormClip(params, self.var_list, self.clip_norm) if self.clip_norm > 0 else None

    def _init_recipe(self):
        """Schedule, weight decay and Nesterov of the config, validated; all of it off by default."""
        cfg = self.cfg
        self.lr_spec, self._lr_out = None, None
        if cfg.has_schedule():
            if self.global_step is None:
                raise ValueError("Optimizer: a learning-rate schedule is a function of global_step - pass one")
            self.lr_spec = ops.lr_schedule_spec(cfg.lr, cfg.lr_boundaries, cfg.lr_values, cfg.lr_decay_steps,
                                                cfg.lr_end, cfg.lr_warmup_steps)
            self._lr_out = torch.full((1,), float(ops.lr_schedule_value(self.lr_spec, 0)), dtype=torch.float32,
                                      device=self.device)
        self.nesterov = bool(cfg.nesterov)
        if self.nesterov and cfg.kind != "momentum":
            raise ValueError("Optimizer: nesterov is an option of the momentum optimizer, not of %r" % (cfg.kind,))
        wd = float(cfg.weight_decay or 0.0)
        if wd < 0:
            raise ValueError("weight_decay must be >= 0 (0 = none), got %r" % (cfg.weight_decay,))
        decay_vars = self.var_list if cfg.decay_vars is None else list(cfg.decay_vars)
        unknown = [n for n in decay_vars if n not in self.var_list]
        if wd > 0 and unknown:
            raise ValueError("Optimizer: decay_vars %r are not in the var list" % (unknown,))
        # per variable of the var list; float32 as the kernel holds it
        self.wd = [wd if wd > 0 and n in decay_vars else 0.0 for n in self.var_list]
        self.decay = any(w != 0 for w in self.wd)
        # exponential moving average: the shadow starts as the variables' initial values (TF initialises it
        # so); full-size like the slots, elements outside the var list are never written
        d = float(getattr(cfg, "ema_decay", 0.0) or 0.0)
        if not 0.0 <= d < 1.0 or not float(ops.ema_decay_value(d, False, 0)) < 1.0:
            raise ValueError("ema_decay must lie in [0, 1) (0 = no moving average), got %r" % (cfg.ema_decay,))
        self.ema_decay = d
        self.ema_num_updates = bool(getattr(cfg, "ema_num_updates", False))
        self.ema, self._ema_out = None, None
        if self.ema_num_updates and not d > 0:
            raise ValueError("Optimizer: ema_num_updates needs ema_decay > 0")
        if d > 0:
            if self.ema_num_updates and self.global_step is None:
                raise ValueError("Optimizer: ema_num_updates makes the decay a function of global_step - pass one")
            self.ema = self.P.master.clone()
            self._ema_out = torch.full((1,), float(ops.ema_decay_value(d, False, 0)), dtype=torch.float32,
                                       device=self.device)
        # LARS: a trust ratio per variable, computed by a launch of its own before the apply, which reads it
        # as the per-segment factor of the rate.  No state to save.
        eeta = float(getattr(cfg, "lars_eeta", 0.0) or 0.0)
        self.lars = None
        if eeta < 0:
            raise ValueError("lars_eeta must be >= 0 (0 = no layer-wise scaling), got %r" % (cfg.lars_eeta,))
        if eeta > 0:
            if cfg.kind != "momentum":
                raise ValueError("Optimizer: lars_eeta is an option of the momentum optimizer, not of %r" % (cfg.kind,))
            lars_vars = getattr(cfg, "lars_vars", None)
            lars_vars = self.var_list if lars_vars is None else list(lars_vars)
            unknown = [n for n in lars_vars if n not in self.var_list]
            if unknown:
                raise ValueError("Optimizer: lars_vars %r are not in the var list" % (unknown,))
            self.lars = LayerTrust(self.P, self.var_list, lars_vars, self.wd, eeta,
                                   float(getattr(cfg, "lars_epsilon", 0.0) or 0.0))

    @property
    def layer_trust(self):
        """The last step's trust ratio of every variable of the var list ([nseg] device tensor, 1 for the
        variables LARS skips; before any step: all 1) - read it on the host only when it is wanted; None
        without lars_eeta."""
        return None if self.lars is None else self.lars.trust

    @property
    def current_ema_decay(self):
        """The decay the last step's moving average used (before any step: ema_decay) as a 1-element device
        tensor - read it on the host only when it is wanted; None without ema_decay."""
        return self._ema_out

    def swap_ema(self):
        """Exchange the var list's masters with their moving averages and rewrite the bf16 working copies
        from the new masters: one launch on the GPU (capturable), tensor ops on the CPU.  A second call
        restores masters, averages and copies bit for bit."""
        if self.ema is None:
            raise ValueError("Optimizer.swap_ema: the optimizer keeps no moving average (ema_decay is 0)")
        if self.device.type == "cuda":
            ops.ema_swap(self._state)
            return
        with torch.no_grad():
            for name in self.var_list:
                o, n = self.P.offsets[name], self.P.spec(name).numel
                v, e = self.P.master[o:o + n], self.ema[o:o + n]
                t = v.clone()
                v.copy_(e)
                e.copy_(t)
            self.P.refresh_copies()

    @contextlib.contextmanager
    def averaged(self):
        """Inside the block the model's weights (masters and bf16 copies) are the moving averages; the
        trained ones come back on leaving it, also when the body raises."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    @property
    def current_lr(self):
        """The rate the last step used (before any step: the rate of step 0) as a 1-element device tensor
        - read it on the host only when it is wanted; None without a schedule (the rate is cfg.lr)."""
        return self._lr_out

    # ---- plan of work items for the fused kernel
    def _build_plan(self, chunk: int = 0):
        # flat work items of `chunk` elements (DTFE_OPT_CHUNK; multiple of 1024): one workgroup
        # each, up to 2048 workgroups per launch.  Default 8192; 2048 for var lists under 2 M elements
        # (the GAN's two Adams over 0.43 M params: 52 workgroups -> 209, 0.0736 -> 0.0702 ms/step; the
        # autoencoder -1 %, LSTM / ResNet-20 neutral - profiles/r6_ref_models_fused.txt)
        if not chunk:
            env = os.environ.get("DTFE_OPT_CHUNK")
            total = sum(self.P.spec(name).numel for name in self.var_list)
            chunk = int(env) if env else (2048 if total < 2_000_000 else 8192)
        segs, work = [], []
        for si, name in enumerate(self.var_list):
            s = self.P.spec(name)
            w16 = self.P.w16.get(name)
            wt16 = self.P.wt16.get(name)
            if s.transpose is not None:
                R, T, C = s.transpose
            else:
                R, T, C = s.numel, 1, 1
            segs.append([self.P.offsets[name], R, T, C, w16.data_ptr() if w16 is not None else 0,
                         wt16.data_ptr() if wt16 is not None else 0])
            if wt16 is not None:
                for t in range(T):
                    for r0 in range(0, R, 64):
                        for c0 in range(0, C, 64):
                            work.append([1, si, t, r0, c0, 0, 0])
            else:
                n = s.numel
                for st in range(0, n, chunk):
                    work.append([0, si, 0, 0, 0, st, min(chunk, n - st)])
        if TILES_FIRST:
            # transposed-copy tiles first: they are short latency chains (16 dependent-free loads, an
            # LDS transpose, scattered stores); dispatched last they were the launch's tail
            work.sort(key=lambda w: -w[0])
        self.nseg, self.nwork = len(segs), len(work)
        self._tables = (segs, work)  # what the state was built from (tests rebuild it)
        c = self.cfg
        sched = ops.lr_schedule_pack(self.lr_spec, self.P.master) if self.lr_spec is not None else None
        self._state = ops.opt_state(self.kind, self.P.master, segs, work, self.done, s1=self.s1, s2=self.s2,
                                    beta1=c.beta1, beta2=c.beta2, eps=c.resolved_eps(), momentum=c.momentum,
                                    rho=c.rho, beta_pow=self.beta_pow, global_step=self.global_step,
                                    wd=self.wd if self.decay else None, sched=sched, lr_out=self._lr_out,
                                    nesterov=self.nesterov, decay=self.decay, ema=self.ema,
                                    ema_decay=self.ema_decay, ema_num_updates=self.ema_num_updates,
                                    ema_out=self._ema_out, seg_lr=self.layer_trust)

    def _wait_mask(self, names) -> int:  # the kernel's wait_segs: 32 bits of var_list indices
        idx = [self.var_list.index(n) if n in self.var_list else -1 for n in names]
        if any(not 0 <= i < 32 for i in idx):
            raise ValueError(f"Optimizer.step(wait=...): {list(names)} must be among the first 32 of var_list")
        return sum(1 << i for i in idx)

    @property
    def global_norm(self):
        """The last step's global gradient norm (after gscale, before clipping) as a 1-element device
        tensor - read it on the host (``.item()``) only when it is wanted; None without clip_norm."""
        return None if self.clip is None else self.clip.out[:1]

    @property
    def clip_out(self):
        """[norm, scale] of the last step's clip (2-float device tensor); None without clip_norm."""
        return None if self.clip is None else self.clip.out

    def step(self, grad=None, grad16=None, gscale: float = 1.0, gs_inc: int = 1, wait=None):
        """Apply gradients (default: the FlatParams grad buffer) to var_list.  ``wait`` (GPU; ignored
        on the CPU) = ``(done, seen, var_names)``: the launch's items of those variables wait on the
        device until the int32 counter ``done`` exceeds ``seen`` (ops.epoch_signal after their
        gradient's producer on another stream); the launch then advances ``seen``."""
        if grad is None and grad16 is None:
            grad = self.P.grad
        if self.clip_norm > 0 and wait is not None:
            # the norm needs every gradient of the var list before the first update
            raise ValueError("Optimizer.step: clip_norm cannot be combined with wait= (a gradient still in flight)")
        if self.lars is not None and wait is not None:
            # the norms need every gradient of the var list before the first update
            raise ValueError("Optimizer.step: lars_eeta cannot be combined with wait= (a gradient still in flight)")
        wait = (None, None, 0) if wait is None else (wait[0], wait[1], self._wait_mask(wait[2]))
        clip = self.clip.compute(grad, grad16, gscale) if self.clip is not None else None
        if self.lars is not None:  # after the clip, whose scale it reads; the apply reads its trust ratios
            self.lars.compute(grad, grad16, gscale, clip_scale=clip)
        if self.device.type == "cuda":
            ops.apply_gradients(self._state, grad, grad16, gscale, self.cfg.lr, gs_inc, *wait, clip_scale=clip)
            return
        self._step_cpu(grad if grad is not None else grad16.float(), gscale, gs_inc, clip)

    @staticmethod
    def step_all(opts, gs_incs, grad=None, grad16=None, gscale: float = 1.0):
        """Apply several optimizers over disjoint var lists of one FlatParams (the reference's
        several ``minimize`` calls per step).  On the GPU, optimizers of one kind share ONE grouped
        launch (each keeps its own beta powers / global-step increment); the math equals
        calling ``step`` on each in order."""
        kinds = {o.kind for o in opts}
        # Optimizers with a schedule take the sequential path: in the grouped launch one optimizer's last
        # workgroup may advance the shared global_step before another optimizer's workgroups have read
        # it, and those would evaluate their schedule one step ahead.  One launch each keeps every read
        # of the step before the launch that advances it (stream order).
        # Likewise optimizers with a moving average: with num_updates its decay is a function of the step.
        # And optimizers with LARS: the grouped kernels have no instantiation with a per-segment rate.
        scheduled = any(o.lr_spec is not None or o.ema is not None or o.lars is not None for o in opts)
        if (len(opts) > 1 and len(opts) <= 4 and len(kinds) == 1 and not scheduled
                and all(o.device.type == "cuda" for o in opts)):
            P = opts[0].P
            assert all(o.P is P for o in opts)
            # one norm launch per clipping optimizer, then the one grouped apply reads each one's scale
            clips = [o.clip.compute(grad, grad16, gscale) if o.clip is not None else None for o in opts]
            ops.apply_gradients_group(
                [o._state for o in opts], P.grad if grad is None and grad16 is None else grad, grad16, gscale,
                [o.cfg.lr for o in opts], list(gs_incs), clips if any(c is not None for c in clips) else None)
            return
        for o, inc in zip(opts, gs_incs):
            o.step(grad=grad, grad16=grad16, gscale=gscale, gs_inc=inc)

    @torch.no_grad()
    def _step_cpu(self, grad, gscale, gs_inc, clip=None):
        c = self.cfg
        if clip is not None:  # g * (gscale * scale), as the kernel forms it
            gscale = float(gscale) * float(clip[0])
        lr = c.lr
        if self.lr_spec is not None:  # the rate of the step this apply starts from, as the kernel reads it
            lr = float(ops.lr_schedule_value(self.lr_spec, int(self.global_step.item())))
            self._lr_out[0] = lr
        lr_t = lr
        if c.kind == "adam":
            b1p, b2p = self.beta_pow.tolist()
            lr_t = lr * math.sqrt(1 - b2p) / (1 - b1p)
        eps = c.resolved_eps()
        ema_d = None
        if self.ema is not None:  # the decay at the step after this apply's advance, as the kernel forms it
            n = (int(self.global_step.item()) + int(gs_inc)) if self.ema_num_updates else 0
            ema_d = ops.ema_decay_value(self.ema_decay, self.ema_num_updates, n)
            self._ema_out[0] = float(ema_d)
        lr0, f = lr, np.float32
        for i, (name, wd) in enumerate(zip(self.var_list, self.wd)):
            s = self.P.spec(name)
            o, n = self.P.offsets[name], s.numel
            if self.lars is not None:  # the rate of this variable: one float32 multiply, as the kernel forms it
                lr = float(f(lr0) * f(self.lars.trust[i].item()))
            v, g = self.P.master[o:o + n], grad[o:o + n] * gscale
            if wd:  # coupled L2, after the clip scale
                g = g + wd * v
            if c.kind == "sgd":
                v -= lr * g
            elif c.kind == "momentum":
                a = self.s1[o:o + n]
                a.mul_(c.momentum).add_(g)
                if self.nesterov:
                    v -= g * lr + a * c.momentum * lr
                else:
                    v -= lr * a
            elif c.kind == "adam":
                m, v2 = self.s1[o:o + n], self.s2[o:o + n]
                m.mul_(c.beta1).add_((1 - c.beta1) * g)
                v2.mul_(c.beta2).add_((1 - c.beta2) * g * g)
                v -= lr_t * m / (v2.sqrt() + eps)
            else:
                ms, mom = self.s1[o:o + n], self.s2[o:o + n]
                ms.mul_(c.rho).add_((1 - c.rho) * g * g)
                mom.mul_(c.momentum).add_(lr * g / (ms + eps).sqrt())
                v -= mom
            if ema_d is not None:  # through the numpy mirror: the same bits as the kernel's update
                e = self.ema[o:o + n]
                e.copy_(torch.from_numpy(ops.ema_update_ref(e.numpy(), v.numpy(), ema_d)))
        if c.kind == "adam":
            self.beta_pow[0] *= c.beta1
            self.beta_pow[1] *= c.beta2
        if self.global_step is not None and gs_inc:
            self.global_step += gs_inc

    # ---- checkpoint naming (TF1 slot conventions)
    def slot_tensors(self):
        """{checkpoint key: fp32 CPU tensor} for this optimizer's slots and non-slot variables."""
        out = {}
        names = self.SLOT_NAMES[self.cfg.kind]
        for var in self.var_list:
            s = self.P.spec(var)
            o, n = self.P.offsets[var], s.numel
            for i, sn in enumerate(names):
                buf = self.s1 if i == 0 else self.s2
                out[f"{var}/{sn}"] = buf[o:o + n].detach().cpu().view(s.shape).clone()
            if self.ema is not None:  # tf.train.ExponentialMovingAverage's shadow variable name
                out[f"{var}/{self.EMA_NAME}"] = self.ema[o:o + n].detach().cpu().view(s.shape).clone()
        if self.beta_pow is not None:
            bp = self.beta_pow.detach().cpu()
            out[self.beta_power_names[0]] = bp[0].clone()
            out[self.beta_power_names[1]] = bp[1].clone()
        return out

    def load_slot_tensors(self, tensors):
        names = self.SLOT_NAMES[self.cfg.kind]
        for var in self.var_list:
            s = self.P.spec(var)
            o, n = self.P.offsets[var], s.numel
            for i, sn in enumerate(names):
                key = f"{var}/{sn}"
                if key in tensors:
                    buf = self.s1 if i == 0 else self.s2
                    buf[o:o + n].copy_(tensors[key].reshape(-1).to(self.device))
            if self.ema is not None:
                key = f"{var}/{self.EMA_NAME}"
                if key in tensors:
                    self.ema[o:o + n].copy_(tensors[key].reshape(-1).to(self.device))
                else:  # a checkpoint from a run without EMA: start the average at the restored variable
                    self.ema[o:o + n].copy_(self.P.master[o:o + n])
        if self.beta_pow is not None and self.beta_power_names[0] in tensors:
            self.beta_pow[0] = float(tensors[self.beta_power_names[0]])
            self.beta_pow[1] = float(tensors[self.beta_power_names[1]])
