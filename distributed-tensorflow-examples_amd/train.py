"""The shared ``main(_)`` of every example script.

``run(model_name, argv)`` reproduces the reference scripts' behaviour once,
for every model (the reference copy-pastes it three times, GAN/ENC/LSTM):

* ``--job_name=ps``: host this task's variable shard, serve the workers, count
  done signals (``ps %d received done %d`` / ``ps %d: quitting``);
* ``--job_name=worker``: build the step program, join the Supervisor (chief =
  task 0), pull -> compute gradients -> push/pull per step printing
  ``Global step %d Local step %d  AvgTime: %3.2fms``, print ``Total Time``,
  (LSTM) ``Test-Accuracy``, signal done to every ps, stop.

plus the north-star modes: ``--sync`` (sync SGD with a chief over the ps) and
``--mode=allreduce`` (ring all-reduce data parallelism, no ps).
"""
from __future__ import annotations

import contextlib
import dataclasses
import json
import os
import sys
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from . import ckpt, ops
from .data import cifar, imagenet_synth
from .data.mnist import DeviceBatcher, read_data_sets as read_mnist
from .models.autoencoder import AutoencoderModel
from .models.base import ScaledScalar
from .models.gan import LR as GAN_LR, GanModel
from .models.lstm import LR as LSTM_LR, LstmModel
from .models.mnist_cnn import MnistCnnModel
from .models.resnet import ResNetModel
from .models.softmax_reg import SoftmaxRegressionModel
from .models.autoencoder import LR as ENC_LR
from .optim import GlobalNormClip, Optimizer
from .parallel.allreduce import BucketAllReduce
from .parallel.comm import make_comm
from .parallel.cluster import ClusterSpec, Server
from .parallel.health import CommWatchdog, Heartbeat, Watchdog
from .utils.faults import FaultInjector
from .utils.timers import PhaseTimer
from .parallel.partition import PartitionedModel
from .parallel.placement import round_robin
from .parallel import ps_native
from .parallel.ps import PSClient, PSServer, Shard, wait_for_init
from .parallel.supervisor import Supervisor
from .utils import device_eval, flags as flagmod
from .utils.graphs import MultiStepGraph, StepGraph

MODELS = {
    "gan": (GanModel, GAN_LR),
    "encoder": (AutoencoderModel, ENC_LR),
    "lstm": (LstmModel, LSTM_LR),
    "softmax": (SoftmaxRegressionModel, 0.01),
    "cnn": (MnistCnnModel, 0.001),
    "resnet20": (lambda lr=0.1: ResNetModel(lr, "resnet20"), 0.1),
    "resnet50": (lambda lr=0.1: ResNetModel(lr, "resnet50"), 0.1),
}


def read_data_sets(model, data_dir, one_hot=True, seed=0, log=print):
    """The model's dataset: MNIST (reference models + CNN), CIFAR-10 (ResNet-20) or a
    synthetic ImageNet-shape set (ResNet-50)."""
    name = getattr(model, "name", "")
    if name == "resnet20":
        return cifar.read_data_sets(data_dir, one_hot=one_hot, seed=seed, log=log)
    if name == "resnet50":
        return imagenet_synth.read_data_sets(one_hot=one_hot, seed=seed, log=log)
    return read_mnist(data_dir, one_hot=one_hot, seed=seed, log=log)


def _print(*args):
    print(*args, flush=True)


def resolve_device(flag: str, local_rank: int = 0):
    if flag == "cpu" or (flag == "auto" and not torch.cuda.is_available()):
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise RuntimeError("--device=cuda but no GPU is visible")
    n = torch.cuda.device_count()
    return torch.device("cuda", local_rank % max(n, 1))


def resolve_backend(flag: str, device) -> str:
    if flag != "auto":
        return flag
    return "nccl" if device.type == "cuda" else "gloo"


# ------------------------------------------------------------------ logging
def step_line(step, local_step, ms, py2=False):
    parts = ("Global step %d" % step, "Local step %d" % local_step, " AvgTime: %3.2fms" % ms)
    return repr(parts) if py2 else " ".join(parts)


def scalar_metrics(metrics) -> dict:
    """Float scalars of a step's metrics (``loss``; GAN ``gen_loss`` / ``disc_loss``) as Python
    floats - the loss values written to the events file and the --metrics_jsonl stream."""
    out = {}
    for k, v in (metrics or {}).items():
        if isinstance(v, ScaledScalar) or (torch.is_tensor(v) and v.numel() == 1 and v.is_floating_point()):
            out[k] = float(v.item())
    return out


def model_step_hook(model, step, metrics, log, ran=1):
    """``ran``: the steps the iteration ran (a multi-step replay); the line prints when any of their
    global steps is one it prints at, with the metrics of the last."""
    inc = getattr(model, "gs_increments", 1)
    if model.name == "gan" and any(s % 1000 == 0 or s == 1 for s in (step - k * inc for k in range(ran))):
        log("Step %i: Generator Loss: %f, Discriminator Loss: %f"
            % (step, float(metrics["gen_loss"].item()), float(metrics["disc_loss"].item())))


CNN_CLIP_ERROR = ("--clip_norm: the MNIST CNN's own schedule applies its fc and conv gradients in separate "
                  "Adam launches and sends its buckets from inside backward, so it cannot form one global norm "
                  "before its first update; pass --bucket_mb to run the CNN on the generic path, which clips")


CNN_RECIPE_ERROR = ("%s: the MNIST CNN's own schedule launches its Adam applies itself, with the learning rate as a "
                    "host argument; pass --bucket_mb to run the CNN on the generic path, which takes a schedule")
PS_RECIPE_ERROR = ("%s: learning-rate schedules, --weight_decay and --nesterov run in local and all-reduce mode "
                   "only - in --mode=ps the shards' optimizers own no global_step to evaluate a schedule from")


CNN_EMA_ERROR = ("%s: the MNIST CNN's own schedule launches its Adam applies itself, in parts; pass --bucket_mb to run "
                 "the CNN on the generic path, whose fused apply keeps the moving average")
PS_EMA_ERROR = ("%s: the moving average of the weights runs in local and all-reduce mode only - in --mode=ps the "
                "shards' applies write the workers' reply buffers and own no global_step")


CNN_LARS_ERROR = ("%s: the MNIST CNN's own schedule launches its Adam applies itself, in parts, before every gradient of "
                  "the step exists; pass --bucket_mb to run the CNN on the generic path, whose optimizer forms the "
                  "per-variable norms before its fused apply")
PS_LARS_ERROR = ("%s: layer-wise rate scaling runs in local and all-reduce mode only - in --mode=ps the shards apply a "
                 "push bucket by bucket and never hold a whole variable's gradient beside its weights")
MODEL_LARS_ERROR = ("%s: only a momentum model that declares its decaying variables takes layer-wise rate scaling "
                    "(resnet20: the conv and dense kernels are scaled, batch-norm variables and biases are not), not %r")


SPG_HOST_ERROR = ("--steps_per_graph %d: several steps per replay need --shuffle device - with --shuffle host the rows "
                  "of every batch are host indices, which cannot enter a replay")
PS_BATCHING_ERROR = ("%s: device-side shuffling and multi-step replays run in local and all-reduce mode only - a "
                     "--mode=ps worker's step is paced by its push / pull with the ps tasks")
CNN_SPG_ERROR = ("--steps_per_graph %d: the MNIST CNN's own schedule is captured one step per replay; pass --bucket_mb "
                 "to run the CNN on the generic path, which replays several")


PS_EVAL_ERROR = ("--eval_every %d: periodic evaluation runs in local and all-reduce mode only - a --mode=ps worker "
                 "holds the variables only between a pull and the next push")
MODEL_EVAL_ERROR = ("--eval_every %d: periodic evaluation needs a program with an inference forward to logits "
                    "(resnet20, resnet50), which model %r does not have")


def check_eval(flags, mode=None):
    """--eval_every against the mode, before anything is built.  (A model whose program cannot evaluate
    is refused where the program is built, run_allreduce.)"""
    if getattr(flags, "eval_every", 0) > 0 and mode == "ps":
        raise ValueError(PS_EVAL_ERROR % flags.eval_every)


def eval_metrics_row(res, topk, eval_ms) -> dict:
    """An evaluation's result as the keys of its --metrics_jsonl row."""
    return {"test_accuracy": res["accuracy"], "test_top%d" % topk: res["topk_accuracy"], "test_loss": res["loss"],
            "test_examples": res["examples"], "eval_ms": eval_ms}


@contextlib.contextmanager
def chief_untrained_vars(model, P, world, group=None):
    """Inside: the variables no optimizer updates (BatchNorm moving averages) hold rank 0's values on every
    rank; on exit each rank has its own back, bit for bit.  Synchronous replicas share their trained
    variables, but every rank's moving averages follow its own batches - evaluated with the chief's (the
    ones its checkpoints hold), all ranks report the same numbers.  One rank: nothing happens."""
    trained = {n for _cfg, vl, _bp in model.opt_groups for n in vl}
    views = [P.view(s.name) for s in model.specs if s.name not in trained] if world > 1 else []
    if not views:
        yield
        return
    own = torch.cat([v.reshape(-1) for v in views])
    chief = own.clone()
    dist.broadcast(chief, src=0, group=group)

    def put(flat):
        o = 0
        for v in views:
            v.copy_(flat[o:o + v.numel()].reshape(v.shape))
            o += v.numel()
    put(chief)
    try:
        yield
    finally:
        put(own)


def batching_flags(flags) -> list:
    """--shuffle / --steps_per_graph where they differ from their defaults, by name."""
    return (["--shuffle"] if getattr(flags, "shuffle", "host") != "host" else []) + \
        (["--steps_per_graph"] if getattr(flags, "steps_per_graph", 1) > 1 else [])


def check_batching(flags, mode=None):
    """--shuffle / --steps_per_graph against mode and each other, before anything is built.  (The MNIST
    CNN's own schedule is refused where that schedule is chosen, run_allreduce.)"""
    names = batching_flags(flags)
    if names and mode == "ps":
        raise ValueError(PS_BATCHING_ERROR % " ".join(names))
    if getattr(flags, "steps_per_graph", 1) > 1 and getattr(flags, "shuffle", "host") != "device":
        raise ValueError(SPG_HOST_ERROR % flags.steps_per_graph)


def check_recipe(flags, model, mode=None):
    """The optimizer-recipe flags against mode and model, before anything is built.  (The MNIST CNN's
    own schedule is refused where that schedule is chosen, run_allreduce - and after it, there, a model
    that cannot take --lars_eeta.)"""
    ema = flagmod.ema_flags(flags)
    if ema and mode == "ps":
        raise ValueError(PS_EMA_ERROR % " ".join(ema))
    lars = flagmod.lars_flags(flags)
    if lars and mode == "ps":
        raise ValueError(PS_LARS_ERROR % " ".join(lars))
    names = flagmod.recipe_flags(flags)
    if not names:
        return
    if mode == "ps":
        raise ValueError(PS_RECIPE_ERROR % " ".join(names))
    if (flags.weight_decay > 0 or flags.nesterov) and getattr(model, "decay_vars", None) is None:
        raise ValueError("%s: only a model that declares its decaying variables takes these (resnet20: the conv and "
                         "dense kernels), not %r" % (" ".join(n for n in names if n in ("--weight_decay", "--nesterov")),
                                                     getattr(model, "name", "")))


def apply_recipe(flags, cfg, model, var_list_):
    """The optimizer-recipe flags into the OptimizerConfig of one var list (validated by the Optimizer)."""
    cfg.lr_boundaries, cfg.lr_values = tuple(flags.lr_boundaries), tuple(flags.lr_values)
    cfg.lr_decay_steps, cfg.lr_end, cfg.lr_warmup_steps = flags.lr_decay_steps, flags.lr_end, flags.lr_warmup_steps
    if getattr(model, "decay_vars", None) is not None:
        cfg.weight_decay, cfg.nesterov = flags.weight_decay, bool(flags.nesterov)
        cfg.decay_vars = tuple(n for n in model.decay_vars if n in var_list_)


def apply_lars(flags, cfg, model, var_list_):
    """--lars_eeta / --lars_epsilon into the OptimizerConfig of one var list: the adaptive variables are the
    model's decaying ones, whose weight decay (--weight_decay, or none) enters the trust ratio."""
    cfg.lars_eeta, cfg.lars_epsilon = flags.lars_eeta, flags.lars_epsilon
    cfg.lars_vars = tuple(n for n in model.decay_vars if n in var_list_)


def trust_metrics(opts) -> dict:
    """The smallest and largest trust ratio of the step over the adaptive variables (``trust_min``,
    ``trust_max``), read from the device.  A host read: log steps only."""
    t = [o.layer_trust.cpu()[o.lars.index] for o in opts if o.lars is not None and o.lars.index]
    if not t:
        return {}
    t = torch.cat(t)
    return {"trust_min": float(t.min()), "trust_max": float(t.max())}


def lr_metrics(opts) -> dict:
    """The learning rate the step used, read from the device (``lr``; ``lr_<i>`` per scheduled
    optimizer of several).  A host read: log steps only."""
    s = [o for o in opts if o.current_lr is not None]
    if len(s) == 1:
        return {"lr": float(s[0].current_lr.item())}
    return {"lr_%d" % i: float(o.current_lr.item()) for i, o in enumerate(s)}


def ema_metrics(opts) -> dict:
    """The decay the step's moving average used, read from the device (``ema_decay``; ``ema_decay_<i>``
    per optimizer of several).  A host read: log steps only."""
    s = [o for o in opts if o.current_ema_decay is not None]
    if len(s) == 1:
        return {"ema_decay": float(s[0].current_ema_decay.item())}
    return {"ema_decay_%d" % i: float(o.current_ema_decay.item()) for i, o in enumerate(s)}


@contextlib.contextmanager
def averaged_weights(opts):
    """Inside: every optimizer's variables hold their moving averages (Optimizer.averaged); the trained
    values come back on exit.  Optimizers without one: nothing happens."""
    with contextlib.ExitStack() as st:
        for o in opts:
            if o.ema is not None:
                st.enter_context(o.averaged())
        yield


def clip_metrics(clips) -> dict:
    """The step's global gradient norms, read from the device: ``global_norm`` for a single optimizer,
    ``global_norm_<i>`` per optimizer of several (the GAN).  A host read: log steps only."""
    if len(clips) == 1:
        return {"global_norm": float(clips[0].norm.item())}
    return {"global_norm_%d" % i: float(c.norm.item()) for i, c in enumerate(clips)}


class MetricsLog:
    def __init__(self, path):
        self.f = open(path, "a") if path else None

    def write(self, **kw):
        if self.f:
            self.f.write(json.dumps(kw) + "\n")
            self.f.flush()


# ---------------------------------------------------------------- batching
def check_augment(augment: str, model):
    """--augment cifar is the CIFAR-10 recipe: only the CIFAR model (resnet20) takes it."""
    if augment != "none" and getattr(model, "name", "") != "resnet20":
        raise ValueError("--augment %s: the CIFAR-10 input transforms (32x32x3 crop / flip / channel statistics) "
                         "apply to --model resnet20 only, not to %r" % (augment, getattr(model, "name", "")))


def check_mix(mix: str, label_smoothing: float, augment: str):
    """--mix / --label_smoothing are written by the augmenting batch launch: they need --augment cifar."""
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError("--label_smoothing %g: must lie in [0, 1)" % label_smoothing)
    if augment == "none" and (mix != "none" or label_smoothing > 0):
        raise ValueError("--mix / --label_smoothing: the mixed images and soft label rows are written by the "
                         "augmenting batch launch, add --augment cifar (--model resnet20)")


class Feeder:
    """next batch for a program: host next_batch on CPU, HBM gather on GPU.

    ``augment`` ("none" / "cifar", the --augment flag): the CIFAR input transforms on every training
    batch - on GPUs inside the batcher's one launch, written straight into the program's input buffer;
    on CPU ``ops.augment_rows`` over the host batch.  The draws are seeded with the training set's
    seed (the per-rank data seed), and ``program.input_norm`` is set so that evaluation standardises too.

    ``shuffle`` ("host" / "device", the --shuffle flag): "device" draws the rows of every batch from a
    per-epoch permutation evaluated inside the batcher's one launch (``DeviceBatcher(sampling="device")``),
    so ``next()`` can be captured into the step graph; on CPU the same batcher runs on host tensors through
    the ops' mirrors.  ``seek(k)`` continues at batch k (device mode)."""

    def __init__(self, data, program, device, augment="none", shuffle="host", mix="none", label_smoothing=0.0):
        self.B = program.batch_size
        self.shuffle = shuffle
        self.dev = None
        self.aug = None
        check_mix(mix, label_smoothing, augment)
        if augment != "none":
            check_augment(augment, program.model)
            self.aug = dataclasses.replace(cifar.Augment.cifar(data.train.images_u8), mix=mix,
                                           label_smoothing=float(label_smoothing))
            self.stats = program.input_norm = self.aug.stats_on(device)
        if device.type == "cuda" or shuffle == "device":
            self.dev = DeviceBatcher(data.train, device, self.B, one_hot=True, augment=self.aug,
                                     out=program.x if self.aug is not None and device.type == "cuda" else None,
                                     sampling=shuffle)
        elif self.aug is not None:
            self.x = torch.empty(self.B, self.aug.H * self.aug.W * self.aug.C)
            self.y = torch.empty(self.B, data.train.num_classes)
            self.labels = torch.from_numpy(data.train.labels_int.astype(np.int32))
            self.ctr = torch.zeros(1, dtype=torch.int64)
            self.done = torch.zeros(1, dtype=torch.int32)
        self.data = data

    def seek(self, step: int):
        """Device mode: the next batch is batch ``step`` of the run (rows and crop / flip draws)."""
        if self.shuffle == "device":
            self.dev.seek(step)

    @property
    def epochs_completed(self):
        return self.dev.epochs_completed if self.dev is not None else self.data.train.epochs_completed

    def next(self):
        if self.dev is not None:
            return self.dev.next_batch()
        if self.aug is not None:
            a, train = self.aug, self.data.train
            idx = torch.from_numpy(train.next_batch_indices(self.B).astype(np.int32))
            ops.augment_rows(torch.from_numpy(train.images_u8), self.x, a.H, a.W, a.C, pad=a.pad, flip=a.flip,
                             mean=self.stats[0], inv_std=self.stats[1], idx=idx, labels_src=self.labels, seed=train.seed,
                             counter=self.ctr, done=self.done, onehot=self.y, mix=a.mix,
                             label_smoothing=a.label_smoothing)
            return self.x, self.y
        x, y = self.data.train.next_batch(self.B)
        return torch.from_numpy(x), torch.from_numpy(y)


# ---------------------------------------------------------- checkpoint glue
def var_list(model):
    shapes = model.tf_shapes()
    out = []
    for n in model.var_order:
        if n == model.gs_name:
            out.append((n, ckpt.DT_INT32, []))
        else:
            out.append((n, ckpt.DT_FLOAT, list(shapes[n])))
    return out


def tensors_from_flat(model, P, optimizers, gs: int):
    """Checkpoint dict (TF names and layouts) from a FlatParams + its optimizers."""
    out = {}
    for s in model.specs:
        if s.name in P.offsets:  # a ps shard holds a subset
            out[s.name] = model.to_tf(s.name, P.view(s.name).detach().cpu())
    for o in optimizers:
        for k, t in o.slot_tensors().items():
            base = k.rsplit("/", 1)[0]  # "<var>/Adam" -> "<var>"; beta powers have no slash
            if "/" in k and base in P.offsets:
                t = model.to_tf(base, t)
            out[k] = t
    out[model.gs_name] = torch.tensor(int(gs), dtype=torch.int32)
    return out


def load_flat_from_tensors(model, P, optimizers, tensors):
    for s in model.specs:
        if s.name in tensors and s.name in P.offsets:
            P.view(s.name).copy_(model.from_tf(s.name, tensors[s.name]).reshape(s.shape).to(P.device))
    conv = {}
    for k, t in tensors.items():
        if "/" in k:
            base = k.rsplit("/", 1)[0]
            if base in P.offsets:
                t = model.from_tf(base, t)
        conv[k] = t
    for o in optimizers:
        o.load_slot_tensors(conv)
    P.refresh_copies()
    return int(tensors.get(model.gs_name, torch.tensor(0)).item())


# --------------------------------------------------------------------- ps
def _shard_layout(model, num_ps):
    placement = round_robin(model.var_order, num_ps)
    shard_specs = {k: [s for s in model.specs if placement[s.name] == k] for k in range(num_ps)}
    return placement, shard_specs


def ps_view(flags, model):
    """The model as the ps tasks see it: with --ps_partition_mb, large variables split into
    partitions that are placed (and checkpointed) like TF's PartitionedVariable parts."""
    mb = getattr(flags, "ps_partition_mb", 0.0) or 0.0
    return PartitionedModel(model, int(mb * (1 << 20))) if mb > 0 else model


def run_ps(flags, model, server, device, log):
    model = ps_view(flags, model)
    placement, shard_specs = _shard_layout(model, len(server.cluster.ps))
    k = server.task_index
    gs_here = placement[model.gs_name] == k
    shard = Shard(shard_specs[k], model.opt_groups, device, gs_here, model.gs_increments)
    comm = "cpu" if server.backend == "gloo" else device
    hb = Heartbeat(server.store, "ps", k, flags.heartbeat_secs)
    wd = Watchdog(server.store, [("worker", i) for i in range(len(server.cluster.worker))],
                  flags.heartbeat_timeout) if flags.heartbeat_secs > 0 else None
    ps = PSServer(server, shard, num_workers=flags.workers, sync=flags.sync,
                  replicas_to_aggregate=flags.replicas_to_aggregate, hogwild=flags.hogwild, comm_device=comm,
                  log=log, watchdog=wd, faults=FaultInjector("ps", k, log=log))
    if _native_ps(flags, server, device):
        ps.native = ps_native.NativeShardService(server, shard, len(server.cluster.worker), sync=flags.sync,
                                                 replicas_to_aggregate=flags.replicas_to_aggregate,
                                                 hogwild=flags.hogwild)
    ps.serve_forever()
    if ps.native is not None:
        st = ps.native.stats()
        log("ps %d: native data plane: %d requests, %d applies (%d bucket applies during backward), %d stale"
            % (k, st["requests"], st["applies"], st["bucket_applies"], st["stale"]))
        ps.native.stop()
    hb.stop()
    if ps.lost:
        # service threads of lost workers are blocked in recv: leave without the collective teardown
        sys.stdout.flush()
        os._exit(0)
    # The ps hosts the TCPStore and owns nothing the job still needs once every worker has
    # said done (checkpoints are the chief's).  Tear the process groups down, then leave
    # without interpreter finalisation: static destructors of the communicator / store
    # threads racing the workers' own teardown end in std::terminate on a ROCm box.
    server.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def _native_ps(flags, server, device) -> bool:
    """Whether the ps roles move PUSH / PULL over the native single-node data plane."""
    if flags.ps_transport == "pg":
        return False
    ok = ps_native.eligible(server, device)
    if flags.ps_transport == "native" and not ok:
        raise SystemExit("--ps_transport=native needs every task on this host, on GPUs")
    return ok


def ps_state(client, model, shard_specs, placement):
    """Gather every shard's params + slots from the ps tasks into one TF-named dict (partitioned
    variables: one ``ckpt.Sliced`` per variable / slot)."""
    states, gs = client.fetch_state()
    out = {}
    for k, flat in states.items():
        mirror = Shard(shard_specs[k], model.opt_groups, "cpu", False, model.gs_increments)
        mirror.load_state_payload(flat)
        out.update(tensors_from_flat(model, mirror.P, mirror.opts, gs))
    out[model.gs_name] = torch.tensor(int(gs), dtype=torch.int32)
    if isinstance(model, PartitionedModel):
        out = model.merge_tf(out)
    return out, gs


def ps_restore(client, model, shard_specs, tensors):
    states = {}
    gs = int(tensors.get(model.gs_name, torch.tensor(0)).item())
    if isinstance(model, PartitionedModel):
        tensors = model.split_tf(tensors)
    for k, specs in shard_specs.items():
        if not specs:
            continue
        mirror = Shard(specs, model.opt_groups, "cpu", False, model.gs_increments)
        load_flat_from_tensors(model, mirror.P, mirror.opts, tensors)
        states[k] = mirror.state_payload()
    client.set_state(states, gs)


def run_worker_ps(flags, model, server, device, log):
    cl = server.cluster
    full_model, model = model, ps_view(flags, model)
    placement, shard_specs = _shard_layout(model, len(cl.ps))
    gs_rank = cl.rank_of("ps", placement[model.gs_name])
    prog = full_model.program(device, flags.batch_size, seed=flags.seed)
    # --clip_norm: the worker clips before it pushes, as TF does (the ps applies what it receives):
    # one global norm per minimize call over its var list, then the gradient scaled in place
    clips = []
    if flags.clip_norm > 0:
        if hasattr(getattr(prog, "core", None), "allreduce") and flags.bucket_mb is None:
            raise ValueError(CNN_CLIP_ERROR)
        clips = [GlobalNormClip(prog.P, vl, flags.clip_norm) for _cfg, vl, _bp in full_model.opt_groups]

    def clip_grads():
        for c in clips:
            c.compute()
            c.scale_grad()

    if isinstance(model, PartitionedModel):
        model.add_aliases(prog.P)  # the parts as views of the worker's full variables
    comm = "cpu" if server.backend == "gloo" else device
    client = PSClient(server, prog.P, placement, shard_specs, gs_rank, model.opt_groups, comm_device=comm)
    is_chief = server.task_index == 0
    sv = Supervisor(
        is_chief, flags.model_dir,
        state_fn=lambda: ps_state(client, model, shard_specs, placement),
        restore_fn=lambda t: ps_restore(client, model, shard_specs, t),
        init_fn=client.init_variables,
        wait_fn=lambda: wait_for_init(client),
        var_list_fn=lambda: var_list(model),
        gs_fn=lambda: client.status()[1],
        save_model_secs=flags.save_model_secs, save_summaries_secs=flags.save_summaries_secs,
        max_to_keep=flags.max_to_keep, log=log)
    data = read_data_sets(model, "" if flags.synthetic else flags.data_dir, one_hot=True,
                          seed=flags.seed * 1000 + server.task_index + 1, log=log)
    feeder = Feeder(data, prog, device, augment=flags.augment, mix=flags.mix, label_smoothing=flags.label_smoothing)
    metrics_log = MetricsLog(flags.metrics_jsonl)
    hb = Heartbeat(server.store, "worker", server.task_index, flags.heartbeat_secs)
    faults = FaultInjector("worker", server.task_index, log=log)
    begin_time = time.time()
    sv.prepare()
    if flags.reinit_on_join:
        # GAN:181 / ENC:160: every worker re-runs init, clobbering restore + progress
        prog.P.initialize(flags.seed)
        client.init_variables()
    link = None
    if _native_ps(flags, server, device):
        # gradient buckets in backward-completion order (flat order = the order backward produces them)
        link = ps_native.NativePSLink(server, prog.P, placement, shard_specs, placement[model.gs_name], device,
                                      buckets=_ps_buckets(prog, flags.bucket_mb))
        core = getattr(prog, "core", None)
        if clips:
            pass                        # clipping: every bucket is pushed after the scaling (end_step)
        elif core is not None and hasattr(core, "allreduce"):
            core.allreduce = link       # the CNN program pushes its buckets from inside backward
        elif hasattr(prog, "grad_ready"):
            prog.grad_ready = link.ready
    state = {}

    def native_step():
        state["m"] = prog.compute_grads()
        clip_grads()
        link.end_step()    # push what backward has not pushed yet, request / wait / pull

    runner = StepGraph(native_step, warmup=2, capture_error_mode="thread_local",
                       enabled=link is not None and flags.hip_graph) if link is not None else None
    if link is not None:
        link.pull()
    else:
        client.pull()
    step = 0
    local_step = 0
    try:
        while not sv.should_stop() and step < flags.num_steps:
            t0 = time.time()
            prog.load_batch(feeder.next())
            if link is not None:
                runner()
                link.note_request()
                step = link.host_reply()
                metrics = state.get("m")
                if local_step % flags.log_every == 0:
                    link.check()
                    prog.check_health()
            else:
                metrics = prog.compute_grads()
                clip_grads()
                step = client.push_pull(prog.P.grad)
            if flags.check_pull:
                log("pull checksum gs=%d: %.9e" % (step, float(prog.P.master.double().sum().item())))
                log("pull l2norm gs=%d: %.9e" % (step, float(prog.P.master.double().norm().item())))
            faults.step(step)
            elapsed = time.time() - t0
            ips = prog.batch_size / max(elapsed, 1e-9)
            sc = scalar_metrics(metrics)
            if local_step % flags.log_every == 0:
                if clips:
                    sc.update(clip_metrics(clips))
                log(step_line(step, local_step, elapsed * 1000, flags.py2_print))
                sv.summary(step, dict(sc, **{"images/sec": ips}))
            model_step_hook(model, step, metrics, log)
            metrics_log.write(step=local_step, gs=step, ms=elapsed * 1000, images_per_sec=ips, **sc)
            local_step += 1
        log("Total Time: %3.2fs" % float(time.time() - begin_time))
        if model.name in ("lstm", "cnn"):
            link.pull() if link is not None else client.pull()
            test_len = 128
            acc = prog.evaluate(torch.from_numpy(data.test.images[:test_len]).to(device),
                                torch.from_numpy(data.test.labels[:test_len]).to(device))
            log("Test-Accuracy: %2.4f" % acc)
        # the chief's checkpoint / step-counter threads talk to the ps: join them before the done
        # message (the last done makes the ps quit, and a save started after it fails on a closed
        # connection)
        sv.stop()
        client.done()
    finally:
        hb.stop()
        sv.stop()
        if link is not None:
            link.close()


# --------------------------------------------------------------- allreduce
def run_allreduce(flags, model, device, log, world=1, rank=0, group=None, store=None):
    check_recipe(flags, model)
    check_batching(flags)
    recipe = flagmod.recipe_flags(flags)
    ema = flagmod.ema_flags(flags)
    lars = flagmod.lars_flags(flags)
    spg = max(1, int(getattr(flags, "steps_per_graph", 1)))
    dev_shuffle = getattr(flags, "shuffle", "host") == "device"
    prog = model.program(device, flags.batch_size, seed=flags.seed)
    eval_every = max(0, int(getattr(flags, "eval_every", 0)))
    if eval_every and not device_eval.supports(prog):
        raise ValueError(MODEL_EVAL_ERROR % (eval_every, getattr(model, "name", "")))
    # programs with their own data-parallel schedule (the MNIST CNN: the one bench.py times) run it
    # here too, unless --bucket_mb asks for generic flat-buffer buckets (a single process: only together
    # with --clip_norm, a recipe flag, --ema_decay, --lars_eeta or --steps_per_graph > 1, which that schedule cannot do)
    native = (hasattr(prog, "attach_data_parallel") and len(model.opt_groups) == 1
              and (flags.bucket_mb is None or (world == 1 and not flags.clip_norm > 0 and not recipe and not ema
                                               and not lars and spg == 1)))
    if native and flags.clip_norm > 0:
        raise ValueError(CNN_CLIP_ERROR)
    if native and spg > 1:
        raise ValueError(CNN_SPG_ERROR % spg)
    if native and recipe:
        raise ValueError(CNN_RECIPE_ERROR % " ".join(recipe))
    if native and ema:
        raise ValueError(CNN_EMA_ERROR % " ".join(ema))
    if native and lars:
        raise ValueError(CNN_LARS_ERROR % " ".join(lars))
    if lars and (getattr(model, "decay_vars", None) is None
                 or any(cfg.kind != "momentum" for cfg, _vl, _bp in model.opt_groups)):
        raise ValueError(MODEL_LARS_ERROR % (" ".join(lars), getattr(model, "name", "")))
    gstep = torch.zeros(1, dtype=torch.int32, device=device)
    opts = []
    for i, (cfg, var_list_, bp) in enumerate(model.opt_groups):
        cfg.lr = flags.learning_rate if flags.learning_rate is not None else cfg.lr
        cfg.clip_norm = flags.clip_norm
        if recipe:
            apply_recipe(flags, cfg, model, var_list_)
        if ema:
            cfg.ema_decay, cfg.ema_num_updates = flags.ema_decay, bool(flags.ema_num_updates)
        if lars:
            apply_lars(flags, cfg, model, var_list_)
        opts.append(Optimizer(cfg, prog.P, var_list=var_list_, global_step=gstep, beta_power_names=bp))
    is_chief = rank == 0
    # held while the variables hold their moving averages (an evaluation with --ema_decay): the checkpoint
    # thread saves the trained values, never the swapped ones
    weights_lock = threading.Lock()

    def state_fn():
        with weights_lock:
            return tensors_from_flat(model, prog.P, opts, int(gstep.item())), int(gstep.item())

    sv = Supervisor(
        is_chief, flags.model_dir,
        state_fn=state_fn,
        restore_fn=lambda t: gstep.fill_(load_flat_from_tensors(model, prog.P, opts, t)),
        init_fn=lambda: None, wait_fn=lambda: None, var_list_fn=lambda: var_list(model),
        gs_fn=lambda: int(gstep.item()),
        save_model_secs=flags.save_model_secs, save_summaries_secs=flags.save_summaries_secs,
        max_to_keep=flags.max_to_keep, log=log)
    sv.prepare()
    ar = None
    clips = [o.clip for o in opts if o.clip is not None]
    if world > 1:
        # chief's (possibly restored) state is the starting point of every replica
        dist.broadcast(prog.P.master, src=0, group=group)
        dist.broadcast(gstep, src=0, group=group)
        for o in opts:
            for b in (o.s1, o.s2, o.beta_pow, o.ema):
                if b is not None:
                    dist.broadcast(b, src=0, group=group)
        prog.P.refresh_copies()
        # on GPUs the buckets go through dtfe's own RCCL communicator (capturable: the whole step,
        # all-reduce included, replays as one hipGraph); gloo / CPU keeps ProcessGroup collectives
        bks = prog.core.buckets if native else _buckets(prog.P, flags.bucket_mb)
        comm = None
        # (gloo + --comm=ipc: several ranks sharing one GPU rehearse the in-graph IPC path)
        if device.type == "cuda" and flags.comm != "pg" and (dist.get_backend(group) != "gloo" or flags.comm == "ipc"):
            cdt = torch.bfloat16 if flags.comm_dtype == "bf16" else torch.float32
            comm = make_comm(device, group, [(hi - lo) * (2 if cdt == torch.bfloat16 else 4) for lo, hi in bks], cdt,
                             mode=flags.comm, log=log if is_chief else None,
                             timeout_s=flags.heartbeat_timeout if flags.heartbeat_secs > 0 else 30.0)
        ar = BucketAllReduce(prog.P.grad, bks, group=group, comm=comm,
                             comm_dtype=torch.bfloat16 if flags.comm_dtype == "bf16" else torch.float32)
        if not native and hasattr(prog, "grad_ready"):  # programs reporting backward progress overlap the all-reduce
            prog.grad_ready = ar.ready
    if native:
        prog.attach_data_parallel(ar, opts[0])
    data = read_data_sets(model, "" if flags.synthetic else flags.data_dir, one_hot=True, seed=flags.seed * 1000 + rank + 1,
                          log=log if is_chief else (lambda *_: None))
    feeder = Feeder(data, prog, device, augment=flags.augment, shuffle="device" if dev_shuffle else "host", mix=flags.mix,
                    label_smoothing=flags.label_smoothing)
    # --shuffle device: rows and crop / flip draws are functions of the batch number, so a restored run
    # (the chief's state, broadcast above) continues the epoch order and the augmentation stream
    feeder.seek(int(gstep.item()) // model.gs_increments)
    metrics_log = MetricsLog(flags.metrics_jsonl)
    # --eval_every: the test split resident on the device, built after the feeder (which sets the program's
    # input statistics); every rank evaluates the whole set, with the chief's BatchNorm moving averages
    # (chief_untrained_vars) - the trained variables are the same on every replica, so the lines agree
    evaluator = None
    if eval_every:
        evaluator = device_eval.DeviceEvaluator(prog, data.test.images_u8, data.test.labels_int, topk=flags.eval_topk,
                                                examples=flags.eval_examples, graph=flags.hip_graph)
        prog.evaluator = evaluator  # (tests and tools read .graph / .capture_error)

    def evaluate(step):
        """One evaluation at global step ``step``: the log line, the chief's summaries, the metrics keys."""
        t_ev = time.time()
        with chief_untrained_vars(model, prog.P, world, group):
            if ema:  # --ema_decay: the averaged weights are what is evaluated
                with weights_lock:
                    with averaged_weights(opts):
                        res = evaluator.run()
                    if device.type == "cuda":  # the trained values are back before the lock is
                        torch.cuda.current_stream(device).synchronize()
            else:
                res = evaluator.run()
        row = eval_metrics_row(res, evaluator.topk, (time.time() - t_ev) * 1000)
        if ema:
            row["eval_weights"] = "ema"
        log("Global step %d Test-Accuracy%s: %2.4f Test-Loss: %.4f"
            % (step, "(EMA)" if ema else "", res["accuracy"], res["loss"]))
        sv.summary(step, {k: v for k, v in row.items() if k not in ("test_examples", "eval_weights")})
        return row

    state = {}
    trace = flags.trace_json if world == 1 or not flags.trace_json else \
        flags.trace_json.replace(".json", "") + ".rank%d.json" % rank
    timer = PhaseTimer(device, trace_path=trace or None, rank=rank) \
        if (flags.phase_timers or flags.trace_json) else None
    phase = timer.phase if timer else (lambda _n: contextlib.nullcontext())
    faults = FaultInjector("worker", rank, log=log)
    # failure detection, on by default in this mode (utils/flags.py resolve_mode): every
    # rank beats into the TCPStore and a watchdog thread aborts the collectives and ends this rank when
    # a peer goes silent (or never beats) / the store vanishes / RCCL reports an error - the step graph
    # itself would wait on a dead peer forever
    hb = wd = None
    if world > 1 and store is not None and flags.heartbeat_secs > 0:
        hb = Heartbeat(store, "worker", rank, flags.heartbeat_secs)
        wd = CommWatchdog(store, "worker", rank, world, comm=ar.comm if ar is not None else None,
                          interval=min(1.0, flags.heartbeat_secs), timeout=flags.heartbeat_timeout, log=log)

    def train_step():
        if dev_shuffle:  # the batch draw is one launch off the feeder's device counter: part of the captured step
            prog.load_batch(feeder.next())
        if native:  # forward, backward, overlapped all-reduce and Adam in the program's own order
            with phase("step"):
                state["m"] = prog.train_step(grad16=ar.grad16 if ar is not None else None, gscale=1.0 / world)
            return
        with phase("fwd+bwd"):
            state["m"] = prog.compute_grads()
        g16 = None
        if ar is not None:
            with phase("comm"):
                ar.flush()
                ar.wait()
            g16 = ar.grad16
        with phase("apply"):
            # every minimize op of the step in one (grouped) launch; gs advances once per step by gs_increments
            Optimizer.step_all(opts, [model.gs_increments if i == len(opts) - 1 else 0 for i in range(len(opts))],
                               grad16=g16, gscale=1.0 / world)

    # one step per replay, or --steps_per_graph of them (and single-step replays for a remainder)
    runner = MultiStepGraph(train_step, spg, warmup=2, capture_error_mode="thread_local",
                            enabled=(device.type == "cuda" and (world == 1 or ar.comm is not None) and flags.hip_graph
                                     and timer is None))
    prog.step_runner = runner  # (tests and tools read .graph / .capture_error)
    begin_time = time.time()
    step = int(gstep.item())
    local_step = 0
    capture_error_logged = graph_logged = evaluated = False
    try:
        while not sv.should_stop() and step < flags.num_steps:
            t0 = time.time()
            # never past --num_steps: a whole S-step replay only while S steps remain (each advances
            # global_step by gs_increments), else one step; the graphs capture themselves on the way
            left = -(-(flags.num_steps - step) // model.gs_increments)
            if not dev_shuffle:
                prog.load_batch(feeder.next())
            if runner.many is not None and left >= spg:
                runner.many()
                ran = spg
            else:
                runner.one()
                ran = 1
            if spg > 1 and not graph_logged and runner.many.graph is not None:
                graph_logged = True
                log("hip_graph: captured %d steps per replay" % spg)
            if runner.capture_error is not None and not capture_error_logged:
                capture_error_logged = True  # the step runs on, eagerly: say so once
                log("capture_error: %s: %s; continuing with eager launches"
                    % (type(runner.capture_error).__name__, runner.capture_error))
            step = int(gstep.item())
            faults.step(step)
            elapsed = (time.time() - t0) / ran
            ips = prog.batch_size * world / max(elapsed, 1e-9)
            sc = scalar_metrics(state.get("m"))
            # a log step: a multiple of --log_every lies among the local steps this replay ran
            log_step = (local_step + ran - 1) // flags.log_every > (local_step - 1) // flags.log_every
            if clips and log_step:
                sc.update(clip_metrics(clips))  # (the all-reduce has completed before step_all: every rank's norm)
            if recipe and log_step:
                sc.update(lr_metrics(opts))
            if ema and log_step:
                sc.update(ema_metrics(opts))
            if lars and log_step:
                sc.update(trust_metrics(opts))
            if local_step == 0 and native and ar is not None and is_chief:
                log("schedule: " + " < ".join(prog.core.schedule))
            if log_step:
                if dev_shuffle:
                    sc["epoch"] = feeder.epochs_completed
                log(step_line(step, local_step + ran - 1, elapsed * 1000, flags.py2_print))
                if timer is not None:
                    log(PhaseTimer.format(timer.summary()))
                sv.summary(step, dict(sc, **{"images/sec": ips}))
                if ar is not None and ar.comm is not None:
                    ar.comm.check_health()  # IPC barrier timeouts fail the job on every rank
                prog.check_health()
            if "m" in state:
                model_step_hook(model, step, state["m"], log, ran)
            # an evaluation step: a multiple of --eval_every lies among the model steps this replay ran, or
            # training ends here (elapsed was taken above: the step's ms excludes the evaluation)
            evaluated = False
            if evaluator is not None:
                ms_ = step // model.gs_increments
                if ms_ // eval_every > (ms_ - ran) // eval_every or step >= flags.num_steps:
                    sc.update(evaluate(step))
                    evaluated = True
            # one line per replay: the replay's last step, ms = replay time / steps run
            metrics_log.write(step=local_step + ran - 1, gs=step, ms=elapsed * 1000, images_per_sec=ips,
                              **(dict(sc, steps=ran) if spg > 1 else sc))
            local_step += ran
        if evaluator is not None and not evaluated:  # (stopped early, or nothing left to train)
            evaluate(step)
        if wd is not None:  # training is over: peers may now leave at their own pace
            wd.stop()
            _leave_watchdog(store, rank, world, flags.heartbeat_timeout)
        if ar is not None and ar.comm is not None:
            ar.comm.check_health()
        prog.check_health()
        log("Total Time: %3.2fs" % float(time.time() - begin_time))
        if world > 1 and flags.check_pull:  # synchronous replicas: identical parameters on every worker
            log("params checksum %.12e" % float(prog.P.master.double().sum().item()))
        if model.name in ("lstm", "cnn"):  # every worker evaluates and prints, as LSTM:134-138
            test_len = 128
            acc = prog.evaluate(torch.from_numpy(data.test.images[:test_len]).to(device),
                                torch.from_numpy(data.test.labels[:test_len]).to(device))
            log("Test-Accuracy: %2.4f" % acc)
            if ema:  # the same examples with the averaged weights
                with weights_lock:
                    with averaged_weights(opts):
                        acc = prog.evaluate(torch.from_numpy(data.test.images[:test_len]).to(device),
                                            torch.from_numpy(data.test.labels[:test_len]).to(device))
                    if device.type == "cuda":
                        torch.cuda.current_stream(device).synchronize()
                log("EMA Test-Accuracy: %2.4f" % acc)
    finally:
        if wd is not None:
            wd.stop()
        if hb is not None:
            hb.stop()
        if timer is not None:
            timer.close()
        sv.stop()
    return prog, opts, gstep


def _leave_watchdog(store, rank, world, timeout_s):
    """End of training with the comm watchdog on: the TCPStore lives in rank 0's process, so rank 0
    waits (bounded) until every rank has stopped its watchdog before it can exit - a peer still
    polling would otherwise read the vanished store as a failure.
    The counter is never reset: a store reused by a later run (tests, an in-process rerun) keeps
    counting, and each rank's own ticket tells which run it belongs to - every rank adds exactly
    once per run and a run cannot start before all ranks left the previous one - so rank 0 waits
    for the end of ITS run's group of `world` tickets."""
    key = "dtfe/hb/watchdogs_stopped"
    ticket = store.add(key, 1)
    if rank != 0:
        return
    target = ((ticket - 1) // world + 1) * world
    t_end = time.time() + timeout_s
    while store.add(key, 0) < target and time.time() < t_end:
        time.sleep(0.01)


def _ps_buckets(prog, bucket_mb=None):
    """Push buckets of a ps-mode worker: the program's own (the CNN's [head + fc1], [convs]) unless
    --bucket_mb is given, else ranges of the flat buffer, back to front."""
    core = getattr(prog, "core", None)
    if bucket_mb is None and core is not None and getattr(core, "buckets", None):
        return core.buckets
    return _buckets(prog.P, bucket_mb)


def _buckets(P, bucket_mb=None):
    """Contiguous gradient buckets of ``bucket_mb`` MB of fp32 gradient (default
    comm.DEFAULT_BUCKET_MB), back of the flat buffer first = backward-completion order."""
    from .parallel.comm import DEFAULT_BUCKET_MB

    mb = DEFAULT_BUCKET_MB if bucket_mb is None else float(bucket_mb)
    if mb <= 0:
        raise ValueError("--bucket_mb must be > 0")
    bucket_elems = max(1024, int(mb * (1 << 20)) // 4)
    total = P.total
    b = []
    hi = total
    while hi > 0:
        lo = max(0, hi - bucket_elems)
        b.append((lo, hi))
        hi = lo
    return b


# ------------------------------------------------------------------- entry
def run(model_name: str, argv=None, log=_print):
    cls, lr = MODELS[model_name]
    m0 = cls()
    flags = flagmod.parse(argv, model_defaults=dict(batch_size=m0.default_batch, num_steps=m0.default_steps,
                                                    learning_rate=lr), prog="distributed_%s.py" % model_name)
    model = cls(lr=flags.learning_rate)
    try:
        model.set_dtype(flags.dtype)  # --dtype: the model's program must implement it (no silent fallback)
    except ValueError as e:
        raise SystemExit(str(e))
    check_augment(flags.augment, model)
    check_mix(flags.mix, flags.label_smoothing, flags.augment)
    torch.manual_seed(flags.seed)
    np.random.seed(flags.seed)
    mode = flagmod.resolve_mode(flags)  # (+ mode-dependent defaults: --heartbeat_secs)
    check_recipe(flags, model, mode)
    check_batching(flags, mode)
    check_eval(flags, mode)
    local_rank = int(os.environ.get("LOCAL_RANK", flags.task_index if flags.job_name == "worker" else 0))
    device = resolve_device(flags.device, local_rank)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    backend = resolve_backend(flags.backend, device)
    if mode == "local":
        run_allreduce(flags, model, device, log)
        return 0
    cluster = ClusterSpec.from_flags(flags.ps_hosts, flags.worker_hosts)
    if mode == "ps":
        if not cluster.ps:
            raise SystemExit("--mode=ps needs --ps_hosts")
        server = Server(cluster, flags.job_name, flags.task_index, backend=backend,
                        device=device if backend == "nccl" else None)
        try:
            if flags.job_name == "ps":
                run_ps(flags, model, server, device, log)
            elif flags.job_name == "worker":
                run_worker_ps(flags, model, server, device, log)
            else:
                raise SystemExit("--job_name must be 'ps' or 'worker'")
        finally:
            server.shutdown()
        return 0
    # ring all-reduce: workers only
    if flags.job_name == "ps":
        log("ps %d: nothing to serve in --mode=allreduce; quitting" % flags.task_index)
        return 0
    cluster = ClusterSpec([], cluster.worker)
    server = Server(cluster, "worker", flags.task_index, backend=backend,
                    device=device if backend == "nccl" else None)
    try:
        run_allreduce(flags, model, device, log, world=cluster.world_size, rank=server.rank, store=server.store)
    finally:
        server.shutdown()
    return 0


def main(model_name: str):
    sys.exit(run(model_name, sys.argv[1:]))
