"""Command-line flags.

The eight reference flags keep their names, defaults and absl/gflags syntax
(``--task_index=1`` or ``--task_index 1``; ``--sync``/``--nosync`` for bools):

    --ps_hosts ""  --worker_hosts ""  --job_name ""  --task_index 0
    --data_dir /data_dir  --model_dir /tmp/checkpoints  --workers 3  --ps 1

(``--ps`` is accepted and ignored, exactly as the reference never reads it.)
The reference's hard-coded hyper-parameters become flags whose defaults are
the reference values (per model), and the north-star additions are opt-in.
"""
from __future__ import annotations

import argparse


def _bool(v):
    if isinstance(v, bool):
        return v
    return str(v).lower() in ("1", "true", "yes", "y", "t")


def _int_list(v):
    return tuple(int(x) for x in str(v).split(",") if x.strip())


def _float_list(v):
    return tuple(float(x) for x in str(v).split(",") if x.strip())


def recipe_flags(flags) -> list:
    """The optimizer-recipe flags (learning-rate schedule, weight decay, Nesterov) that are set, by name."""
    names = ("lr_boundaries", "lr_values", "lr_decay_steps", "lr_warmup_steps", "weight_decay", "nesterov")
    return ["--" + n for n in names if getattr(flags, n, None)]


def ema_flags(flags) -> list:
    """The moving-average flags (--ema_decay, --ema_num_updates) that are set, by name."""
    return ["--" + n for n in ("ema_decay", "ema_num_updates") if getattr(flags, n, None)]


def lars_flags(flags) -> list:
    """The layer-wise scaling flags (--lars_eeta, --lars_epsilon) that are set, by name."""
    return ["--" + n for n in ("lars_eeta", "lars_epsilon") if getattr(flags, n, None)]


def add_bool(ap, name, default, help_):
    ap.add_argument("--" + name, dest=name, nargs="?", const=True, default=default, type=_bool, help=help_)
    ap.add_argument("--no" + name, dest=name, action="store_false", help=argparse.SUPPRESS)


# --heartbeat_secs default of --mode=allreduce: a survivor's watchdog aborts the collectives and exits
# non-zero --heartbeat_timeout seconds after a peer's last beat (parallel/health.py CommWatchdog)
AR_HEARTBEAT_SECS = 1.0


def resolve_mode(flags) -> str:
    """The run mode (explicit --mode, else ps when --ps_hosts is set, else allreduce when
    --worker_hosts is, else local) with the mode-dependent defaults filled in: --heartbeat_secs
    (None -> AR_HEARTBEAT_SECS for allreduce, 0 otherwise)."""
    mode = flags.mode or ("ps" if flags.ps_hosts else ("allreduce" if flags.worker_hosts else "local"))
    if flags.heartbeat_secs is None:
        flags.heartbeat_secs = AR_HEARTBEAT_SECS if mode == "allreduce" else 0.0
    return mode


def build_parser(model_defaults: dict | None = None, prog=None):
    d = dict(batch_size=None, num_steps=None, learning_rate=None)
    if model_defaults:
        d.update(model_defaults)
    ap = argparse.ArgumentParser(prog=prog, allow_abbrev=False)
    # ---- reference flags (GAN:31-45)
    ap.add_argument("--ps_hosts", default="", help="Comma-separated list of hostname:port pairs")
    ap.add_argument("--worker_hosts", default="", help="Comma-separated list of hostname:port pairs")
    ap.add_argument("--job_name", default="", help="One of 'ps', 'worker'")
    ap.add_argument("--task_index", type=int, default=0, help="Index of task within the job")
    ap.add_argument("--data_dir", default="/data_dir", help="Directory for storing mnist data")
    ap.add_argument("--model_dir", default="/tmp/checkpoints", help="Directory for storing the checkpoints")
    ap.add_argument("--workers", type=int, default=3, help="Number of workers")
    ap.add_argument("--ps", type=int, default=1, help="Number of ps (unused, as in the reference)")
    # ---- reference hyper-parameters as flags (defaults = C02 per model)
    ap.add_argument("--batch_size", type=int, default=d["batch_size"])
    ap.add_argument("--num_steps", type=int, default=d["num_steps"], help="global-step budget (training_steps)")
    ap.add_argument("--learning_rate", type=float, default=d["learning_rate"])
    # ---- lifecycle
    ap.add_argument("--save_model_secs", type=float, default=60.0)
    ap.add_argument("--save_summaries_secs", type=float, default=120.0)
    ap.add_argument("--max_to_keep", type=int, default=5)
    # ---- north-star / framework additions
    ap.add_argument("--mode", choices=["ps", "allreduce", "local"], default=None,
                    help="ps: between-graph parameter server (reference); allreduce: ring all-reduce DP; "
                         "local: single process. Default: ps when --ps_hosts is set, else allreduce/local")
    add_bool(ap, "sync", False, "sync SGD with a chief (SyncReplicasOptimizer semantics) in ps mode")
    ap.add_argument("--replicas_to_aggregate", type=int, default=None)
    ap.add_argument("--device", choices=["auto", "cpu", "cuda"], default="auto")
    ap.add_argument("--backend", choices=["auto", "gloo", "nccl"], default="auto")
    ap.add_argument("--seed", type=int, default=0)
    add_bool(ap, "hogwild", False, "lock-free ps updates (TF use_locking=False race)")
    add_bool(ap, "reinit_on_join", False, "every worker re-runs init (GAN:181 / ENC:160 quirk)")
    add_bool(ap, "py2_print", False, "print the Python-2 tuple form of the LSTM step line (LSTM:130)")
    add_bool(ap, "synthetic", False, "force synthetic MNIST-shaped data")
    add_bool(ap, "hip_graph", True, "capture the per-step kernels into a hipGraph (GPU)")
    ap.add_argument("--log_every", type=int, default=1, help="print the per-step line every N local steps")
    ap.add_argument("--comm_dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--bucket_mb", type=float, default=None,
                    help="all-reduce bucket size in MB of fp32 gradient (default: the model's own buckets - the "
                         "MNIST CNN's [head + fc1] / [convs] - else parallel/comm.py DEFAULT_BUCKET_MB); > 0")
    ap.add_argument("--dtype", choices=["auto", "fp32", "bf16"], default="auto",
                    help="compute dtype: fp32 = exact-fp32 MFMA kernels and fp32 activations (the reference's "
                         "precision), bf16 = bf16 MFMA with fp32 accumulation / masters; auto = the model's default. "
                         "GAN / autoencoder / LSTM / softmax: fp32 only; CNN: bf16 (default) or fp32; ResNets: bf16")
    ap.add_argument("--comm", choices=["auto", "rccl", "ipc", "pg"], default="auto",
                    help="all-reduce engine on GPUs: auto = faster of RCCL / hipIpc two-shot per bucket size "
                         "(both in-graph); pg = torch.distributed ProcessGroupNCCL (eager)")
    ap.add_argument("--ps_transport", choices=["auto", "native", "pg"], default="auto",
                    help="--mode=ps data plane: native = hipIpc mailboxes + C++ service thread (one node, GPUs; "
                         "parallel/ps_native.py), pg = torch.distributed send/recv; auto = native when eligible")
    ap.add_argument("--ps_partition_mb", type=float, default=0.0,
                    help="--mode=ps: split every variable larger than this many MB (fp32) into partitions "
                         "'<var>/part_<i>' dealt round-robin over the ps tasks (tf.variable_axis_size_partitioner "
                         "semantics; checkpoints keep the TF slice layout).  0: whole variables, as the reference")
    ap.add_argument("--clip_norm", type=float, default=0.0,
                    help="clip each optimizer's gradients by their global norm (tf.clip_by_global_norm over the "
                         "minimize call's var list, after the 1/world averaging) on the device, inside the "
                         "captured step; 0 (default): off, the reference's behaviour.  ps mode: the worker clips "
                         "before it pushes.  The MNIST CNN's own schedule cannot clip: add --bucket_mb")
    ap.add_argument("--augment", choices=["none", "cifar"], default="none",
                    help="input transforms on the training batches: cifar = per-channel standardisation with the "
                         "training set's statistics, 4-pixel zero pad + random 32x32 crop, random horizontal flip, "
                         "in the batch-gather launch on GPUs (resnet20 only; its evaluation standardises too); "
                         "none (default): pixels / 255 as they are.  The crop / flip draws are a counter-based "
                         "stream seeded with the worker's data seed; a restart begins its counter at 0 again (with "
                         "--shuffle device: at the restored global step)")
    ap.add_argument("--mix", choices=["none", "mixup", "cutmix"], default="none",
                    help="blend every training image with a partner of its batch inside the --augment cifar launch "
                         "(needs it): mixup = lam * image + (1 - lam) * partner, cutmix = a random box of the partner "
                         "pasted in, the label rows mixed by lam resp. the kept area; lam ~ Uniform[0, 1) = Beta(1, 1). "
                         "The partner is the batch rotated by a per-step shift, the draws continue the crop / flip "
                         "stream's counter.  The logged loss is the soft-target cross-entropy; none (default): off")
    ap.add_argument("--label_smoothing", type=float, default=0.0,
                    help="E in [0, 1): the training label rows hold 1 - E + E / classes for the label and E / classes "
                         "elsewhere, written by the --augment cifar launch (needs it); evaluation keeps hard labels.  "
                         "0 (default): off")
    ap.add_argument("--shuffle", choices=["host", "device"], default="host",
                    help="where a batch's rows are chosen (local / all-reduce modes): host = the host EpochBatcher's "
                         "indices, copied to the device per step (the default); device = a per-epoch permutation of "
                         "the training set evaluated inside the batch-gather launch from a device counter, so the "
                         "batch draw is captured with the step.  Both visit every image once per epoch (in different "
                         "orders); device mode continues the epoch order and the crop / flip stream after a restart, and "
                         "its log steps report 'epoch' (host mode's metrics lines stay as they were)")
    ap.add_argument("--steps_per_graph", type=int, default=1,
                    help="training steps per hipGraph replay (needs --shuffle device: host indices cannot enter a "
                         "replay).  The loop's unit becomes a replay: stop checks, the metrics line and the step line "
                         "come once per replay; --num_steps is never overshot (the remainder runs one step per replay); "
                         "the graphs are captured by the run's first replays, whose ms include the capture")
    ap.add_argument("--lr_boundaries", type=_int_list, default=(),
                    help="learning-rate schedule, evaluated from global_step inside the fused apply (local / "
                         "all-reduce modes; the MNIST CNN's own schedule needs --bucket_mb): the steps of "
                         "tf.train.piecewise_constant, e.g. 32000,48000 (at most 8), with --lr_values")
    ap.add_argument("--lr_values", type=_float_list, default=(),
                    help="the rates of --lr_boundaries, one more than boundaries, e.g. 0.1,0.01,0.001: the first "
                         "while step <= the first boundary, the last beyond the last boundary")
    ap.add_argument("--lr_decay_steps", type=int, default=0,
                    help="linear decay (tf.train.polynomial_decay, power 1, no cycling) from --learning_rate to "
                         "--lr_end over this many steps, constant after; not together with --lr_boundaries")
    ap.add_argument("--lr_end", type=float, default=0.0, help="the rate --lr_decay_steps ends at")
    ap.add_argument("--lr_warmup_steps", type=int, default=0,
                    help="linear warm-up: the rate times (step + 1) / W during the first W steps")
    ap.add_argument("--weight_decay", type=float, default=0.0,
                    help="coupled L2 weight decay: D * w is added to the gradient of every variable the model "
                         "declares as decaying (resnet20: the conv and dense kernels; not batch-norm scales, "
                         "offsets or biases), after --clip_norm's scale, inside the fused apply.  The logged loss "
                         "stays the cross-entropy alone, without the L2 term.  0 (default): off")
    add_bool(ap, "nesterov", False, "Nesterov momentum (TF1 MomentumOptimizer use_nesterov) for models that declare "
                                    "decaying variables (resnet20)")
    ap.add_argument("--ema_decay", type=float, default=0.0,
                    help="keep an exponential moving average of every trained variable "
                         "(tf.train.ExponentialMovingAverage: shadow -= (1 - D) * (shadow - variable) after each "
                         "update, started at the initial values), updated inside the fused apply (local / "
                         "all-reduce modes; the MNIST CNN's own schedule needs --bucket_mb).  With it --eval_every "
                         "and the lstm / cnn end-of-run accuracy evaluate the averaged weights, checkpoints gain "
                         "<var>/ExponentialMovingAverage, log steps report ema_decay.  In [0, 1); 0 (default): off")
    add_bool(ap, "ema_num_updates", False, "with --ema_decay: the decay is min(D, (1 + step) / (10 + step)) "
                                           "(ExponentialMovingAverage's num_updates=global_step)")
    ap.add_argument("--lars_eeta", type=float, default=0.0,
                    help="layer-wise adaptive rate scaling (tf.contrib.opt.LARSOptimizer) for momentum models that "
                         "declare decaying variables (resnet20): each of those variables (conv and dense kernels) "
                         "takes the rate times E * |w| / (|g| + D * |w| + --lars_epsilon), D being --weight_decay "
                         "and |g| the norm after --clip_norm's scale; batch-norm scales, offsets and biases keep "
                         "the rate.  The ratios come from one extra launch before the fused apply (local / "
                         "all-reduce modes; the MNIST CNN's own schedule needs --bucket_mb); log steps report "
                         "trust_min and trust_max.  0 (default): off")
    ap.add_argument("--lars_epsilon", type=float, default=0.0,
                    help="with --lars_eeta: the epsilon added to the trust ratio's denominator (default 0)")
    ap.add_argument("--eval_every", type=int, default=0,
                    help="evaluate on the test split whenever a multiple of N lies among the model steps an "
                         "iteration ran, and once at the end of training (local / all-reduce modes; models whose "
                         "program has an inference forward to logits: resnet20, resnet50).  The test set stays on "
                         "the device, the chunks replay as one captured graph and the host reads once per "
                         "evaluation; every rank evaluates the whole set.  The step's ms excludes the evaluation; "
                         "its metrics line gains test_accuracy, test_top<K>, test_loss, test_examples, eval_ms.  "
                         "0 (default): off")
    ap.add_argument("--eval_examples", type=int, default=0,
                    help="with --eval_every: evaluate the first M test examples only; 0 (default): the whole split")
    ap.add_argument("--eval_topk", type=int, default=5,
                    help="with --eval_every: K of the top-K accuracy reported next to top-1 (1 <= K <= classes)")
    ap.add_argument("--metrics_jsonl", default="", help="append {step, gs, ms, images/sec, loss} lines here")
    ap.add_argument("--heartbeat_secs", type=float, default=None,
                    help="publish a TCPStore heartbeat every N s; 0: off.  Default: %s s in --mode=allreduce "
                         "(failure detection on: a dead peer ends every rank), 0 in --mode=ps / local (the "
                         "reference has no heartbeat)" % AR_HEARTBEAT_SECS)
    ap.add_argument("--heartbeat_timeout", type=float, default=30.0,
                    help="ps: count a worker silent for this long as lost; all-reduce: a rank whose peer "
                         "is silent this long aborts the collectives and exits non-zero (with --heartbeat_secs)")
    add_bool(ap, "phase_timers", False, "time fwd+bwd / comm / apply per step with hipEvents (no hipGraph)")
    add_bool(ap, "check_pull", False, "debug: checksum (and L2 norm of) the pulled parameters every step (ps mode) / the "
                                      "replicas' parameters at the end (all-reduce mode)")
    ap.add_argument("--trace_json", default="", help="write the per-step phase timings as a Chrome trace "
                                                     "(chrome://tracing / Perfetto); implies --phase_timers")
    return ap


def parse(argv=None, model_defaults=None, prog=None):
    ap = build_parser(model_defaults, prog)
    args, unknown = ap.parse_known_args(argv)
    if unknown:
        ap.error("unknown flags: %s" % " ".join(unknown))
    if not args.clip_norm >= 0:
        ap.error("--clip_norm must be >= 0 (0 = off), got %r" % args.clip_norm)
    if not args.weight_decay >= 0:
        ap.error("--weight_decay must be >= 0 (0 = off), got %r" % args.weight_decay)
    if not args.steps_per_graph >= 1:
        ap.error("--steps_per_graph must be >= 1, got %r" % args.steps_per_graph)
    if not args.eval_every >= 0:
        ap.error("--eval_every must be >= 0 (0 = off), got %r" % args.eval_every)
    if not args.eval_examples >= 0:
        ap.error("--eval_examples must be >= 0 (0 = the whole test split), got %r" % args.eval_examples)
    if not args.eval_topk >= 1:
        ap.error("--eval_topk must be >= 1, got %r" % args.eval_topk)
    if not 0 <= args.ema_decay < 1:
        ap.error("--ema_decay must lie in [0, 1) (0 = off), got %r" % args.ema_decay)
    if args.ema_num_updates and not args.ema_decay > 0:
        ap.error("--ema_num_updates shapes the decay of a moving average: it needs --ema_decay")
    if not (args.lars_eeta >= 0 and args.lars_eeta < float("inf")):
        ap.error("--lars_eeta must be >= 0 (0 = off), got %r" % args.lars_eeta)
    if not (args.lars_epsilon >= 0 and args.lars_epsilon < float("inf")):
        ap.error("--lars_epsilon must be >= 0, got %r" % args.lars_epsilon)
    if args.lars_epsilon and not args.lars_eeta > 0:
        ap.error("--lars_epsilon belongs to the trust ratio: it needs --lars_eeta")
    if args.lr_end and not args.lr_decay_steps:
        ap.error("--lr_end is the end of a linear decay: it needs --lr_decay_steps")
    return args
