"""The momentum apply with layer-wise rate scaling (LARS) and with the global-norm clip, alone, at two var lists:
ResNet-20's (0.27 M parameters) and ResNet-50's (25.6 M), both with bf16 copies and transposes.

For each it times, per step:
  (a) the apply alone
  (b) the clip's norm launch + the apply
  (c) the trust launch + the apply reading a rate per variable
  (d) all three launches: norm, trust, apply
and, alone, the norm launch and the trust launch (which reads the masters as well: twice the bytes), the
latter also at the other chunk sizes of its plan.
Every variant is timed twice between two device events: as a hipGraph of ``--reps`` back-to-back steps
(kernel + launch gap, as in a captured step) and as ``--reps`` eager steps (stand-alone: the host's launch
cost shows where it exceeds the kernel).  The variants alternate inside every round, after a warm-up round,
so drift of the machine hits them alike; the table reports the median, minimum and maximum over ``--rounds``
rounds, and the bytes each launch has to move, computed here from the var list.

    python bench/lars_apply_bench.py [--rounds 50] [--reps 20] [--out profiles/lars_apply.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtfe  # noqa: E402,F401
from dtfe import ops  # noqa: E402
from dtfe.models.resnet import ResNetModel  # noqa: E402
from dtfe.optim import FlatParams, LayerTrust, Optimizer, OptimizerConfig  # noqa: E402


def captured(fn, reps):
    fn()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g.replay


def eager(fn, reps):
    def run():
        for _ in range(reps):
            fn()
    return run


def timed(run, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / reps


def workload(title, model, rounds, reps, dev="cuda"):
    names = model.opt_groups[0][1]
    adaptive = tuple(n for n in model.decay_vars if n in names)
    P = FlatParams(model.specs, dev, seed=0)
    P.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    P.grad.mul_(1e-3)
    kw = dict(kind="momentum", lr=1e-4, momentum=0.9, weight_decay=1e-4, decay_vars=adaptive)
    lars = dict(lars_eeta=0.001, lars_vars=adaptive)
    gs = torch.zeros(1, dtype=torch.int32, device=dev)
    mk = lambda **k: Optimizer(OptimizerConfig(**kw, **k), P, var_list=names, global_step=gs)
    plain, clip, trust, both = mk(), mk(clip_norm=1e9), mk(**lars), mk(clip_norm=1e9, **lars)
    n_ad = sum(P.spec(v).numel for v in adaptive)
    chunks = [1024, 2048, ops.LARS_CHUNK_MAX]
    alone = {c: LayerTrust(P, names, adaptive, trust.wd, 0.001, 0.0, chunk=c) for c in chunks}
    variants = [("(a) apply", plain.step), ("(b) norm + apply", clip.step), ("(c) trust + apply", trust.step),
                ("(d) norm + trust + apply", both.step), ("norm launch alone", clip.clip.compute)]
    variants += [("trust launch alone, chunk %d%s" % (c, " (the plan's choice)" if c == ops.LARS_CHUNK_MAX else ""),
                  alone[c].compute) for c in chunks]
    runs = [(n + " [graph]", captured(f, reps)) for n, f in variants] + [(n + " [eager]", eager(f, reps)) for n, f in variants]
    for _n, r in runs:
        timed(r, reps)
    t = {n: [] for n, _ in runs}
    for _ in range(rounds):
        for n, r in runs:
            t[n].append(timed(r, reps))
    med = {n: statistics.median(v) for n, v in t.items()}
    n_el = sum(P.spec(v).numel for v in names)
    b16 = sum(P.spec(v).numel * ((v in P.w16) + (v in P.wt16)) for v in names)
    lines = ["%s: momentum, %d parameters in %d variables (%d adaptive, %d parameters), %d apply work items, trust plan "
             "%d chunks of <= %d" % (title, n_el, len(names), len(adaptive), n_ad, plain.nwork, trust.lars.plan.shape[0],
                                     ops.LARS_CHUNK_MAX),
             "  bytes: apply %.2f MB (p, g, slot in; p, slot out; bf16 copies), norm %.2f MB (g), trust %.2f MB (p and g "
             "of the adaptive variables)" % ((4 * n_el * 5 + 2 * b16) / 1e6, 4 * n_el / 1e6, 8 * n_ad / 1e6),
             "  us per step over %d rounds of %d steps: median (min .. max)" % (rounds, reps)]
    for n, _ in runs:
        lines.append("  %-58s %9.2f  (%.2f .. %.2f)" % (n, med[n], min(t[n]), max(t[n])))
    for mode in ("graph", "eager"):
        a, b, c, d = (med["%s [%s]" % (variants[i][0], mode)] for i in range(4))
        nl, tl = med["norm launch alone [%s]" % mode], med["%s [%s]" % (variants[-1][0], mode)]
        lines.append("  %s: norm adds %.2f us to the apply, trust adds %.2f, both add %.2f; alone the trust launch is %.2f "
                     "us against the norm's %.2f (%.2fx, for %.2fx the bytes)"
                     % (mode, b - a, c - a, d - a, tl, nl, tl / nl, 2.0 * n_ad / n_el))
    lines.append("  finite: %s" % bool(torch.isfinite(P.master).all() and torch.isfinite(both.layer_trust).all()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lars_apply_bench: needs a GPU (a CPU timing says nothing about these kernels)")
    lines = ["The momentum apply with LARS and with the global-norm clip (bench/lars_apply_bench.py) on %s"
             % torch.cuda.get_device_name(0), ""]
    lines += workload("ResNet-20", ResNetModel(0.1, "resnet20"), args.rounds, args.reps) + [""]
    lines += workload("ResNet-50", ResNetModel(0.1, "resnet50"), args.rounds, args.reps)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
