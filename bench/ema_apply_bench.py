"""The fused apply with and without the exponential moving average of the weights, alone, at two var lists:
the MNIST CNN's (Adam, 3.27 M parameters) and ResNet-50's (momentum, bf16 copies with transposes).

For each it times, per launch:
  (a) the apply without EMA
  (b) the apply with EMA (one more read stream and one more write stream inside the same launch)
  (c) (a) followed by the stock alternative, ``ema.add_(p - ema, alpha=1 - d)`` over the flat buffer
  (c') (a) followed by ``ema.lerp_(p, 1 - d)`` - the same update as one stock kernel, the fairer rival
  (d) ema_swap alone
Every variant is a hipGraph of ``--reps`` back-to-back launches (kernel + launch gap, as in a captured step),
timed between two device events.  The variants alternate inside every round, after a warm-up round, so drift
of the machine hits them alike; the table reports the median, minimum and maximum over ``--rounds`` rounds
and (b)/(a) next to the ratio of the bytes the two launches move, computed here from the var list.
The claim to check is (b) < (c).

    python bench/ema_apply_bench.py [--rounds 100] [--reps 20] [--out profiles/ema_apply.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtfe  # noqa: E402,F401
from dtfe.models.mnist_cnn import MnistCnnModel  # noqa: E402
from dtfe.models.resnet import ResNetModel  # noqa: E402
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig  # noqa: E402

D = 0.999
STREAMS = {"sgd": 3, "momentum": 5, "adam": 7, "rmsprop": 7}  # fp32 streams of an apply: p, g, slots in; p, slots out


def apply_bytes(P, names, kind, ema):
    n = sum(P.spec(v).numel for v in names)
    b16 = sum(P.spec(v).numel * ((v in P.w16) + (v in P.wt16)) for v in names)
    return 4 * n * (STREAMS[kind] + (2 if ema else 0)) + 2 * b16


def captured(fn, reps):
    fn()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g


def timed(graph, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    graph.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / reps


def workload(title, model, kind, rounds, reps, dev="cuda"):
    names = model.opt_groups[0][1]
    P = FlatParams(model.specs, dev, seed=0)
    P.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    P.grad.mul_(1e-3)
    kw = dict(kind=kind, lr=1e-4, momentum=0.9 if kind == "momentum" else 0.0)
    gs = torch.zeros(1, dtype=torch.int32, device=dev)
    plain = Optimizer(OptimizerConfig(**kw), P, var_list=names, global_step=gs)
    fused = Optimizer(OptimizerConfig(ema_decay=D, **kw), P, var_list=names, global_step=gs)
    stock = P.master.clone()

    def add_():
        plain.step()
        stock.add_(P.master - stock, alpha=1 - D)

    def lerp_():
        plain.step()
        stock.lerp_(P.master, 1 - D)

    variants = [("(a) apply", plain.step), ("(b) apply + EMA, fused", fused.step),
                ("(c) apply, then ema.add_(p - ema, alpha=1 - d)", add_),
                ("(c') apply, then ema.lerp_(p, 1 - d)", lerp_), ("(d) ema_swap", fused.swap_ema)]
    graphs = [(n, captured(f, reps)) for n, f in variants]
    for _n, g in graphs:
        timed(g, reps)
    t = {n: [] for n, _ in graphs}
    for _ in range(rounds):
        for n, g in graphs:
            t[n].append(timed(g, reps))
    n_el = sum(P.spec(v).numel for v in names)
    ba, bb = apply_bytes(P, names, kind, False), apply_bytes(P, names, kind, True)
    med = {n: statistics.median(v) for n, v in t.items()}
    a, b, c, c2 = (med[graphs[i][0]] for i in range(4))
    lines = ["%s: %s, %d parameters in %d variables, %d work items, flat buffer %d floats"
             % (title, kind, n_el, len(names), plain.nwork, P.total),
             "  us per launch over %d rounds of %d captured launches: median (min .. max)" % (rounds, reps)]
    for n, _ in graphs:
        lines.append("  %-48s %9.2f  (%.2f .. %.2f)" % (n, med[n], min(t[n]), max(t[n])))
    lines += ["  (b)/(a) time %.3f, bytes moved %.3f (%.1f MB against %.1f MB: %d against %d fp32 streams plus the "
              "bf16 stores)" % (b / a, bb / ba, bb / 1e6, ba / 1e6, STREAMS[kind] + 2, STREAMS[kind]),
              "  (b) effective bandwidth %.0f GB/s, (a) %.0f GB/s" % (bb / b / 1e3, ba / a / 1e3),
              "  (b) < (c): %s (%.2f against %.2f us); (b) < (c'): %s (%.2f us)"
              % ("yes" if b < c else "NO", b, c, "yes" if b < c2 else "NO", c2),
              "  finite: %s" % bool(torch.isfinite(P.master).all() and torch.isfinite(fused.ema).all())]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_apply_bench: needs a GPU (a CPU timing says nothing about this kernel)")
    lines = ["The fused apply with the EMA of the weights (bench/ema_apply_bench.py) on %s"
             % torch.cuda.get_device_name(0), ""]
    lines += workload("MNIST CNN", MnistCnnModel(), "adam", args.rounds, args.reps) + [""]
    lines += workload("ResNet-50", ResNetModel(0.1, "resnet50"), "momentum", args.rounds, args.reps)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
