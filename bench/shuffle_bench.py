"""The batch-gather launch with rows sampled with replacement (hash % n) against the same launch with rows
from the per-epoch permutation (shuffle=True), gather_rows and augment_rows, at the shapes the examples
train with: CIFAR-10 (n = 50000, 32x32x3 uint8 -> bf16) at B = 128 and 256, MNIST (n = 55000, 28x28x1
uint8 -> f32) at B = 100.  The permutation costs 4 hashes per walk and a 64-bit divide per row where the
other mode costs one hash; the target is the shuffled median at most 25 % above the with-replacement
median of the same run.

The launches alternate in rounds (neighbours on the machine move all alike); a round replays a hipGraph
of ``--reps`` back-to-back launches between two device events and reports microseconds per launch; the
figures are the median, minimum and maximum over ``--rounds`` rounds after a warm-up round of each.

    python bench/shuffle_bench.py [--rounds 200] [--reps 50] [--out profiles/device_shuffle.txt]
    python bench/shuffle_bench.py --replace_only            # (a build without the mode: DTFE_KERNEL_LIB=...)

``--cli MODEL``: the training CLI's milliseconds per step instead - the median ``ms`` of the metrics lines
after the first ``--skip`` steps of a ``--steps``-step run, for the flags after ``--``:

    python bench/shuffle_bench.py --cli resnet20 --steps 400 -- --batch_size 128 --augment cifar \\
        --shuffle device --steps_per_graph 4

``--tree DIR`` imports the package from another checkout (a build of the parent commit, for the baseline).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

TARGET = 1.25
# (name, n_rows, (H, W, C), pad, flip, destination, batch sizes)
SHAPES = [("cifar", 50000, (32, 32, 3), 4, True, "bf16", (128, 256)),
          ("mnist", 55000, (28, 28, 1), 2, False, "f32", (100,))]


def chain(torch, fn, reps):
    """``reps`` launches of fn captured back to back into one hipGraph (a linear chain): a replay costs
    the device the kernels and the gaps between them, not the Python wrapper's microseconds per call."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g


def timeit(torch, g, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / reps


def launches(args, torch, ops):
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lines = ["batch gather, rows with replacement vs rows from the epoch permutation (shuffle): uint8 sources, labels + "
             "one-hot rows + counter ticket in the launch",
             "us per launch over %d rounds of %d launches, all alternating: median [min, max]" % (args.rounds, args.reps)]
    for name, n, (H, W, C), pad, flip, dd, batches in SHAPES:
        D = H * W * C
        src = torch.randint(0, 256, (n, D), generator=g, dtype=torch.uint8).to(dev)
        lab = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).to(dev)
        mean = torch.full((C,), 0.47, device=dev)
        inv_std = torch.full((C,), 4.0, device=dev)
        for B in batches:
            dst = torch.empty(B, H, W, C, device=dev, dtype=torch.bfloat16 if dd == "bf16" else torch.float32)
            flat = dst.view(B, -1)
            ld = torch.empty(B, dtype=torch.int32, device=dev)
            oh = torch.empty(B, 10, device=dev)
            ctr = torch.zeros(1, dtype=torch.int64, device=dev)
            done = torch.zeros(1, dtype=torch.int32, device=dev)

            def gather(**kw):
                ops.gather_rows(src, flat, None, lab, ld, seed=1, counter=ctr, done=done, onehot=oh, **kw)

            def augment(**kw):
                ops.augment_rows(src, dst, H, W, C, pad=pad, flip=flip, mean=mean, inv_std=inv_std, labels_src=lab,
                                 labels_dst=ld, seed=1, counter=ctr, done=done, onehot=oh, **kw)

            fns = {"gather_rows": gather, "augment_rows": augment}
            if not args.replace_only:
                fns["gather_rows shuffle"] = lambda: gather(shuffle=True)
                fns["augment_rows shuffle"] = lambda: augment(shuffle=True)
            graphs = {k: chain(torch, f, args.reps) for k, f in fns.items()}
            t = {k: [] for k in fns}
            for k in fns:
                timeit(torch, graphs[k], args.reps)
            for _ in range(args.rounds):
                for k in fns:
                    t[k].append(timeit(torch, graphs[k], args.reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            for k, v in t.items():
                lines.append("%-5s n=%-5d D=%-4d B=%-3d %-20s %6.2f [%6.2f, %6.2f] us" % (name, n, D, B, k, med[k],
                                                                                       min(v), max(v)))
            for k in ("gather_rows", "augment_rows"):
                if k + " shuffle" in med:
                    ratio = med[k + " shuffle"] / med[k]
                    lines.append("%-5s B=%-3d %s shuffle / with replacement = %.3f  (target <= %.2f: %s)"
                                 % (name, B, k, ratio, TARGET, "met" if ratio <= TARGET else "NOT met"))
    return lines


def cli(args, torch, train):
    with tempfile.TemporaryDirectory() as d:
        mj = os.path.join(d, "m.jsonl")
        argv = ["--mode=local", "--device=cuda", "--synthetic", "--save_model_secs=0", "--log_every=1000000",
                "--num_steps=%d" % args.steps, "--metrics_jsonl=" + mj, "--model_dir=" + os.path.join(d, "ck")] + args.rest
        train.run(args.cli, argv, log=lambda *_: None)
        torch.cuda.synchronize()
        rows = [json.loads(line) for line in open(mj)]
    ms = [r["ms"] for r in rows if r["gs"] > args.skip]
    q = statistics.quantiles(ms, n=10)
    return ["cli %-8s %-60s ms/step median %.4f  [p10 %.4f, p90 %.4f]  (%d lines after step %d)"
            % (args.cli, " ".join(args.rest), statistics.median(ms), q[0], q[-1], len(ms), args.skip)]


def main():
    argv = sys.argv[1:]
    rest = []
    if "--" in argv:
        rest = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--replace_only", action="store_true", help="time the with-replacement launches only")
    ap.add_argument("--cli", default="", help="model name: time the training CLI with the flags after --")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--skip", type=int, default=100)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default="", help="append the lines to this file")
    args = ap.parse_args(argv)
    args.rest = rest
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch

    import dtfe  # noqa: F401
    from dtfe import ops, train

    if not torch.cuda.is_available():
        raise SystemExit("shuffle_bench: needs a GPU (a CPU timing says nothing about these kernels)")
    lines = cli(args, torch, train) if args.cli else launches(args, torch, ops)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
