"""augment_rows with mixing and label smoothing against the plain launch on the same tensors: a 4096-row
pool of 32x32x3 uint8 images -> a bf16 batch of B = 128, pad 4, flip, channel statistics, rows drawn by the
device shuffle, labels + label rows + counter ticket in the launch.

Variants: ``plain`` (a call without the new arguments: the yardstick), ``none`` (mix="none", E = 0 through
them: the same kernel instantiation, so it must equal ``plain`` within the spread of the rounds),
``none+smooth`` (E = 0.1), ``mixup`` and ``cutmix`` (E = 0.1): the last two stage two images per workgroup.

The launches alternate in rounds (neighbours on the machine move all alike); a round replays a hipGraph of
``--reps`` back-to-back launches between two device events and reports microseconds per launch (kernel +
launch gap, as in a captured step); the figures are the median, minimum and maximum over ``--rounds`` rounds
after a warm-up round of each, and the ratio of the medians to ``plain``.

    python bench/mix_bench.py [--rounds 200] [--reps 50] [--out profiles/mix_augment.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtfe  # noqa: E402,F401
from dtfe import ops  # noqa: E402

N_ROWS, H, W, C, B = 4096, 32, 32, 3, 128
VARIANTS = [("plain", None), ("none", dict(mix="none", label_smoothing=0.0)),
            ("none+smooth", dict(mix="none", label_smoothing=0.1)), ("mixup", dict(mix="mixup", label_smoothing=0.1)),
            ("cutmix", dict(mix="cutmix", label_smoothing=0.1))]


def chain(fn, reps):
    """``reps`` launches of fn captured back to back into one hipGraph (a linear chain): a replay costs
    the device the kernels and the gaps between them, not the Python wrapper's microseconds per call."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    return g


def timeit(g, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: needs a GPU (a CPU timing says nothing about these kernels)")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (N_ROWS, H * W * C), generator=g, dtype=torch.uint8).to(dev)
    lab = torch.randint(0, 10, (N_ROWS,), generator=g, dtype=torch.int32).to(dev)
    mean = torch.tensor([0.49, 0.48, 0.45], device=dev)
    inv_std = torch.tensor([4.0, 4.1, 3.8], device=dev)
    dst = torch.empty(B, H, W, C, device=dev, dtype=torch.bfloat16)
    ld = torch.empty(B, dtype=torch.int32, device=dev)
    oh = torch.empty(B, 10, device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(kw):
        def fn():
            ops.augment_rows(src, dst, H, W, C, pad=4, flip=True, mean=mean, inv_std=inv_std, labels_src=lab,
                             labels_dst=ld, seed=1, counter=ctr, done=done, onehot=oh, shuffle=True, **(kw or {}))
        return fn

    graphs = [(name, chain(launch(kw), args.reps)) for name, kw in VARIANTS]
    t = {name: [] for name, _ in graphs}
    for name, gr in graphs:
        timeit(gr, args.reps)
    for _ in range(args.rounds):
        for name, gr in graphs:
            t[name].append(timeit(gr, args.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = ["augment_rows, mixing and label smoothing (pad 4, flip, statistics, device shuffle): %d x %dx%dx%d uint8 -> "
             "bf16, B = %d, labels + label rows + counter ticket in the launch" % (N_ROWS, H, W, C, B),
             "us per launch over %d rounds of %d launches, the variants alternating: median [min, max], median / plain"
             % (args.rounds, args.reps)]
    for name, v in t.items():
        lines.append("%-12s %6.2f [%6.2f, %6.2f] us   %.3f" % (name, med[name], min(v), max(v), med[name] / med["plain"]))
    lo, hi = min(t["plain"]), max(t["plain"])
    lines.append("none vs plain (one instantiation): median %.2f %s plain's [%.2f, %.2f]"
                 % (med["none"], "inside" if lo <= med["none"] <= hi else "OUTSIDE", lo, hi))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
