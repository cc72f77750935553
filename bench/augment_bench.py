"""gather_rows against augment_rows (pad 4, flip, channel statistics) on the same tensors: a 4096-row
pool of 32x32x3 uint8 images -> a bf16 batch, rows sampled on the device, B = 128 and 256.  Both
kernels read B * 3072 bytes and write B * 6144, so the target is parity: the augment_rows median at
most 25 % above the gather_rows median of the same run (the margin pays the LDS round trip).

The two launches alternate in rounds (neighbours on the machine move both alike); a round replays a
hipGraph of ``--reps`` back-to-back launches between two device events and reports microseconds per
launch (kernel + launch gap, as in a captured step); the figures are the median, minimum and maximum
over ``--rounds`` rounds after a warm-up round of each.

    python bench/augment_bench.py [--rounds 200] [--reps 50] [--out profiles/augment.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtfe  # noqa: E402,F401
from dtfe import ops  # noqa: E402

N_ROWS, H, W, C = 4096, 32, 32, 3
TARGET = 1.25


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
        raise SystemExit("augment_bench: needs a GPU (a CPU timing says nothing about these kernels)")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (N_ROWS, H * W * C), generator=g, dtype=torch.uint8).to(dev)
    lab = torch.randint(0, 10, (N_ROWS,), generator=g, dtype=torch.int32).to(dev)
    mean = torch.tensor([0.49, 0.48, 0.45], device=dev)
    inv_std = torch.tensor([4.0, 4.1, 3.8], device=dev)
    lines = ["gather_rows vs augment_rows (pad 4, flip, statistics): %d x %dx%dx%d uint8 -> bf16, sampled rows, "
             "labels + one-hot rows + counter ticket in the launch" % (N_ROWS, H, W, C),
             "us per launch over %d rounds of %d launches, the two alternating: median [min, max]" % (args.rounds, args.reps)]
    for B in (128, 256):
        dst = torch.empty(B, H, W, C, device=dev, dtype=torch.bfloat16)
        ld = torch.empty(B, dtype=torch.int32, device=dev)
        oh = torch.empty(B, 10, device=dev)
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        done = torch.zeros(1, dtype=torch.int32, device=dev)
        flat = dst.view(B, -1)

        def gather():
            ops.gather_rows(src, flat, None, lab, ld, seed=1, counter=ctr, done=done, onehot=oh)

        def augment():
            ops.augment_rows(src, dst, H, W, C, pad=4, flip=True, mean=mean, inv_std=inv_std, labels_src=lab,
                             labels_dst=ld, seed=1, counter=ctr, done=done, onehot=oh)

        t = {"gather_rows": [], "augment_rows": []}
        gg, ga = chain(gather, args.reps), chain(augment, args.reps)
        timeit(gg, args.reps)
        timeit(ga, args.reps)
        for _ in range(args.rounds):
            t["gather_rows"].append(timeit(gg, args.reps))
            t["augment_rows"].append(timeit(ga, args.reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        nbytes = B * H * W * C * 3
        for k, v in t.items():
            lines.append("B=%-4d %-13s %6.2f [%6.2f, %6.2f] us   %5.1f GB/s" % (B, k, med[k], min(v), max(v),
                                                                             nbytes / med[k] / 1e3))
        ratio = med["augment_rows"] / med["gather_rows"]
        lines.append("B=%-4d augment / gather = %.3f  (target <= %.2f: %s)" % (B, ratio, TARGET,
                                                                           "met" if ratio <= TARGET else "NOT met"))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
