"""The fused apply of ResNet-20's var list (momentum, 0.27 M parameters, the conv kernels on the
transposed-tile path), alone: plain, as the model ran it before there was a recipe, against the full
CIFAR-10 recipe inside the same launch - piecewise-constant schedule with warm-up read from global_step on
the device, L2 weight decay on the kernels, Nesterov momentum, the rate written to lr_out.

The recipe adds no memory stream (the parameters it decays are loaded anyway), so the expectation is
parity.  A run replays a hipGraph of ``--reps`` back-to-back launches between two device events and
reports microseconds per launch (kernel + launch gap, as in a captured step): median, minimum and maximum
over ``--rounds`` replays after a warm-up replay.  ``--plain`` uses only the optimizer API that existed
before the recipe, so the same file times the commit before it.

    python bench/apply_recipe_bench.py [--plain] [--rounds 200] [--reps 50]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtfe  # noqa: E402,F401
from dtfe.models.resnet import ResNetModel  # noqa: E402
from dtfe.optim import FlatParams, Optimizer, OptimizerConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", action="store_true", help="constant rate, no decay, no Nesterov: today's API only")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("apply_recipe_bench: needs a GPU (a CPU timing says nothing about this kernel)")
    dev = "cuda"
    model = ResNetModel()
    names = model.opt_groups[0][1]
    P = FlatParams(model.specs, dev, seed=0)
    P.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    P.grad.mul_(1e-3)
    gs = torch.zeros(1, dtype=torch.int32, device=dev)
    cfg = OptimizerConfig(kind="momentum", lr=0.1, momentum=0.9)
    if not args.plain:
        # boundaries the launches of a run cross: the schedule's branches are all taken
        cfg = OptimizerConfig(kind="momentum", lr=0.1, momentum=0.9, lr_boundaries=(2000, 6000),
                              lr_values=(0.1, 0.01, 0.001), lr_warmup_steps=500, weight_decay=1e-4,
                              decay_vars=tuple(model.decay_vars), nesterov=True)
    opt = Optimizer(cfg, P, var_list=names, global_step=gs)
    opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.reps):
            opt.step()

    def timeit():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1000 / args.reps

    timeit()
    t = [timeit() for _ in range(args.rounds)]
    n = sum(P.spec(v).numel for v in names)
    print(json.dumps({"bench": "apply_recipe", "variant": "plain" if args.plain else "recipe", "elements": n,
                      "work_items": opt.nwork, "us_per_launch_median": round(statistics.median(t), 3),
                      "min": round(min(t), 3), "max": round(max(t), 3), "rounds": args.rounds, "reps": args.reps,
                      "global_step": int(gs.item()), "finite": bool(torch.isfinite(P.master).all())}), flush=True)


if __name__ == "__main__":
    main()
