"""On-device evaluation, measured: writes profiles/device_eval.txt (run on the MI355X).

  (a) ResNet-20, B = 128, the 10 k synthetic CIFAR test rows: DeviceEvaluator.run() against
      ResNetProgram.evaluate() over the same rows
  (b) the eval_metrics kernel alone at (B, NC) = (128, 10) and (256, 1000), beside softmax_xent
  (c) the ResNet-20 CLI's ms / step with --eval_every 0 against another checkout (--parent_dir: the
      parent commit, built), each run a fresh process

Every comparison alternates its variants inside one command, 5 runs each, and reports the median and the
min - max.  Times are host clocks around work that ends in a device synchronise ((a), (c)) or device events
around a block of launches ((b)).

    python bench/eval_bench.py [--parent_dir DIR] [--out profiles/device_eval.txt] [--runs 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtfe  # noqa: E402,F401
from dtfe import ops  # noqa: E402
from dtfe.data import cifar  # noqa: E402
from dtfe.models.resnet import ResNetModel  # noqa: E402
from dtfe.utils.device_eval import DeviceEvaluator  # noqa: E402

DEV = "cuda:0"


def fmt(xs, unit):
    return "median %.3f %s (min %.3f - max %.3f, %d runs)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def part_a(runs, out):
    (_, _), (te_x, te_y) = cifar.synthetic_arrays(n_train=128, n_test=10000)
    prog = ResNetModel(0.1, "resnet20").program(torch.device(DEV), 128, seed=0)
    n = te_x.shape[0]
    ev = DeviceEvaluator(prog, te_x, te_y, topk=5)
    images = torch.from_numpy(te_x.astype(np.float32) / 255.0).to(DEV)
    labels = torch.from_numpy(te_y).view(-1, 1).to(DEV)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000, r

    for _ in range(2):  # warm both (the evaluator's first pass captures its graph)
        res = ev.run()
        acc = prog.evaluate(images, labels)
    assert ev.capture_error is None and ev.graph is not None, ev.capture_error
    assert res["accuracy"] * n == round(acc * n), (res, acc)
    t_ev, t_old = [], []
    for _ in range(runs):
        t_ev.append(timed(ev.run)[0])
        t_old.append(timed(lambda: prog.evaluate(images, labels))[0])
        print("(a) run: evaluator %.2f ms, evaluate %.2f ms" % (t_ev[-1], t_old[-1]), flush=True)
    out.append("(a) ResNet-20, B = 128, %d synthetic CIFAR test rows (%d chunks), accuracy %.4f both ways"
               % (n, ev.chunks, acc))
    out.append("    DeviceEvaluator.run()   " + fmt(t_ev, "ms"))
    out.append("    prog.evaluate()         " + fmt(t_old, "ms"))
    out.append("    ratio of medians (evaluator / evaluate): %.3f" % (statistics.median(t_ev) / statistics.median(t_old)))


def part_b(runs, out, launches=200):
    out.append("(b) one launch, us (device events around %d back-to-back eager launches)" % launches)
    for B, NC in ((128, 10), (256, 1000)):
        g = torch.Generator().manual_seed(B + NC)
        z = torch.randn(B, NC, generator=g).to(DEV)
        t = torch.randint(0, NC, (B,), generator=g, dtype=torch.int32).to(DEV)
        state = ops.eval_state(DEV, B)
        idx = torch.zeros(B, dtype=torch.int32, device=DEV)
        ws = torch.zeros(2 * B, dtype=torch.int32, device=DEV)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        loss = torch.zeros(1, device=DEV)
        correct = torch.zeros(1, dtype=torch.int32, device=DEV)

        def ev_launch():
            # (reset_eval sets n = B * launches before a block: every launch of the block scores B rows)
            ops.eval_metrics(z, t, 5, state, idx=idx, ws=ws, ticket=ticket)

        def xent_launch():
            ops.softmax_xent(z, labels_i=t, loss_sum=loss, correct=correct)

        def block(fn, reset):
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1000 / launches

        def reset_eval():
            state.zero_()
            state[ops.EVAL_N:ops.EVAL_N + 1].fill_(B * launches)  # never past the end inside a block

        for _ in range(2):
            block(ev_launch, reset_eval)
            block(xent_launch, loss.zero_)
        t_ev, t_x = [], []
        for _ in range(runs):
            t_ev.append(block(ev_launch, reset_eval))
            t_x.append(block(xent_launch, loss.zero_))
        out.append("    (B, NC) = (%d, %d)  eval_metrics  %s" % (B, NC, fmt(t_ev, "us")))
        out.append("    (B, NC) = (%d, %d)  softmax_xent  %s" % (B, NC, fmt(t_x, "us")))


def cli_ms(tree, steps, extra=()):
    """Median ms / step of the ResNet-20 CLI in checkout ``tree`` (a fresh process), after its first 50 steps."""
    with tempfile.TemporaryDirectory() as td:
        mj = os.path.join(td, "m.jsonl")
        cmd = [sys.executable, os.path.join(tree, "examples", "resnet", "distributed_resnet20.py"), "--device=cuda",
               "--synthetic", "--num_steps", str(steps), "--log_every", "1000000", "--save_model_secs=0",
               "--model_dir", os.path.join(td, "ck"), "--metrics_jsonl", mj] + list(extra)
        p = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError("CLI failed in %s:\n%s" % (tree, p.stdout[-2000:]))
        rows = [json.loads(line) for line in open(mj)]
    return statistics.median(r["ms"] for r in rows[50:])


def part_c(runs, out, parent_dir, steps=400):
    out.append("(c) ResNet-20 CLI (B = 128, synthetic CIFAR, --eval_every 0), median ms / step of steps 50..%d of a "
               "fresh process" % steps)
    if not parent_dir:
        out.append("    not measured: no --parent_dir given")
        return
    parent_dir = os.path.abspath(parent_dir)
    t_new, t_old = [], []
    for _ in range(runs):
        t_new.append(cli_ms(ROOT, steps))
        t_old.append(cli_ms(parent_dir, steps))
        print("(c) run: this tree %.3f ms, parent %.3f ms" % (t_new[-1], t_old[-1]), flush=True)
    out.append("    this tree     " + fmt(t_new, "ms"))
    out.append("    parent commit " + fmt(t_old, "ms"))
    inside = min(t_old) <= statistics.median(t_new) <= max(t_old)
    out.append("    this tree's median lies %s the parent's min - max" % ("inside" if inside else "OUTSIDE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_dir", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_eval.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs the GPU (a CPU timing says nothing about it)")
    out = ["On-device evaluation (bench/eval_bench.py) on %s" % torch.cuda.get_device_name(0), ""]
    if "a" in a.parts:
        part_a(a.runs, out)
        out.append("")
    if "b" in a.parts:
        part_b(a.runs, out)
        out.append("")
    if "c" in a.parts:
        part_c(a.runs, out, a.parent_dir)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
