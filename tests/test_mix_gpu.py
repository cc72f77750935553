"""Mixup, CutMix and label smoothing in augment_rows (csrc/kernels/augment.hip) on the GPU against the host
mirror (ops.mix_draws, ops.augment_draws) and the per-sample numpy construction of test_mix_cpu: every
comparison of a batch is torch.equal, and no expectation comes from another launch of the kernels."""
import json
import math
import os
import sys

import pytest
import torch

from dtfe import ops, train
from dtfe.data import cifar
from dtfe.data.mnist import DataSet, DeviceBatcher
from dtfe.utils.graphs import StepGraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import SENTINEL, construct, mirror_rows, source, stats  # noqa: E402
from test_mix_cpu import NCLS, STREAMS, expected, mix_covers, run_mix_case, soft_target_loss_matches  # noqa: E402
from test_rng_streams_cpu import BIG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf = torch.bfloat16
u8, f32 = torch.uint8, torch.float32

# (32,32,3): the LDS kernel at the CIFAR shape; (8,8,3) with pad 7: nearly everything is border, so zero is
# mixed with zero and with pixels; (5,5,3): D = 75, the per-element kernel; (4,4,16): channels a multiple of
# the chunk; (6,4,1): uint8 rows of 24 bytes, staged 8 bytes at a time
SHAPES = [((32, 32, 3), 4), ((8, 8, 3), 7), ((5, 5, 3), 4), ((4, 4, 16), 3), ((6, 4, 1), 3)]


@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("shape,pad", SHAPES)
def test_mixed_batches_equal_the_construction(B, shape, pad):
    """Per mix mode and smoothing value: uint8 -> bf16 with statistics and sampled rows under all six
    (seed, counter) streams, and the other 23 combinations of source / destination dtype, statistics and
    explicit / sampled / device-shuffled rows under one stream each (rotating through the six).  B = 130: the
    mirror's draws must cover lam on both sides of 0.5, boxes cut off at every edge, an inner and (small
    images) an empty box."""
    combos = [(s, d, st, r) for s in (u8, f32) for d in (bf, f32) for st in (True, False)
              for r in ("sampled", "idx", "shuffle")]
    assert combos[0] == (u8, bf, True, "sampled") and len(combos) == 24
    k = 0
    for mix in ("mixup", "cutmix"):
        for E in (0.0, 0.1):
            for i, (s, d, st, r) in enumerate(combos):
                for seed, ctr in (STREAMS if i == 0 else [STREAMS[(k + i) % 6]]):
                    draws = run_mix_case(DEV, B, shape, pad, s, d, st, r, seed, ctr, mix, E)
                    if B == 130:
                        assert mix_covers(draws, shape[0], shape[1], empty=shape[0] < 32), (shape, seed, ctr)
            k += 1


@pytest.mark.parametrize("shape", [(32, 32, 3), (5, 5, 3)])
def test_smoothing_alone_and_defaults(shape):
    """E = 0.1 without mixing: the plain batch with smoothed rows (the SMOOTH instantiations, every sampling
    mode); mix="none", E = 0 through the new arguments: a call without them, bit for bit."""
    H, W, C = shape
    for r in ("sampled", "idx", "shuffle"):
        for B in (5, 130):
            run_mix_case(DEV, B, shape, 1, u8, bf, True, r, 9, 5, "none", 0.1)
            run_mix_case(DEV, B, shape, 1, u8, bf, True, r, 9, 5, "none", 0.0)
    src, lab = source(H, W, C, u8)
    mean, inv_std = stats(C)
    B, outs = 130, []
    for kw in ({}, dict(mix="none", label_smoothing=0.0)):
        dst = torch.full((B, H, W, C), SENTINEL, device=DEV, dtype=bf)
        oh = torch.full((B, NCLS), SENTINEL, device=DEV)
        ops.augment_rows(src.to(DEV), dst, H, W, C, pad=1, flip=True, mean=mean.to(DEV), inv_std=inv_std.to(DEV),
                         labels_src=lab.to(DEV), seed=3, counter=torch.tensor([BIG], device=DEV), onehot=oh, **kw)
        outs.append((dst.cpu(), oh.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    rows = mirror_rows(3, BIG, B)
    assert torch.equal(outs[1][0], construct(src, rows, H, W, C, 1, ops.augment_draws(3, BIG, B, 1, True), mean, inv_std, bf))
    assert torch.equal(outs[1][1], torch.nn.functional.one_hot(lab[rows].long(), NCLS).float())


@pytest.mark.parametrize("shape", [(32, 32, 3), (5, 5, 3)])
@pytest.mark.parametrize("mix", ["mixup", "cutmix"])
def test_ticket_and_zero_ranges(shape, mix):
    """Two launches back to back with the ticket: the mirror's batches of counters c and c + 1, four zero
    ranges cleared (their neighbours not), the counter advanced by 1 per launch, the ticket word back at 0."""
    H, W, C = shape
    B, seed, pad, E = 130, 9, 1, 0.1
    src, lab = source(H, W, C, u8)
    mean, inv_std = stats(C)
    for c0 in (5, BIG):
        ctr = torch.tensor([c0], dtype=torch.int64, device=DEV)
        done = torch.zeros(1, dtype=torch.int32, device=DEV)
        for call in range(2):
            dst = torch.full((B, H, W, C), SENTINEL, device=DEV, dtype=bf)
            ld = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            oh = torch.full((B, NCLS), SENTINEL, device=DEV)
            pool = torch.full((4, 3000), 3.0, device=DEV)
            lens = (1, 7, 2600, 300)
            ops.augment_rows(src.to(DEV), dst, H, W, C, pad=pad, flip=True, mean=mean.to(DEV), inv_std=inv_std.to(DEV),
                             labels_src=lab.to(DEV), labels_dst=ld, seed=seed, counter=ctr, done=done,
                             zero=[pool[i, :n] for i, n in enumerate(lens)], onehot=oh, mix=mix, label_smoothing=E)
            torch.cuda.synchronize()
            c = c0 + call
            rows = mirror_rows(seed, c, B)
            A = construct(src, rows, H, W, C, pad, ops.augment_draws(seed, c, B, pad, True), mean, inv_std, f32)
            x, y = expected(A, lab[rows], ops.mix_draws(seed, c, B, H, W), mix, E, bf)
            assert torch.equal(dst.cpu(), x), (c0, call)
            assert torch.equal(oh.cpu(), y) and torch.equal(ld.cpu().long(), lab[rows].long()), (c0, call)
            for i, n in enumerate(lens):
                assert bool((pool[i, :n] == 0).all()) and bool((pool[i, n:] == 3.0).all()), (i, n)
            assert int(ctr.item()) == c + 1 and int(done.item()) == 0


def _batcher(B, seed, mix, E, out=True):
    (tr_x, tr_y), _ = cifar.synthetic_arrays(n_train=40, n_test=8)
    import dataclasses

    aug = dataclasses.replace(cifar.Augment.cifar(tr_x), mix=mix, label_smoothing=E)
    x = torch.empty(B, 32, 32, 3, device=DEV, dtype=bf) if out else None
    return DeviceBatcher(DataSet(tr_x, tr_y, True, seed), DEV, B, one_hot=True, augment=aug, out=x,
                         sampling="device"), aug, tr_x, tr_y


def _mirror_batch(aug, tr_x, tr_y, seed, c, B):
    rows = torch.from_numpy(ops.shuffled_rows(seed, c, B, len(tr_x)))
    mean, inv_std = torch.from_numpy(aug.mean), torch.from_numpy(aug.inv_std)
    A = construct(torch.from_numpy(tr_x), rows, 32, 32, 3, 4, ops.augment_draws(seed, c, B, 4, True), mean, inv_std, f32)
    return expected(A, tr_y[rows.numpy()], ops.mix_draws(seed, c, B, 32, 32), aug.mix, aug.label_smoothing, bf)


def test_captured_batcher_replays_the_stream():
    """DeviceBatcher.next_batch() (device sampling, cutmix, E = 0.1) in a StepGraph: two eager warm-up calls,
    the capture's replay, then three replays - call k yields the mirror's batch of counter c + k."""
    B, seed, c = 16, 21, 5
    batcher, aug, tr_x, tr_y = _batcher(B, seed, "cutmix", 0.1)
    batcher.seek(c)
    runner = StepGraph(batcher.next_batch, warmup=2)
    for k in range(6):
        runner()
        torch.cuda.synchronize()
        assert (runner.graph is not None) == (k >= 2), runner.capture_error
        x, y = _mirror_batch(aug, tr_x, tr_y, seed, c + k, B)
        assert torch.equal(batcher.out.cpu(), x) and torch.equal(batcher.y.cpu(), y), k
        assert int(batcher.counter.item()) == c + k + 1
    assert runner.capture_error is None


@pytest.mark.parametrize("mix", ["mixup", "cutmix"])
def test_batcher_seek_continues_the_stream(mix):
    B, seed, k = 16, 21, 3
    fresh, aug, tr_x, tr_y = _batcher(B, seed, mix, 0.1)
    for _ in range(k + 1):
        fx, fy = fresh.next_batch()
    sought = _batcher(B, seed, mix, 0.1)[0]
    sought.seek(k)
    sx, sy = sought.next_batch()
    x, y = _mirror_batch(aug, tr_x, tr_y, seed, k, B)
    assert torch.equal(sx, fx) and torch.equal(sy, fy)
    assert torch.equal(sx.cpu(), x) and torch.equal(sy.cpu(), y)
    assert torch.equal(sought.y_int.cpu().long(), torch.from_numpy(tr_y[ops.shuffled_rows(seed, k, B, len(tr_x))]).long())


def test_resnet20_training_step_on_a_mixed_batch():
    soft_target_loss_matches(DEV, 16, 1e-4)


def test_cli_run_with_cutmix_and_smoothing(tmp_path):
    """The flags through the CLI with the batch draw captured into the step graph: finite soft-target losses
    and no new field in the metrics line."""
    keys = []
    for name, extra in (("plain", []), ("mixed", ["--mix", "cutmix", "--label_smoothing", "0.1"])):
        mj = tmp_path / (name + ".jsonl")
        rc = train.run("resnet20", ["--mode=local", "--device=cuda", "--synthetic", "--augment", "cifar", "--shuffle", "device",
                                    "--batch_size", "32", "--num_steps", "3", "--save_model_secs=0",
                                    "--metrics_jsonl=" + str(mj), "--model_dir=" + str(tmp_path / name)] + extra,
                       log=lambda *_: None)
        rows = [json.loads(line) for line in mj.read_text().splitlines()]
        assert rc == 0 and [r["gs"] for r in rows] == [1, 2, 3]
        assert all(math.isfinite(r["loss"]) and r["loss"] > 0 for r in rows), rows
        keys.append([sorted(r) for r in rows])
    assert keys[0] == keys[1]
