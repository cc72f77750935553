"""augment_rows (csrc/kernels/augment.hip) on the GPU against the host mirror (ops.augment_draws) and
the np.pad construction of test_augment_cpu: every comparison is torch.equal.  Expectations never come
from another launch of the kernel under test."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.data import cifar
from dtfe.data.mnist import DataSet, DeviceBatcher
from dtfe.models.resnet import ResNetModel
from dtfe.utils.graphs import StepGraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import (SENTINEL, construct, eval_with_input_norm_matches_hand_standardised,  # noqa: E402
                              mirror_rows, run_case, source, stats)
from test_rng_streams_cpu import BIG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf = torch.bfloat16
u8, f32 = torch.uint8, torch.float32
STREAMS = [(seed, ctr) for seed in (3, 9) for ctr in (0, 5, BIG)]

# (32,32,3): the CIFAR shape; (8,8,3) with pad 7: nearly everything is border; (5,5,3): D = 75, the
# per-element kernel; (4,4,16): channels a multiple of the chunk; (6,4,1): uint8 rows of 24 bytes
SHAPES = [((32, 32, 3), (0, 1, 4)), ((8, 8, 3), (0, 1, 4, 7)), ((5, 5, 3), (0, 1, 4)), ((4, 4, 16), (0, 1, 3)),
          ((6, 4, 1), (0, 1, 3))]


def covers(draws, pad, flip=True):
    dy, dx, fl = draws
    ends = (dx == 0).any() and (dx == 2 * pad).any() and (dy == 0).any() and (dy == 2 * pad).any()
    return bool(ends and (fl.any() and (~fl).any() if flip else not fl.any()))


@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("shape,pads", SHAPES)
def test_augment_rows_equals_the_construction(B, shape, pads):
    """Per pad and flip: uint8 -> bf16 with statistics and sampled rows under all six (seed, counter)
    streams, and the other 15 combinations of source / destination dtype, statistics and explicit /
    sampled rows under one stream each (rotating through the six).  B = 130 with a pad: the mirror's
    draws must reach both ends of dx and dy and both flip values, so every edge is exercised."""
    combos = [(s, d, st, sm) for s in (u8, f32) for d in (bf, f32) for st in (True, False) for sm in (True, False)]
    assert combos[0] == (u8, bf, True, True)
    k = 0
    for pad in pads:
        for flip in (False, True):
            for i, (s, d, st, sm) in enumerate(combos):
                for seed, ctr in (STREAMS if i == 0 else [STREAMS[(k + i) % 6]]):
                    draws = run_case(DEV, B, shape, pad, flip, s, d, st, sm, seed, ctr)
                    if B == 130 and pad:
                        assert covers(draws, pad, flip), (shape, pad, flip, seed, ctr)
            k += 1
    # counter=None is counter value 0
    run_case(DEV, B, shape, pads[1], True, u8, bf, True, True, 9, None)


def test_mirror_draws_cover_every_edge_at_b130():
    """The coverage the grid relies on, for every stream it uses; at (seed 9, counter 5, pad 4) no
    sample is the identity transform: a kernel that ignored the draws would be wrong on every row."""
    for seed, ctr in STREAMS:
        for pad in (1, 3, 4, 7):
            assert covers(ops.augment_draws(seed, ctr, 130, pad, True), pad), (seed, ctr, pad)
    dy, dx, fl = ops.augment_draws(9, 5, 130, 4, True)
    assert not ((dy == 4) & (dx == 4) & ~fl).any()


@pytest.mark.parametrize("dst_dtype", [bf, f32])
@pytest.mark.parametrize("shape", [(32, 32, 3), (5, 5, 3), (6, 4, 1)])
def test_identity_transform_is_gather_rows_bitwise(shape, dst_dtype):
    H, W, C = shape
    src, lab = source(H, W, C, u8)
    src, lab = src.to(DEV), lab.to(DEV)
    for B in (5, 130):
        for seed, ctr in ((3, 0), (9, BIG)):
            outs = []
            for op in ("gather", "augment"):
                dst = torch.full((B, H * W * C), SENTINEL, device=DEV, dtype=dst_dtype)
                ld = torch.full((B,), -1, dtype=torch.int32, device=DEV)
                c = torch.tensor([ctr], dtype=torch.int64, device=DEV)
                if op == "gather":
                    ops.gather_rows(src, dst, None, lab, ld, seed=seed, counter=c)
                else:
                    ops.augment_rows(src, dst, H, W, C, labels_src=lab, labels_dst=ld, seed=seed, counter=c)
                outs.append((dst, ld))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (B, seed, ctr)
            assert bool((outs[1][0] != SENTINEL).all())


@pytest.mark.parametrize("shape", [(32, 32, 3), (5, 5, 3)])
def test_labels_onehot_zero_ranges_and_counter_advance(shape):
    """Two launches back to back with the ticket: the mirror's batches of counters c and c + 1, labels and
    one-hot rows of the sampled rows, four zero ranges cleared (their neighbours not), the counter
    advanced by exactly 1 per launch and the ticket word back at 0."""
    H, W, C = shape
    B, seed = 130, 9
    src, lab = source(H, W, C, u8)
    mean, inv_std = stats(C)
    for c0 in (5, BIG):
        ctr = torch.tensor([c0], dtype=torch.int64, device=DEV)
        done = torch.zeros(1, dtype=torch.int32, device=DEV)
        for call in range(2):
            dst = torch.full((B, H, W, C), SENTINEL, device=DEV, dtype=bf)
            ld = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            oh = torch.full((B, 10), SENTINEL, device=DEV)
            pool = torch.full((4, 3000), 3.0, device=DEV)
            lens = (1, 7, 2600, 300)
            ops.augment_rows(src.to(DEV), dst, H, W, C, pad=4 if H > 8 else 1, flip=True, mean=mean.to(DEV),
                             inv_std=inv_std.to(DEV), labels_src=lab.to(DEV), labels_dst=ld, seed=seed, counter=ctr,
                             done=done, zero=[pool[i, :n] for i, n in enumerate(lens)], onehot=oh)
            torch.cuda.synchronize()
            pad = 4 if H > 8 else 1
            rows = mirror_rows(seed, c0 + call, B)
            exp = construct(src, rows, H, W, C, pad, ops.augment_draws(seed, c0 + call, B, pad, True), mean, inv_std, bf)
            assert torch.equal(dst.cpu(), exp), (c0, call)
            assert torch.equal(ld.cpu().long(), lab[rows].long())
            assert torch.equal(oh.cpu(), torch.nn.functional.one_hot(lab[rows].long(), 10).float())
            for i, n in enumerate(lens):
                assert bool((pool[i, :n] == 0).all()) and bool((pool[i, n:] == 3.0).all()), (i, n)
            assert int(ctr.item()) == c0 + call + 1 and int(done.item()) == 0


def test_captured_launch_replays_the_stream():
    """One augment_rows launch in a StepGraph (a single-kernel graph): two eager warm-up calls, the
    capture's replay, then three replays - call k produces the mirror's batch of counter value k."""
    H, W, C, B, seed = 32, 32, 3, 130, 3
    src, lab = source(H, W, C, u8)
    mean, inv_std = stats(C)
    dsrc, dlab, dm, ds = src.to(DEV), lab.to(DEV), mean.to(DEV), inv_std.to(DEV)
    dst = torch.empty(B, H, W, C, device=DEV, dtype=bf)
    oh = torch.empty(B, 10, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    runner = StepGraph(lambda: ops.augment_rows(dsrc, dst, H, W, C, pad=4, flip=True, mean=dm, inv_std=ds, labels_src=dlab,
                                                seed=seed, counter=ctr, done=done, onehot=oh), warmup=2)
    for k in range(6):
        runner()
        torch.cuda.synchronize()
        assert (runner.graph is not None) == (k >= 2), runner.capture_error
        rows = mirror_rows(seed, k, B)
        exp = construct(src, rows, H, W, C, 4, ops.augment_draws(seed, k, B, 4, True), mean, inv_std, bf)
        assert torch.equal(dst.cpu(), exp), k
        assert torch.equal(oh.cpu(), torch.nn.functional.one_hot(lab[rows].long(), 10).float()), k
        assert int(ctr.item()) == k + 1
    assert runner.capture_error is None


def test_device_batcher_augments_into_the_program_buffer():
    B, seed = 8, 21
    (tr_x, tr_y), _ = cifar.synthetic_arrays(n_train=40, n_test=8)
    prog = ResNetModel(arch="resnet20").program(DEV, B, seed=0)
    aug = cifar.Augment.cifar(tr_x)
    ds = DataSet(tr_x, tr_y, True, seed)
    handed = []
    nxt = ds.next_batch_indices
    ds.next_batch_indices = lambda n: handed.append(nxt(n)) or handed[-1]
    batcher = DeviceBatcher(ds, DEV, B, one_hot=True, augment=aug, out=prog.x)
    mean, inv_std = torch.from_numpy(aug.mean), torch.from_numpy(aug.inv_std)
    for k in range(3):
        x, y = batcher.next_batch()
        assert x is prog.x and prog.x.dtype == bf
        prog.load_batch((x, y))  # no copy onto itself; the labels reach the program
        torch.cuda.synchronize()
        rows = torch.from_numpy(handed[k].astype(np.int64))
        exp = construct(torch.from_numpy(tr_x), rows, 32, 32, 3, 4, ops.augment_draws(seed, k, B, 4, True), mean,
                        inv_std, bf)
        onehot = torch.nn.functional.one_hot(torch.from_numpy(tr_y[rows.numpy()]), 10).float()
        assert torch.equal(prog.x.cpu(), exp), k
        assert torch.equal(y.cpu(), onehot) and torch.equal(prog.y.cpu(), onehot), k
        assert int(batcher.aug_ctr.item()) == k + 1
    assert len(handed) == 3
    with pytest.raises(ValueError, match="augment"):
        DeviceBatcher(ds, DEV, B, out=prog.x)


def test_resnet_evaluate_with_input_norm_gpu():
    eval_with_input_norm_matches_hand_standardised(DEV, 8)


def test_cli_run_with_augment_cifar(tmp_path):
    mj = tmp_path / "m.jsonl"
    rc = train.run("resnet20", ["--mode=local", "--device=cuda", "--synthetic", "--augment", "cifar", "--batch_size", "128",
                                "--num_steps", "3", "--save_model_secs=0", "--metrics_jsonl=" + str(mj),
                                "--model_dir=" + str(tmp_path / "ck")], log=lambda *_: None)
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    assert rc == 0 and [r["gs"] for r in rows] == [1, 2, 3]
    assert all(math.isfinite(r["loss"]) and r["loss"] > 0 for r in rows), rows
