"""Epoch-exact batch sampling on the GPU: gather_rows / augment_rows with shuffle=True against the host
mirror (ops.shuffled_rows, itself checked against its definition in test_shuffle_cpu), the device-mode
DeviceBatcher under graph replay, and the training CLI with --shuffle device / --steps_per_graph.
Kernel comparisons are torch.equal; expectations never come from another launch of the kernel under test."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.data import cifar
from dtfe.data.mnist import DataSet, DeviceBatcher
from dtfe.models.autoencoder import AutoencoderModel
from dtfe.models.lstm import LstmModel
from dtfe.models.resnet import ResNetModel
from dtfe.utils import flags as flagmod
from dtfe.utils.graphs import StepGraph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "launch"))
import local_cluster  # noqa: E402
from test_augment_cpu import construct  # noqa: E402
from test_rng_streams_cpu import BIG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf, u8, f32 = torch.bfloat16, torch.uint8, torch.float32
SENTINEL = -7.0

# n = 1: every draw is row 0; 5 < B = 130: a batch spans 26 epochs; 130 / 257: straddles; 4097: just
# above a power of 4 (the worst domain / n ratio, 4 walks on average); 4096: the exact power of 4
SIZES = [1, 5, 130, 257, 4097]
COUNTERS = [0, 5, BIG]
DTYPES = [(u8, f32), (u8, bf), (f32, f32), (f32, bf)]
POOL_N, POOL_D = 4097, 3072
_POOL = {}


def pool(dtype):
    """One [POOL_N][POOL_D] pool per source dtype (and the labels), on the host and on the device; a
    case's source is its leading [n][D] block."""
    if not _POOL:
        g = torch.Generator().manual_seed(20)
        _POOL[u8] = torch.randint(0, 256, (POOL_N, POOL_D), generator=g, dtype=u8)
        _POOL[f32] = torch.randn(POOL_N, POOL_D, generator=g)
        _POOL["lab"] = torch.randint(0, 10, (POOL_N,), generator=g, dtype=torch.int32)
    return _POOL[dtype], _POOL["lab"]


def block(dtype, n, D):
    key = (dtype, n, D)
    if key not in _POOL:
        src, lab = pool(dtype)
        host = src[:n, :D].contiguous()
        _POOL[key] = (host, lab[:n].contiguous(), host.to(DEV), lab[:n].to(DEV))
    return _POOL[key]


def expected_rows(src, rows, dst_dtype):
    """The gather's arithmetic: a byte times float32(1 / 255), one rounding; floats as they are."""
    v = src[rows]
    if v.dtype == u8:
        v = v.float() * torch.tensor(float(np.float32(1.0) / np.float32(255.0)))
    return v.to(dst_dtype)


def gather_case(n, D, B, ctr, seed, sd, dd, shuffle=True):
    src, lab, dsrc, dlab = block(sd, n, D)
    full = torch.full((B + 2, D), SENTINEL, dtype=dd, device=DEV)
    ld = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    oh = torch.full((B, 10), SENTINEL, device=DEV)
    z = torch.ones(37, device=DEV)
    counter = torch.tensor([ctr], dtype=torch.int64, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.gather_rows(dsrc, full[:B], None, dlab, ld, seed=seed, counter=counter, done=done, zero=(z,), onehot=oh,
                    shuffle=shuffle)
    if shuffle:
        rows = torch.from_numpy(ops.shuffled_rows(seed, ctr, B, n))
    else:
        rows = torch.from_numpy((ops.hash_u32(seed, np.uint64(ctr * B) + np.arange(B, dtype=np.uint64))
                                 % np.uint32(n)).astype(np.int64))
    what = (n, D, B, ctr, seed, sd, dd, shuffle)
    assert torch.equal(full[:B].cpu(), expected_rows(src, rows, dd)), what
    assert bool((full[B:] == SENTINEL).all()), ("stored past row B", what)
    assert torch.equal(ld.cpu(), lab[rows]), what
    assert torch.equal(oh.cpu(), torch.nn.functional.one_hot(lab[rows].long(), 10).float()), what
    assert not bool(z.any()), what
    assert int(counter.item()) == ctr + 1 and int(done.item()) == 0, what
    return rows


@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("D", [24, 75, 3072])
def test_gather_rows_shuffle_equals_the_mirror(B, D):
    """D = 24: the 8-element item path with several rows per 256-item window; 75: one wave per row;
    3072: one or two rows per window.  The full product: every n, counter, dtype pair and both seeds."""
    for n in SIZES:
        for ctr in COUNTERS:
            for sd, dd in DTYPES:
                for seed in (3, 9):
                    gather_case(n, D, B, ctr, seed, sd, dd)
    rows = gather_case(4096, D, B, 5, 3, u8, bf)  # the domain is exactly n: no walk
    assert len(set(rows.tolist())) == min(B, 4096)


@pytest.mark.parametrize("D", [24, 75, 3072])
def test_gather_rows_without_shuffle_is_unchanged(D):
    """shuffle=False (and the default): the with-replacement stream hash_u32(seed, c * B + b) % n."""
    for ctr in COUNTERS:
        for sd, dd in DTYPES:
            gather_case(257, D, 130, ctr, 9, sd, dd, shuffle=False)
    src, lab, dsrc, dlab = block(u8, 257, D)
    a, b = torch.empty(130, D, device=DEV), torch.empty(130, D, device=DEV)
    ops.gather_rows(dsrc, a, None, seed=9, counter=torch.tensor([5], device=DEV))
    ops.gather_rows(dsrc, b, None, seed=9, counter=torch.tensor([5], device=DEV), shuffle=False)
    assert torch.equal(a, b)


def augment_case(shape, pad, n, B, ctr, seed, sd, dd, shuffle=True):
    H, W, C = shape
    D = H * W * C
    src, lab, dsrc, dlab = block(sd, n, D)
    g = torch.Generator().manual_seed(C)
    mean, inv_std = torch.rand(C, generator=g) * 0.5 + 0.25, torch.rand(C, generator=g) * 3 + 1
    full = torch.full((B + 2, H, W, C), SENTINEL, dtype=dd, device=DEV)
    ld = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    oh = torch.full((B, 10), SENTINEL, device=DEV)
    z = torch.ones(37, device=DEV)
    counter = torch.tensor([ctr], dtype=torch.int64, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.augment_rows(dsrc, full[:B], H, W, C, pad=pad, flip=True, mean=mean.to(DEV), inv_std=inv_std.to(DEV),
                     labels_src=dlab, labels_dst=ld, seed=seed, counter=counter, done=done, zero=(z,), onehot=oh,
                     shuffle=shuffle)
    if shuffle:
        rows = torch.from_numpy(ops.shuffled_rows(seed, ctr, B, n))
    else:
        rows = torch.from_numpy((ops.hash_u32(seed, np.uint64(ctr * B) + np.arange(B, dtype=np.uint64))
                                 % np.uint32(n)).astype(np.int64))
    exp = construct(src, rows, H, W, C, pad, ops.augment_draws(seed, ctr, B, pad, True), mean, inv_std, dd)
    what = (shape, pad, n, B, ctr, seed, sd, dd, shuffle)
    assert torch.equal(full[:B].cpu(), exp), what
    assert bool((full[B:] == SENTINEL).all()), ("stored past row B", what)
    assert torch.equal(ld.cpu(), lab[rows]), what
    assert torch.equal(oh.cpu(), torch.nn.functional.one_hot(lab[rows].long(), 10).float()), what
    assert not bool(z.any()), what
    assert int(counter.item()) == ctr + 1 and int(done.item()) == 0, what


@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("shape,pad", [((32, 32, 3), 4), ((5, 5, 3), 1)])
def test_augment_rows_shuffle_equals_the_mirror(B, shape, pad):
    """(32, 32, 3): the one-workgroup-per-image LDS kernel; (5, 5, 3): the per-element kernel (D = 75).
    Rows from the permutation, crop / flip draws as without it.  Every n, counter and dtype pair; the
    seed alternates with n and the pair, so every counter and every pair meets both seeds."""
    for ni, n in enumerate(SIZES):
        for ctr in COUNTERS:
            for di, (sd, dd) in enumerate(DTYPES):
                augment_case(shape, pad, n, B, ctr, (3, 9)[(ni + di) % 2], sd, dd)
    augment_case(shape, pad, 4096, B, 5, 3, u8, bf)
    for sd, dd in DTYPES:  # the unchanged path
        augment_case(shape, pad, 257, B, 5, 9, sd, dd, shuffle=False)


def test_shuffle_with_idx_raises_on_the_device():
    src, lab, dsrc, dlab = block(u8, 130, 75)
    idx = torch.zeros(5, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="shuffle"):
        ops.gather_rows(dsrc, torch.empty(5, 75, device=DEV), idx, shuffle=True)
    with pytest.raises(ValueError, match="shuffle"):
        ops.augment_rows(dsrc, torch.empty(5, 5, 5, 3, device=DEV), 5, 5, 3, idx=idx, shuffle=True)


# -------------------------------------------------------------- the batcher
def test_device_batcher_under_graph_replay():
    """n = 37, B = 5: a StepGraph around next_batch (two eager calls, the capture's replay, replays):
    call k yields the mirror's batch k, across seven epoch boundaries; the counter counts launches."""
    g = np.random.RandomState(37)
    ds = DataSet(g.randint(0, 256, size=(37, 24)).astype(np.uint8), g.randint(0, 10, size=37), True, 11)
    batcher = DeviceBatcher(ds, DEV, 5, sampling="device")
    runner = StepGraph(batcher.next_batch, warmup=2)
    for k in range(22):
        runner()
        torch.cuda.synchronize()
        assert (runner.graph is not None) == (k >= 2), runner.capture_error
        rows = ops.shuffled_rows(11, k, 5, 37)
        assert torch.equal(batcher.x.cpu(), expected_rows(torch.from_numpy(ds.images_u8), torch.from_numpy(rows), f32)), k
        assert torch.equal(batcher.y.cpu(), torch.nn.functional.one_hot(torch.from_numpy(ds.labels_int[rows]), 10).float()), k
        assert torch.equal(batcher.y_int.cpu().long(), torch.from_numpy(ds.labels_int[rows])), k
        assert int(batcher.counter.item()) == k + 1
    assert runner.capture_error is None and batcher.epochs_completed == 22 * 5 // 37 and ds.epochs_completed == 0
    batcher.seek(3)
    runner()
    torch.cuda.synchronize()
    rows = ops.shuffled_rows(11, 3, 5, 37)
    assert torch.equal(batcher.y_int.cpu().long(), torch.from_numpy(ds.labels_int[rows]))


# ------------------------------------------------------------------ the CLI
def _run(model_cls, name, tmp_path, tag, extra, lr):
    m0 = model_cls()
    argv = ["--device=cuda", "--synthetic", "--batch_size=8", "--save_model_secs=0", "--num_steps=7", "--seed=3",
            "--shuffle=device", "--model_dir=" + str(tmp_path / tag)] + extra
    fl = flagmod.parse(argv, model_defaults=dict(batch_size=m0.default_batch, num_steps=m0.default_steps, learning_rate=lr))
    logs = []
    prog, opts, gstep = train.run_allreduce(fl, model_cls(lr=fl.learning_rate), torch.device("cuda", 0), logs.append)
    torch.cuda.synchronize()
    return prog, opts, int(gstep.item()), logs


@pytest.mark.parametrize("model_cls,name", [(AutoencoderModel, "encoder"), (LstmModel, "lstm")])
def test_cli_steps_per_graph_changes_nothing(model_cls, name, tmp_path):
    one = _run(model_cls, name, tmp_path, "one", [], 0.01)
    three = _run(model_cls, name, tmp_path, "three", ["--steps_per_graph=3"], 0.01)
    for prog, _opts, gs, logs in (one, three):
        assert gs == 7 and prog.step_runner.graph is not None, logs
        assert prog.step_runner.capture_error is None and not any("capture_error" in l for l in logs), logs
    assert three[0].step_runner.many.graph is not None  # two 3-step replays ran, then one step
    assert torch.equal(one[0].P.master, three[0].P.master)
    for oa, ob in zip(one[1], three[1]):
        ta, tb = oa.slot_tensors(), ob.slot_tensors()
        assert ta.keys() == tb.keys() and all(torch.equal(ta[k].cpu(), tb[k].cpu()) for k in ta)


@pytest.mark.parametrize("name", ["softmax", "gan", "cnn"])
def test_cli_batch_draw_is_captured(name, tmp_path):
    """The other models' load_batch inside the captured step: a graph, no capture error, the step count."""
    logs = []
    rc = train.run(name, ["--mode=local", "--device=cuda", "--synthetic", "--batch_size=8", "--save_model_secs=0",
                          "--num_steps=6", "--shuffle=device", "--model_dir=" + str(tmp_path / "ck")]
                   + (["--steps_per_graph=2"] if name != "cnn" else []), log=logs.append)
    assert rc == 0 and not any("capture_error" in l for l in logs), logs
    gs = [int(m.group(1)) for l in logs for m in [re.match(r"Global step (\d+) Local step", l)] if m]
    assert gs[-1] == 6, logs


def test_cli_resnet20_augmented_multi_step(tmp_path):
    mj = tmp_path / "m.jsonl"
    m0 = ResNetModel(0.1, "resnet20")
    fl = flagmod.parse(["--device=cuda", "--synthetic", "--batch_size=8", "--augment=cifar", "--shuffle=device",
                        "--steps_per_graph=3", "--num_steps=7", "--save_model_secs=0", "--seed=3",
                        "--metrics_jsonl=" + str(mj), "--model_dir=" + str(tmp_path / "ck")],
                       model_defaults=dict(batch_size=m0.default_batch, num_steps=m0.default_steps, learning_rate=0.1))
    logs = []
    prog, opts, gstep = train.run_allreduce(fl, ResNetModel(0.1, "resnet20"), torch.device("cuda", 0), logs.append)
    torch.cuda.synchronize()
    assert int(gstep.item()) == 7
    assert prog.step_runner.many.graph is not None and prog.step_runner.capture_error is None
    assert not any("capture_error" in l for l in logs), logs
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    assert [(r["gs"], r["steps"]) for r in rows] == [(3, 3), (6, 3), (7, 1)]
    assert all(math.isfinite(r["loss"]) and r["loss"] > 0 for r in rows), rows
    assert all("epoch" in r for r in rows)
    # the last step's batch: the mirror's batch at counter 6 of the rank's data seed
    data = train.read_data_sets(prog.model, "", one_hot=True, seed=3 * 1000 + 1, log=lambda *_: None)
    tr = data.train
    aug = cifar.Augment.cifar(tr.images_u8)
    pick = torch.from_numpy(ops.shuffled_rows(tr.seed, 6, 8, tr.num_examples))
    exp = construct(torch.from_numpy(tr.images_u8), pick, 32, 32, 3, 4, ops.augment_draws(tr.seed, 6, 8, 4, True),
                    torch.from_numpy(aug.mean), torch.from_numpy(aug.inv_std), prog.x.dtype)
    assert torch.equal(prog.x.cpu().reshape(exp.shape), exp)
    assert torch.equal(prog.y.cpu(), torch.nn.functional.one_hot(torch.from_numpy(tr.labels_int[pick.numpy()]), 10).float())


def test_two_ranks_multi_step_ipc_in_graph(tmp_path):
    """--mode=allreduce, 2 workers sharing cuda:0, the IPC all-reduce inside 3-step replays: both ranks
    end at step 7 with the same parameters (each rank draws from its own data seed)."""
    extra = ["--mode=allreduce", "--device=cuda", "--backend=gloo", "--comm=ipc", "--synthetic", "--num_steps=7",
             "--batch_size=16", "--model_dir=" + str(tmp_path / "ck"), "--save_model_secs=0", "--shuffle=device",
             "--steps_per_graph=3", "--check_pull"]
    codes, out, _ = local_cluster.launch("encoder", 0, 2, extra, timeout=600, stream=False, gpus=1)
    assert all(c == 0 for c in codes.values()), "%s\n%s" % (codes, "\n".join(
        "---- %s\n%s" % (k, "\n".join(v[-40:])) for k, v in out.items()))
    for w in (0, 1):
        gs = [int(m.group(1)) for l in out[("worker", w)] for m in [re.match(r"Global step (\d+) Local step", l)] if m]
        assert gs[-1] == 7, out[("worker", w)]
        assert not any("capture_error" in l for l in out[("worker", w)])
        # the 3-step graph was captured (with more than one rank only a step with in-graph comm is)
        assert "hip_graph: captured 3 steps per replay" in out[("worker", w)], out[("worker", w)]
    sums = [[l for l in out[("worker", w)] if l.startswith("params checksum")] for w in (0, 1)]
    assert sums[0] and sums[0] == sums[1], sums
