"""Epoch-exact batch sampling on the CPU: the host mirror of the device's keyed permutation
(ops.epoch_permutation / ops.shuffled_rows) against its definition written here with Python integers,
the CPU paths of gather_rows / augment_rows with shuffle=True, DeviceBatcher(sampling="device") on host
tensors, and the training CLI's --shuffle / --steps_per_graph on --device=cpu.  Everything is exact."""
import json
import os

import numpy as np
import pytest
import torch

from dtfe import ckpt, ops, train
from dtfe.data import cifar
from dtfe.data.mnist import DataSet, DeviceBatcher
from dtfe.models.autoencoder import AutoencoderModel
from dtfe.utils import flags as flagmod

from test_augment_cpu import construct
from test_rng_streams_cpu import BIG

M64 = (1 << 64) - 1
SIZES = [1, 2, 3, 5, 130, 257, 4096, 4097, 50000]
SEEDS = (1, 3, 9)
EPOCHS = (0, 1, (1 << 40) + 3)


# ------------------------------------------------------------ the definition
def hash_def(seed, idx):
    """common.h hash_u32 with Python integers."""
    z = (seed * 0x9E3779B97F4A7C15 + idx * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & 0xFFFFFFFF


def perm_def(seed, epoch, n, i):
    """common.h perm_index(seed ^ SHUF_SALT, epoch, n, i), one element, as the header writes it out."""
    key = (seed & M64) ^ 0x5EED0FE90C45A1D3
    bits = max(2, ((n - 1).bit_length() + 1) // 2 * 2)
    h = bits // 2
    mask = (1 << h) - 1
    x = i
    while True:
        L, R = x >> h, x & mask
        for r in range(4):
            L, R = R, L ^ (hash_def(key, ((epoch << 18) & M64) | (r << 16) | R) & mask)
        x = (L << h) | R
        if x < n:
            return x


def test_hash_def_is_the_host_hash():
    idx = [0, 1, 63, 2**31, 2**32 + 1, BIG * 65536 + 17, 2**64 - 1]
    for seed in (0, 5, 2**63 + 9):
        assert [hash_def(seed, i) for i in idx] == ops.hash_u32(seed, np.array(idx, dtype=np.uint64)).tolist()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 130, 257, 4097])
def test_mirror_equals_the_definition(n):
    for seed in SEEDS:
        for epoch in EPOCHS:
            got = ops.epoch_permutation(seed, epoch, n)
            assert got.dtype == np.int64 and got.shape == (n,)
            pick = range(n) if n <= 257 else list(range(0, n, 97)) + [n - 1]
            assert [int(got[i]) for i in pick] == [perm_def(seed, epoch, n, i) for i in pick], (n, seed, epoch)
    assert ops.SHUF_SALT == 0x5EED0FE90C45A1D3 and ops.SHUF_SALT != ops.AUG_SALT


def test_mirror_at_the_largest_domain():
    """n = 2^31 (32-bit domain, h = 16): a few elements of the mirror's element-wise form."""
    n = 1 << 31
    i = np.array([0, 1, 12345, n - 1], dtype=np.uint64)
    got = ops._perm_index(3 ^ ops.SHUF_SALT, np.uint64(7), n, i)
    assert got.tolist() == [perm_def(3, 7, n, int(k)) for k in i]
    assert (got >= 0).all() and (got < n).all()
    for bad in (0, (1 << 31) + 1):
        with pytest.raises(ValueError):
            ops.epoch_permutation(1, 0, bad)
        with pytest.raises(ValueError):
            ops.shuffled_rows(1, 0, 4, bad)


@pytest.mark.parametrize("n", SIZES)
def test_epoch_permutation_is_a_permutation(n):
    for seed in SEEDS:
        for epoch in EPOCHS:
            p = ops.epoch_permutation(seed, epoch, n)
            assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch)


@pytest.mark.parametrize("n", [4096, 4097, 50000])
def test_permutations_are_not_degenerate(n):
    """Two epochs of a seed, and two seeds, agree in at most 8 positions (a random pair agrees in 1 on
    average), and at most 8 positions continue their predecessor (p[i + 1] == p[i] + 1; also 1 on
    average) - for the seeds the other tests use."""
    for seed in SEEDS:
        a, b, c = (ops.epoch_permutation(seed, 0, n), ops.epoch_permutation(seed, 1, n),
                   ops.epoch_permutation(seed + 1, 0, n))
        assert int((a == b).sum()) <= 8 and int((a == c).sum()) <= 8, (n, seed)
        for p in (a, b, c):
            assert int((p[1:] == p[:-1] + 1).sum()) <= 8, (n, seed)
            assert not np.array_equal(p, np.arange(n))


# ------------------------------------------------------------ shuffled_rows
def test_shuffled_rows_stitches_epochs():
    n, B, seed = 7, 5, 3
    stream = np.concatenate([ops.shuffled_rows(seed, c, B, n) for c in range(7)])  # 35 positions = 5 epochs
    for e in range(5):
        assert np.array_equal(stream[e * n:(e + 1) * n], ops.epoch_permutation(seed, e, n)), e
        assert np.array_equal(np.sort(stream[e * n:(e + 1) * n]), np.arange(n))
    # batch 1 = positions 5..9: the tail of epoch 0, then the head of epoch 1
    assert np.array_equal(ops.shuffled_rows(seed, 1, B, n),
                          np.concatenate([ops.epoch_permutation(seed, 0, n)[5:], ops.epoch_permutation(seed, 1, n)[:3]]))
    assert not np.array_equal(ops.epoch_permutation(seed, 0, n), ops.epoch_permutation(seed, 1, n))


def test_shuffled_rows_batch_larger_than_the_set():
    n, B, seed = 5, 130, 9
    for c in (0, 1, 4):
        rows = ops.shuffled_rows(seed, c, B, n)
        assert rows.shape == (B,) and rows.dtype == np.int64
        exp = np.concatenate([ops.epoch_permutation(seed, e, n) for e in range(c * B // n, (c * B + B) // n + 1)])
        off = c * B % n
        assert np.array_equal(rows, exp[off:off + B]), c
        assert (np.bincount(rows, minlength=n) == B // n).all()


def test_shuffled_rows_at_a_large_counter():
    n, B, seed = 37, 5, 3
    c = (1 << 40) + 11
    rows = ops.shuffled_rows(seed, c, B, n)
    for b in range(B):
        p = c * B + b
        assert int(rows[b]) == perm_def(seed, p // n, n, p % n), b
    # BIG * 130 positions into a 5-row set: epoch numbers beyond 2^36
    rows = ops.shuffled_rows(seed, BIG, 130, 5)
    assert [int(r) for r in rows[:12]] == [perm_def(seed, (BIG * 130 + b) // 5, 5, (BIG * 130 + b) % 5) for b in range(12)]


def test_one_epoch_of_shuffled_draws_repeats_no_row():
    """What the feature is for: the first n draws of the with-replacement stream repeat rows (about
    37 % of the rows are never drawn); the shuffled stream of the same seed draws each exactly once."""
    n, B, seed = 4000, 100, 1
    i = np.arange(n, dtype=np.uint64)
    replace = ops.hash_u32(seed, i) % np.uint32(n)
    assert len(np.unique(replace)) < 0.7 * n
    shuffled = np.concatenate([ops.shuffled_rows(seed, c, B, n) for c in range(n // B)])
    assert len(np.unique(shuffled)) == n


# ------------------------------------------------------------------ the ops
def _pool(n, D, seed=0):
    g = torch.Generator().manual_seed(seed + n * 31 + D)
    return (torch.randint(0, 256, (n, D), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), generator=g, dtype=torch.int32))


@pytest.mark.parametrize("n,B", [(37, 5), (5, 130)])
def test_gather_rows_cpu_shuffle(n, B):
    src, lab = _pool(n, 24)
    for seed in (3, 9):
        ctr = torch.tensor([4], dtype=torch.int64)
        done = torch.zeros(1, dtype=torch.int32)
        for c in (4, 5):
            dst = torch.empty(B, 24)
            ld = torch.full((B,), -1, dtype=torch.int32)
            oh = torch.full((B, 10), 7.0)
            z = torch.ones(6)
            ops.gather_rows(src, dst, None, lab, ld, seed=seed, counter=ctr, done=done, zero=(z,), onehot=oh, shuffle=True)
            rows = torch.from_numpy(ops.shuffled_rows(seed, c, B, n))
            assert torch.equal(dst, src[rows].float() / 255.0)
            assert torch.equal(ld, lab[rows])
            assert torch.equal(oh, torch.nn.functional.one_hot(lab[rows].long(), 10).float())
            assert not z.any() and int(ctr.item()) == c + 1
    # shuffle off: the with-replacement stream, as on the device
    dst = torch.empty(B, 24)
    ops.gather_rows(src, dst, None, lab, None, seed=3, counter=torch.tensor([4]))
    rows = torch.from_numpy((ops.hash_u32(3, np.uint64(4 * B) + np.arange(B, dtype=np.uint64)) % np.uint32(n)).astype(np.int64))
    assert torch.equal(dst, src[rows].float() / 255.0)


def test_augment_rows_cpu_shuffle():
    H, W, C, n, B, seed = 5, 5, 3, 37, 10, 9
    src, lab = _pool(n, H * W * C)
    mean, inv_std = torch.tensor([0.4, 0.5, 0.45]), torch.tensor([3.0, 4.0, 3.5])
    ctr = torch.tensor([3], dtype=torch.int64)
    done = torch.zeros(1, dtype=torch.int32)
    for c in (3, 4):  # batch 3 = positions 30..39 straddles the epoch boundary at 37
        dst = torch.empty(B, H, W, C)
        ld = torch.empty(B, dtype=torch.int32)
        oh = torch.empty(B, 10)
        ops.augment_rows(src, dst, H, W, C, pad=1, flip=True, mean=mean, inv_std=inv_std, labels_src=lab, labels_dst=ld,
                         seed=seed, counter=ctr, done=done, onehot=oh, shuffle=True)
        rows = torch.from_numpy(ops.shuffled_rows(seed, c, B, n))
        exp = construct(src, rows, H, W, C, 1, ops.augment_draws(seed, c, B, 1, True), mean, inv_std, torch.float32)
        assert torch.equal(dst, exp) and torch.equal(ld, lab[rows])
        assert torch.equal(oh, torch.nn.functional.one_hot(lab[rows].long(), 10).float())
    assert int(ctr.item()) == 5


def test_shuffle_with_idx_raises():
    src, lab = _pool(8, 75)
    idx = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="shuffle"):
        ops.gather_rows(src, torch.empty(4, 75), idx, shuffle=True)
    with pytest.raises(ValueError, match="shuffle"):
        ops.augment_rows(src, torch.empty(4, 5, 5, 3), 5, 5, 3, idx=idx, shuffle=True)


# -------------------------------------------------------------- the batcher
def _dataset(n=37, D=24, seed=11):
    g = np.random.RandomState(n)
    return DataSet(g.randint(0, 256, size=(n, D)).astype(np.uint8), g.randint(0, 10, size=n), True, seed)


def test_device_batcher_device_sampling_on_cpu():
    ds = _dataset()
    B = 5
    served = DeviceBatcher(ds, "cpu", B, sampling="device")
    assert served.epochs_completed == 0
    for k in range(9):
        x, y = served.next_batch()
        rows = ops.shuffled_rows(ds.seed, k, B, 37)
        assert torch.equal(x, torch.from_numpy(ds.images_u8[rows]).float() / 255.0), k
        assert torch.equal(y, torch.nn.functional.one_hot(torch.from_numpy(ds.labels_int[rows]), 10).float()), k
        assert int(served.counter.item()) == k + 1
        assert served.epochs_completed == (k + 1) * B // 37
    assert ds.epochs_completed == 0  # the host batcher was never asked
    sought = DeviceBatcher(ds, "cpu", B, sampling="device")
    sought.seek(9)
    a, b = served.next_batch(), sought.next_batch()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sought.seek(BIG)
    assert sought.epochs_completed == BIG * B // 37
    with pytest.raises(ValueError, match="seek"):
        DeviceBatcher(ds, "cpu", B).seek(3)
    with pytest.raises(ValueError, match="sampling"):
        DeviceBatcher(ds, "cpu", B, sampling="gpu")


def test_device_batcher_device_sampling_with_augment_on_cpu():
    (tr_x, tr_y), _ = cifar.synthetic_arrays(n_train=21, n_test=4)
    ds = DataSet(tr_x, tr_y, True, 5)
    aug = cifar.Augment.cifar(tr_x)
    served = DeviceBatcher(ds, "cpu", 8, augment=aug, sampling="device")
    sought = DeviceBatcher(ds, "cpu", 8, augment=aug, sampling="device")
    for _ in range(4):
        last = [t.clone() for t in served.next_batch()]
    sought.seek(3)
    x, y = sought.next_batch()
    assert torch.equal(x, last[0]) and torch.equal(y, last[1])
    rows = torch.from_numpy(ops.shuffled_rows(5, 3, 8, 21))
    exp = construct(torch.from_numpy(tr_x.reshape(21, -1)), rows, 32, 32, 3, 4, ops.augment_draws(5, 3, 8, 4, True),
                    torch.from_numpy(aug.mean), torch.from_numpy(aug.inv_std), torch.float32)
    assert torch.equal(x.reshape(exp.shape), exp)


# ------------------------------------------------------------------ the CLI
def test_flag_defaults_and_values():
    f = flagmod.parse([])
    assert f.shuffle == "host" and f.steps_per_graph == 1
    f = flagmod.parse(["--shuffle=device", "--steps_per_graph", "4"])
    assert f.shuffle == "device" and f.steps_per_graph == 4
    for bad in (["--shuffle=gpu"], ["--steps_per_graph=0"]):
        with pytest.raises(SystemExit):
            flagmod.parse(bad)


def test_gan_loss_line_under_replays():
    """The GAN (global_step advances by 2 per step) prints at steps 1000, 2000, ...: a replay prints when
    one of the steps it ran is such a step; one step per iteration prints exactly where it did."""
    from dtfe.models.gan import GanModel

    model = GanModel()
    assert model.gs_increments == 2
    m = {"gen_loss": torch.tensor(1.0), "disc_loss": torch.tensor(2.0)}

    def printed(step, ran):
        out = []
        train.model_step_hook(model, step, m, out.append, ran)
        return bool(out)

    assert printed(1000, 1) and printed(1, 1) and not printed(1002, 1) and not printed(998, 1)
    assert printed(1002, 3) and printed(1004, 3) and not printed(1006, 3) and not printed(998, 3)
    out = []
    train.model_step_hook(model, 1000, m, out.append)  # (the ps worker's call)
    assert out == ["Step 1000: Generator Loss: 1.000000, Discriminator Loss: 2.000000"]


BASE = ["--device=cpu", "--synthetic", "--batch_size=8", "--save_model_secs=0"]


@pytest.mark.parametrize("model,extra,what", [
    ("encoder", ["--steps_per_graph=3"], "--shuffle device"),
    ("encoder", ["--steps_per_graph=3", "--shuffle=host"], "--shuffle device"),
    ("encoder", ["--mode=ps", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", "--job_name=worker",
                 "--shuffle=device"], "--shuffle"),
    ("encoder", ["--mode=ps", "--ps_hosts=localhost:1", "--worker_hosts=localhost:2", "--job_name=worker",
                 "--shuffle=device", "--steps_per_graph=2"], "--steps_per_graph"),
    ("cnn", ["--shuffle=device", "--steps_per_graph=3"], "--bucket_mb"),
])
def test_cli_refusals(model, extra, what, tmp_path):
    with pytest.raises(ValueError, match=what):
        train.run(model, BASE + ["--num_steps=1", "--model_dir=" + str(tmp_path)] + extra, log=lambda *_: None)


def _run_encoder(tmp_path, name, extra, num_steps):
    m0 = AutoencoderModel()
    fl = flagmod.parse(BASE + ["--num_steps=%d" % num_steps, "--seed=3", "--model_dir=" + str(tmp_path / name)] + extra,
                       model_defaults=dict(batch_size=m0.default_batch, num_steps=m0.default_steps, learning_rate=0.01))
    logs = []
    prog, opts, gstep = train.run_allreduce(fl, AutoencoderModel(lr=fl.learning_rate), torch.device("cpu"), logs.append)
    return prog, opts, int(gstep.item()), logs


def _same_state(a, b):
    assert torch.equal(a[0].P.master, b[0].P.master)
    for oa, ob in zip(a[1], b[1]):
        ta, tb = oa.slot_tensors(), ob.slot_tensors()
        assert ta.keys() == tb.keys() and all(torch.equal(ta[k], tb[k]) for k in ta)


def test_cli_never_overshoots_num_steps(tmp_path):
    mj = tmp_path / "m.jsonl"
    prog, opts, gs, logs = _run_encoder(tmp_path, "a", ["--shuffle=device", "--steps_per_graph=3",
                                                        "--metrics_jsonl=" + str(mj)], 7)
    assert gs == 7
    rows = [json.loads(line) for line in mj.read_text().splitlines()]
    assert [(r["gs"], r["steps"], r["step"]) for r in rows] == [(3, 3, 2), (6, 3, 5), (7, 1, 6)]
    assert not any("capture_error" in l for l in logs)
    # the cnn leaves its own schedule for the generic path with --bucket_mb, and replays several there
    rc = train.run("cnn", BASE + ["--num_steps=4", "--shuffle=device", "--steps_per_graph=3", "--bucket_mb=4",
                                  "--model_dir=" + str(tmp_path / "c")], log=logs.append)
    assert rc == 0 and any(l.startswith("Global step 4 Local step 3") for l in logs)


def test_cli_steps_per_graph_changes_nothing(tmp_path):
    one = _run_encoder(tmp_path, "one", ["--shuffle=device"], 7)
    three = _run_encoder(tmp_path, "three", ["--shuffle=device", "--steps_per_graph=3"], 7)
    assert one[2] == three[2] == 7
    _same_state(one, three)
    host = _run_encoder(tmp_path, "host", [], 7)  # (the host order is another one)
    assert not torch.equal(host[0].P.master, one[0].P.master)


def test_cli_log_every_with_replays(tmp_path):
    _, _, gs, logs = _run_encoder(tmp_path, "l", ["--shuffle=device", "--steps_per_graph=3", "--log_every=4"], 10)
    # local steps 0..9 in replays [0-2] [3-5] [6-8] [9]: multiples of 4 lie in the 1st, 2nd and 3rd
    assert gs == 10
    assert [l.split("  AvgTime")[0] for l in logs if l.startswith("Global step")] == [
        "Global step 3 Local step 2", "Global step 6 Local step 5", "Global step 9 Local step 8"]


def test_cli_resume_continues_the_epoch_order(tmp_path):
    """A run restored at step 4 draws batches 4..7: with batch 8 over the synthetic set the rows are a
    function of the batch number alone, so the resumed run ends where the uninterrupted one does."""
    extra = ["--shuffle=device", "--steps_per_graph=3"]
    whole = _run_encoder(tmp_path, "whole", extra, 8)
    first = _run_encoder(tmp_path, "first", extra, 4)
    assert first[2] == 4
    md = tmp_path / "resumed"
    os.makedirs(md)
    model = AutoencoderModel(lr=0.01)
    ckpt.save_bundle(str(md / "model.ckpt-4"), train.tensors_from_flat(model, first[0].P, first[1], 4))
    ckpt.write_checkpoint_state(str(md), "model.ckpt-4", ["model.ckpt-4"])
    resumed = _run_encoder(tmp_path, "resumed", extra, 8)
    assert resumed[2] == whole[2] == 8
    _same_state(whole, resumed)
    assert not torch.equal(first[0].P.master, whole[0].P.master)
