"""The CIFAR input transforms (ops.augment_rows: crop of the zero-padded image, flip, per-channel
standardisation) on the CPU: the host mirror of the draws (ops.augment_draws), the CPU path of the op
against a construction written here with np.pad, argument errors, the data-layer records, the
--augment flag and ResNetProgram.evaluate with input statistics.  Everything compares with
torch.equal: the definition is exact (csrc/kernels/augment.h)."""
import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.data import cifar
from dtfe.models.resnet import ResNetModel
from dtfe.utils import flags as flagmod

from test_rng_streams_cpu import BIG

bf = torch.bfloat16
N_ROWS = 50
SENTINEL = -7.0
_SOURCES = {}


def source(H, W, C, dtype):
    """([N_ROWS][H*W*C] source rows, int32 labels [N_ROWS] in 0..9), the same for every test of a shape."""
    key = (H, W, C, dtype)
    if key not in _SOURCES:
        g = torch.Generator().manual_seed(H * 10007 + W * 101 + C)
        u8 = torch.randint(0, 256, (N_ROWS, H * W * C), generator=g, dtype=torch.uint8)
        f32 = torch.randn(N_ROWS, H * W * C, generator=g)
        lab = torch.randint(0, 10, (N_ROWS,), generator=g, dtype=torch.int32)
        _SOURCES[(H, W, C, torch.uint8)] = (u8, lab)
        _SOURCES[(H, W, C, torch.float32)] = (f32, lab)
    return _SOURCES[key]


def stats(C):
    g = torch.Generator().manual_seed(C)
    return torch.rand(C, generator=g) * 0.5 + 0.25, torch.rand(C, generator=g) * 3 + 1


def mirror_rows(seed, step, B, n_rows=N_ROWS):
    i = np.uint64(step * B) + np.arange(B, dtype=np.uint64)
    return torch.from_numpy((ops.hash_u32(seed, i) % np.uint32(n_rows)).astype(np.int64))


def construct(src, rows, H, W, C, pad, draws, mean, inv_std, dst_dtype):
    """The expected batch [B][H][W][C], from the definition: scale bytes by float32(1/255), standardise
    in float32 (subtract, then multiply: two roundings), np.pad the image with zeros (the border is zero
    AFTER standardisation), slice the (dy, dx) window, reverse axis 1 where flipped, round with torch."""
    dy, dx, fl = draws
    img = src[rows].numpy().reshape(len(rows), H, W, C)
    if img.dtype == np.uint8:
        img = img.astype(np.float32) * np.float32(1.0 / 255.0)
    if mean is not None:
        img = (img - mean.numpy().reshape(1, 1, 1, C)) * inv_std.numpy().reshape(1, 1, 1, C)
    assert img.dtype == np.float32
    padded = np.pad(img, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = np.empty_like(img)
    for b in range(len(rows)):
        win = padded[b, dy[b]:dy[b] + H, dx[b]:dx[b] + W]
        out[b] = win[:, ::-1] if fl[b] else win
    return torch.from_numpy(out).to(dst_dtype)


def run_case(dev, B, shape, pad, flip, src_dtype, dst_dtype, with_stats, sampled, seed, ctr, extra_rows=2):
    """One launch into the first B rows of a sentinel-filled [B + extra_rows] destination; checks the
    batch against construct(), the sentinel rows, the labels and an unchanged counter (no ``done``)."""
    H, W, C = shape
    src, lab = source(H, W, C, src_dtype)
    mean, inv_std = stats(C) if with_stats else (None, None)
    rows = mirror_rows(seed, ctr or 0, B) if sampled else (torch.arange(B) * 7 + 3) % N_ROWS
    full = torch.full((B + extra_rows, H, W, C), SENTINEL, dtype=dst_dtype, device=dev)
    ld = torch.full((B,), -1, dtype=torch.int32, device=dev)
    counter = None if ctr is None else torch.tensor([ctr], dtype=torch.int64, device=dev)
    ops.augment_rows(src.to(dev), full[:B], H, W, C, pad=pad, flip=flip,
                     mean=None if mean is None else mean.to(dev), inv_std=None if inv_std is None else inv_std.to(dev),
                     idx=None if sampled else rows.int().to(dev), labels_src=lab.to(dev), labels_dst=ld, seed=seed,
                     counter=counter)
    draws = ops.augment_draws(seed, ctr or 0, B, pad, flip)
    exp = construct(src, rows, H, W, C, pad, draws, mean, inv_std, dst_dtype)
    what = (B, shape, pad, flip, src_dtype, dst_dtype, with_stats, sampled, seed, ctr)
    assert torch.equal(full[:B].cpu(), exp), what
    assert bool((full[B:] == SENTINEL).all()), ("stored past row B", what)
    assert torch.equal(ld.cpu().long(), lab[rows].long()), what
    if counter is not None:
        assert int(counter.item()) == ctr, ("advanced without a ticket", what)
    return draws


def pads_of(shape, pads=(0, 1, 4)):
    return [p for p in pads if p < min(shape[0], shape[1])]


# ------------------------------------------------------------------ draws
def test_augment_draws_ranges_and_switches():
    for pad in (0, 1, 4, 15):
        for step in (0, 5, BIG):
            dy, dx, fl = ops.augment_draws(7, step, 1000, pad, True)
            assert dy.shape == dx.shape == fl.shape == (1000,) and fl.dtype == bool
            assert dy.min() >= 0 and dy.max() <= 2 * pad and dx.min() >= 0 and dx.max() <= 2 * pad
            if pad == 0:
                assert not dy.any() and not dx.any()
            else:
                assert dy.max() == 2 * pad and dx.max() == 2 * pad and dy.min() == 0 and dx.min() == 0
            assert fl.any() and not fl.all()
            off = ops.augment_draws(7, step, 1000, pad, False)
            assert not off[2].any() and np.array_equal(off[0], dy) and np.array_equal(off[1], dx)
    a, b = ops.augment_draws(7, 0, 1000, 4, True), ops.augment_draws(7, 1, 1000, 4, True)
    assert not np.array_equal(a[1], b[1])
    # one stream over steps: sample b of step s is element s * B + b
    two = ops.augment_draws(7, 0, 2000, 4, True)
    assert all(np.array_equal(two[k][1000:], b[k]) for k in range(3))
    assert ops.AUG_SALT == 0xC1FA5A17D00D5EED


def test_augment_draws_outcomes_are_uniform():
    """64800 draws over the 9 * 9 * 2 outcomes of pad 4: 400 expected each (sd 20), 400 +- 100 asked."""
    dy, dx, fl = ops.augment_draws(7, 0, 64800, 4, True)
    counts = np.bincount((dy * 9 + dx) * 2 + fl, minlength=162)
    assert len(counts) == 162 and counts.min() >= 300 and counts.max() <= 500, (counts.min(), counts.max())


# ---------------------------------------------------------------- CPU path
@pytest.mark.parametrize("shape", [(32, 32, 3), (5, 5, 3), (4, 4, 16)])
@pytest.mark.parametrize("flip", [False, True])
def test_augment_rows_cpu_equals_the_construction(shape, flip):
    n = 0
    for pad in pads_of(shape):
        for src_dtype in (torch.uint8, torch.float32):
            for dst_dtype in (torch.float32, bf):
                for with_stats in (False, True):
                    for sampled in (False, True):
                        for ctr in (None, 0, 5, BIG):
                            run_case("cpu", 6, shape, pad, flip, src_dtype, dst_dtype, with_stats, sampled, 3, ctr)
                            n += 1
    assert n == len(pads_of(shape)) * 64


def test_augment_rows_cpu_labels_onehot_zero_ranges_and_counter():
    H, W, C, B = 5, 5, 3, 6
    src, lab = source(H, W, C, torch.uint8)
    mean, inv_std = stats(C)
    ctr, done = torch.tensor([5], dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for call in range(2):
        dst = torch.empty(B, H, W, C)
        ld = torch.full((B,), -1, dtype=torch.int32)
        oh = torch.full((B, 10), SENTINEL)
        zs = [torch.full((n,), 3.0) for n in (1, 7, 64, 5)]
        ops.augment_rows(src, dst, H, W, C, pad=1, flip=True, mean=mean, inv_std=inv_std, labels_src=lab,
                         labels_dst=ld, seed=9, counter=ctr, done=done, zero=zs, onehot=oh)
        rows = mirror_rows(9, 5 + call, B)
        exp = construct(src, rows, H, W, C, 1, ops.augment_draws(9, 5 + call, B, 1, True), mean, inv_std, torch.float32)
        assert torch.equal(dst, exp), call
        assert torch.equal(ld.long(), lab[rows].long())
        assert torch.equal(oh, torch.nn.functional.one_hot(lab[rows].long(), 10).float())
        assert all(bool((z == 0).all()) for z in zs)
        assert int(ctr.item()) == 6 + call


@pytest.mark.parametrize("kw,what", [
    (dict(pad=5), "pad"),                        # pad >= min(H, W)
    (dict(H=40, W=40, src_d=4800, pad=16), "pad"),  # pad > 15
    (dict(src_d=74), "H\\*W\\*C"),                 # row length
    (dict(mean_n=4), "mean"),                    # statistics of the wrong length
    (dict(mean_n=3, inv_n=None), "mean"),        # one statistic without the other
    (dict(pad=-1), "pad"),
])
def test_augment_rows_bad_arguments_raise(kw, what):
    H, W, C = kw.get("H", 5), kw.get("W", 5), 3
    src = torch.zeros(10, kw.get("src_d", 75), dtype=torch.uint8)
    dst = torch.zeros(4, H, W, C)
    mean = torch.zeros(kw["mean_n"]) if "mean_n" in kw else None
    inv_n = kw.get("inv_n", kw.get("mean_n"))
    inv = torch.ones(inv_n) if inv_n is not None else None
    with pytest.raises(ValueError, match=what):
        ops.augment_rows(src, dst, H, W, C, pad=kw.get("pad", 0), mean=mean, inv_std=inv, idx=torch.zeros(4, dtype=torch.int32))
    assert bool((dst == 0).all())


# -------------------------------------------------------------- data layer
def test_channel_stats_against_numpy_float64():
    g = np.random.RandomState(3)
    x = g.randint(0, 256, size=(700, 32 * 32 * 3)).astype(np.uint8)
    x.reshape(-1, 3)[:, 1] //= 3  # channels with different statistics
    mean, inv_std = cifar.channel_stats(x)
    px = x.reshape(-1, 3).astype(np.float64) / 255.0
    assert mean.dtype == inv_std.dtype == np.float32 and mean.shape == inv_std.shape == (3,)
    # float32 results of a float64 computation: within one float32 ulp (2^-23 relative) of numpy's
    assert np.abs(mean / px.mean(0) - 1).max() <= 2.0 ** -23
    assert np.abs(inv_std * px.std(0) - 1).max() <= 2.0 ** -23
    assert mean[1] < 0.5 * mean[0]


def test_augment_record_and_eval():
    x = np.random.RandomState(4).randint(0, 256, size=(64, 3072)).astype(np.uint8)
    a = cifar.Augment.cifar(x)
    assert (a.H, a.W, a.C, a.pad, a.flip) == (32, 32, 3, 4, True)
    m, s = cifar.channel_stats(x)
    assert np.array_equal(a.mean, m) and np.array_equal(a.inv_std, s)
    e = a.eval()
    assert (e.H, e.W, e.C, e.pad, e.flip) == (32, 32, 3, 0, False)
    assert np.array_equal(e.mean, a.mean) and np.array_equal(e.inv_std, a.inv_std)
    assert (a.pad, a.flip) == (4, True)  # eval() returns a new record


# ------------------------------------------------------------ flag and CLI
def test_augment_flag_parses_and_defaults_to_none(capsys):
    assert flagmod.parse([]).augment == "none"
    assert flagmod.parse(["--augment=cifar"]).augment == "cifar"
    assert flagmod.parse(["--augment", "none"]).augment == "none"
    with pytest.raises(SystemExit):
        flagmod.parse(["--augment=imagenet"])
    assert "--augment" in capsys.readouterr().err


@pytest.mark.parametrize("model", ["cnn", "softmax"])
def test_augment_cifar_refuses_other_models(model, tmp_path):
    with pytest.raises(ValueError, match="--augment"):
        train.run(model, ["--mode=local", "--device=cpu", "--synthetic", "--augment=cifar", "--num_steps=1",
                          "--batch_size=4", "--save_model_secs=0", "--model_dir=" + str(tmp_path)],
                  log=lambda *_: None)


def test_feeder_cpu_applies_the_transforms():
    """train.Feeder on CPU with --augment cifar: batch k is the construction over the rows the epoch
    batcher handed out, drawn at counter value k with the data set's seed; evaluation statistics set."""
    B, seed = 4, 11
    (tr_x, tr_y), _ = cifar.synthetic_arrays(n_train=40, n_test=8)
    from dtfe.data.mnist import DataSet, DataSets

    data = DataSets(DataSet(tr_x, tr_y, True, seed), None, None, True)
    twin = DataSet(tr_x, tr_y, True, seed)  # the same seed hands out the same rows

    class Prog:
        batch_size = B
        model = ResNetModel(arch="resnet20")
        input_norm = None

    prog = Prog()
    feeder = train.Feeder(data, prog, torch.device("cpu"), augment="cifar")
    mean, inv_std = (torch.from_numpy(a) for a in cifar.channel_stats(tr_x))
    assert torch.equal(prog.input_norm[0], mean) and torch.equal(prog.input_norm[1], inv_std)
    for k in range(3):
        x, y = feeder.next()
        rows = torch.from_numpy(twin.next_batch_indices(B).astype(np.int64))
        exp = construct(torch.from_numpy(tr_x), rows, 32, 32, 3, 4, ops.augment_draws(seed, k, B, 4, True), mean, inv_std,
                        torch.float32)
        assert torch.equal(x.reshape(B, 32, 32, 3), exp), k
        assert torch.equal(y, torch.nn.functional.one_hot(torch.from_numpy(tr_y[rows.numpy()]), 10).float())
    with pytest.raises(ValueError, match="--augment"):
        Prog.model = ResNetModel(arch="resnet50")
        train.Feeder(data, Prog(), torch.device("cpu"), augment="cifar")


# ------------------------------------------------------------------- model
def eval_with_input_norm_matches_hand_standardised(device, B):
    """evaluate() with input_norm on uint8 images = the same program without it on images standardised
    here ((byte * float32(1/255) - mean) * inv_std in float32): same logits bit for bit, same accuracy."""
    torch.manual_seed(6)
    prog = ResNetModel(arch="resnet20").program(device, B, seed=2)
    g = torch.Generator().manual_seed(8)
    n = B + 3  # two chunks, the second padded by repeated rows
    u8 = torch.randint(0, 256, (n, 3072), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n, 1), generator=g)
    mean, inv_std = (torch.from_numpy(a) for a in cifar.channel_stats(u8.numpy()))
    hand = (u8.float().reshape(n, 32, 32, 3) * torch.tensor(float(np.float32(1.0 / 255.0))) - mean) * inv_std
    assert prog.input_norm is None
    acc_hand = prog.evaluate(hand.reshape(n, -1).to(device), y.to(device))
    logits_hand = prog.logits.clone()
    x_hand = prog.x.clone()
    prog.input_norm = (mean.to(device), inv_std.to(device))
    acc = prog.evaluate(u8.to(device), y.to(device))
    assert torch.equal(prog.x, x_hand)
    assert torch.equal(prog.logits, logits_hand) and acc == acc_hand
    assert bool(torch.isfinite(prog.logits).all()) and prog.logits.std().item() > 0
    # and the statistics matter: the unstandardised images give other logits
    prog.input_norm = None
    prog.evaluate((u8.float() / 255).to(device), y.to(device))
    assert not torch.equal(prog.logits, logits_hand)


def test_resnet_evaluate_with_input_norm_cpu():
    eval_with_input_norm_matches_hand_standardised("cpu", 4)


def test_load_batch_of_its_own_buffer_copies_nothing():
    prog = ResNetModel(arch="resnet20").program("cpu", 2, seed=0)
    prog.x.copy_(torch.rand(prog.x.shape))
    before = prog.x.clone()
    y = torch.tensor([[3], [7]])
    prog.load_batch((prog.x, y))
    assert torch.equal(prog.x, before) and torch.equal(prog.y.argmax(1), y.view(-1))
