"""Mixup, CutMix and label smoothing in ops.augment_rows (csrc/kernels/augment.h has the definition) on the
CPU: the host mirror of the draws (ops.mix_draws) against the definition in Python integers, the coverage
the GPU grid relies on, the CPU path of the op against a per-sample numpy construction on top of
test_augment_cpu's construct(), identities, refusals, the flags, the Feeder and the ResNet-20 loss.
Everything about batches compares with torch.equal: the definition is exact."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from dtfe import ops, train
from dtfe.data import cifar
from dtfe.data.mnist import DataSet, DataSets
from dtfe.models.resnet import ResNetModel
from dtfe.utils import flags as flagmod

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import N_ROWS, SENTINEL, construct, mirror_rows, source, stats  # noqa: E402
from test_rng_streams_cpu import BIG  # noqa: E402

bf = torch.bfloat16
u8, f32 = torch.uint8, torch.float32
NCLS = 10
M64 = 0xFFFFFFFFFFFFFFFF
STREAMS = [(seed, ctr) for seed in (3, 9) for ctr in (0, 5, BIG)]
one = np.float32(1.0)


def smooth(E, ncls=NCLS):
    """(on, off) of the issue: off = fl(E / ncls), on = fl(fl(1 - E) + off), float32 throughout."""
    e = np.float32(E)
    off = e / np.float32(ncls)
    return (one - e) + off, off


def expected(A, labels, d, mix, E, dst_dtype, ncls=NCLS):
    """The mixed batch and label rows from construct()'s float32 batch ``A`` (torch [B][H][W][C]), the slots'
    labels and the draws ``d``, sample by sample with np.float32 scalars: every product and sum is one
    float32 operation of numpy, rounded on its own."""
    A = A.numpy()
    assert A.dtype == np.float32
    B = len(A)
    on, off = smooth(E, ncls)
    out, y = A.copy(), np.empty((B, ncls), dtype=np.float32)
    t = [np.where(np.arange(ncls) == int(labels[b]), on, off).astype(np.float32) for b in range(B)]
    for b in range(B):
        p = int(d.partner[b])
        if mix == "none":
            y[b] = t[b]
            continue
        if mix == "mixup":
            w = np.float32(d.lam[b])
            out[b] = w * A[b] + (one - w) * A[p]
        else:
            y0, y1, x0, x1 = (int(v[b]) for v in d.box)
            out[b, y0:y1, x0:x1] = A[p, y0:y1, x0:x1]
            w = np.float32(d.lam_box[b])
        y[b] = w * t[b] + (one - w) * t[p]
    assert out.dtype == y.dtype == np.float32
    return torch.from_numpy(out).to(dst_dtype), torch.from_numpy(y)


def run_mix_case(dev, B, shape, pad, src_dtype, dst_dtype, with_stats, rows, seed, ctr, mix, E, extra_rows=2):
    """One launch into the first B rows of a sentinel-filled destination: ``rows`` is "idx" (explicit),
    "sampled" (with replacement) or "shuffle" (the epoch permutation).  Checks the batch, the label rows and
    the integer labels against expected(), and the sentinel rows behind the batch."""
    H, W, C = shape
    src, lab = source(H, W, C, src_dtype)
    mean, inv_std = stats(C) if with_stats else (None, None)
    if rows == "idx":
        r = (torch.arange(B) * 7 + 3) % N_ROWS
    elif rows == "sampled":
        r = mirror_rows(seed, ctr, B)
    else:
        r = torch.from_numpy(ops.shuffled_rows(seed, ctr, B, N_ROWS))
    full = torch.full((B + extra_rows, H, W, C), SENTINEL, dtype=dst_dtype, device=dev)
    ld = torch.full((B,), -1, dtype=torch.int32, device=dev)
    oh = torch.full((B, NCLS), SENTINEL, device=dev)
    counter = torch.tensor([ctr], dtype=torch.int64, device=dev)
    ops.augment_rows(src.to(dev), full[:B], H, W, C, pad=pad, flip=True,
                     mean=None if mean is None else mean.to(dev), inv_std=None if inv_std is None else inv_std.to(dev),
                     idx=r.int().to(dev) if rows == "idx" else None, labels_src=lab.to(dev), labels_dst=ld, seed=seed,
                     counter=counter, onehot=oh, shuffle=rows == "shuffle", mix=mix, label_smoothing=E)
    A = construct(src, r, H, W, C, pad, ops.augment_draws(seed, ctr, B, pad, True), mean, inv_std, f32)
    d = ops.mix_draws(seed, ctr, B, H, W)
    x, y = expected(A, lab[r], d, mix, E, dst_dtype)
    what = (B, shape, pad, src_dtype, dst_dtype, with_stats, rows, seed, ctr, mix, E)
    assert torch.equal(full[:B].cpu(), x), what
    assert bool((full[B:] == SENTINEL).all()), ("stored past row B", what)
    assert torch.equal(oh.cpu(), y), what
    assert torch.equal(ld.cpu().long(), lab[r].long()), what
    assert int(counter.item()) == ctr, ("advanced without a ticket", what)
    return d


def mix_covers(d, H, W, empty):
    """lam on both sides of 0.5; a non-empty box cut off at each of the four edges, one that touches none,
    and (small images) an empty one."""
    y0, y1, x0, x1 = d.box
    full = (y1 > y0) & (x1 > x0)
    edges = [(full & (x0 == 0)).any(), (full & (x1 == W)).any(), (full & (y0 == 0)).any(), (full & (y1 == H)).any()]
    inner = (full & (x0 > 0) & (x1 < W) & (y0 > 0) & (y1 < H)).any()
    return bool((d.lam < 0.5).any() and (d.lam > 0.5).any() and all(edges) and inner and ((~full).any() or not empty))


# ------------------------------------------------------------------ draws
def test_salts():
    assert (ops.MIX_LAM_SALT, ops.MIX_BOX_SALT, ops.MIX_ROT_SALT) == (0x4D1C5EEDB1E2D0A7, 0xB0C5CE27E4A1F00D,
                                                                      0x9A27E4F00D5EED13)
    assert "mix_draws" in ops.__all__


@pytest.mark.parametrize("H,W", [(32, 32), (5, 5), (6, 4)])
def test_mix_draws_equal_the_definition_in_python_integers(H, W):
    for B in (2, 5, 130):
        for seed, ctr in STREAMS:
            d = ops.mix_draws(seed, ctr, B, H, W)
            shift = 1 + int(ops.hash_u32(seed ^ ops.MIX_ROT_SALT, ctr)) % (B - 1)
            assert d.shift == shift and 1 <= shift <= B - 1
            assert sorted(d.partner.tolist()) == list(range(B)) and not (d.partner == np.arange(B)).any()
            inv_hw = one / np.float32(H * W)
            for b in range(B):
                i = (ctr * B + b) & M64
                assert d.partner[b] == (b + shift) % B
                k = int(ops.hash_u32(seed ^ ops.MIX_LAM_SALT, i)) >> 8
                assert d.k[b] == k and d.lam[b] == np.float32(k) * np.float32(2.0 ** -24) and 0 <= d.lam[b] < 1
                assert float(one - d.lam[b]) == 1.0 - k / 2.0 ** 24  # 1 - lam is exact in float32
                r24 = math.isqrt(((1 << 24) - k) << 24)
                rw, rh = (W * r24) >> 24, (H * r24) >> 24
                hb = int(ops.hash_u32(seed ^ ops.MIX_BOX_SALT, i))
                cx, cy = hb % W, (hb // W) % H
                box = (max(cy - rh // 2, 0), min(cy + rh // 2, H), max(cx - rw // 2, 0), min(cx + rw // 2, W))
                assert tuple(int(v[b]) for v in d.box) == box
                assert 0 <= box[0] <= box[1] <= H and 0 <= box[2] <= box[3] <= W
                area = (box[1] - box[0]) * (box[3] - box[2])
                assert d.lam_box[b] == np.float32(H * W - area) * inv_hw
                if area == 0:
                    assert d.lam_box[b] == 1.0
            assert d.lam.dtype == d.lam_box.dtype == np.float32
    # one stream over steps: slot b of step s is element s * B + b
    two, second = ops.mix_draws(7, 0, 260, H, W), ops.mix_draws(7, 1, 130, H, W)
    assert np.array_equal(two.k[130:], second.k) and all(np.array_equal(a[130:], b) for a, b in zip(two.box, second.box))


def test_box_scale_is_the_exact_integer_square_root():
    for k in (0, 1, 1 << 23, (1 << 24) - 1):
        v = ((1 << 24) - k) << 24
        r = ops.mix_r24(k)
        assert r == math.isqrt(v) and r * r <= v < (r + 1) * (r + 1)
    assert ops.mix_r24(0) == 1 << 24 and ops.mix_r24((1 << 24) - 1) == 1 << 12
    with pytest.raises(ValueError, match="B >= 2"):
        ops.mix_draws(3, 0, 1, 32, 32)


@pytest.mark.parametrize("H,W", [(32, 32), (8, 8), (5, 5), (4, 4), (6, 4)])
def test_mirror_draws_cover_every_case_at_b130(H, W):
    """What the GPU grid relies on, for every stream and image size it uses."""
    for seed, ctr in STREAMS:
        assert mix_covers(ops.mix_draws(seed, ctr, 130, H, W), H, W, empty=H < 32), (seed, ctr)


# ---------------------------------------------------------------- CPU path
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("shape,pad", [((32, 32, 3), 4), ((5, 5, 3), 1), ((6, 4, 1), 3)])
@pytest.mark.parametrize("mix", ["mixup", "cutmix"])
def test_augment_rows_cpu_equals_the_construction(B, shape, pad, mix):
    n = 0
    for E in (0.0, 0.1):
        for s in (u8, f32):
            for dd in (f32, bf):
                seed, ctr = STREAMS[n % 6]
                run_mix_case("cpu", B, shape, pad, s, dd, n % 2 == 0, ("idx", "sampled", "shuffle")[n % 3], seed, ctr, mix, E)
                n += 1
    assert n == 8


def test_defaults_are_the_plain_launch_bitwise():
    H, W, C, B = 5, 5, 3, 6
    src, lab = source(H, W, C, u8)
    mean, inv_std = stats(C)
    outs = []
    for kw in ({}, dict(mix="none", label_smoothing=0.0)):
        dst, oh = torch.empty(B, H, W, C), torch.full((B, NCLS), SENTINEL)
        ops.augment_rows(src, dst, H, W, C, pad=1, flip=True, mean=mean, inv_std=inv_std, labels_src=lab, seed=9,
                         counter=torch.tensor([5]), onehot=oh, **kw)
        outs.append((dst, oh))
    rows = mirror_rows(9, 5, B)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[1][0], construct(src, rows, H, W, C, 1, ops.augment_draws(9, 5, B, 1, True), mean, inv_std, f32))
    assert torch.equal(outs[1][1], torch.nn.functional.one_hot(lab[rows].long(), NCLS).float())


def test_smoothing_alone_changes_only_the_label_rows():
    for shape in ((32, 32, 3), (5, 5, 3)):
        run_mix_case("cpu", 6, shape, 1, u8, f32, True, "sampled", 3, 5, "none", 0.1)
    on, off = smooth(0.1)
    assert smooth(0.0) == (1.0, 0.0) and ops.smoothing_values(0.0, NCLS) == (1.0, 0.0)
    assert ops.smoothing_values(0.1, NCLS) == (on, off) and on.dtype == off.dtype == np.float32
    H, W, C, B = 5, 5, 3, 130
    src, lab = source(H, W, C, u8)
    oh = torch.empty(B, NCLS)
    ops.augment_rows(src, torch.empty(B, H, W, C), H, W, C, labels_src=lab, seed=3, onehot=oh, label_smoothing=0.1)
    assert set(oh.unique().tolist()) == {float(on), float(off)}
    # ten float32 terms near 0.1 and 0.9: the float64 sum of the stored values lies within 1 ulp of 1
    assert (oh.double().sum(1) - 1).abs().max().item() <= 2.0 ** -23
    # mixed rows: 2 * ncls terms, each product within 2^-25 of exact and each sum within 2^-24 (values <= 1)
    ops.augment_rows(src, torch.empty(B, H, W, C), H, W, C, labels_src=lab, seed=3, onehot=oh, mix="mixup")
    assert (oh.double().sum(1) - 1).abs().max().item() <= 2.0 ** -22
    assert bool((oh > 0).sum(1).max() == 2) and bool((oh > 0).sum(1).min() >= 1)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw,what", [
    (dict(mix="mixup", onehot=None), "onehot"),
    (dict(mix="cutmix", labels_src=None), "labels_src"),
    (dict(label_smoothing=0.1, onehot=None), "onehot"),
    (dict(label_smoothing=0.1, labels_src=None), "labels_src"),
    (dict(mix="mixup", B=1), "B >= 2"),
    (dict(label_smoothing=1.0), "label_smoothing"),
    (dict(label_smoothing=-0.1), "label_smoothing"),
    (dict(mix="blend"), "mix"),
])
def test_bad_mixing_arguments_raise(kw, what):
    kw = dict(kw)
    B = kw.pop("B", 4)
    src, lab = source(5, 5, 3, u8)
    args = dict(labels_src=lab, onehot=torch.zeros(B, NCLS))
    args.update(kw)
    dst = torch.zeros(B, 5, 5, 3)
    with pytest.raises(ValueError, match=what):
        ops.augment_rows(src, dst, 5, 5, 3, **args)
    assert bool((dst == 0).all())


def test_flags_parse_and_default_off(capsys):
    f = flagmod.parse([])
    assert f.mix == "none" and f.label_smoothing == 0.0
    f = flagmod.parse(["--mix=cutmix", "--label_smoothing", "0.1"])
    assert f.mix == "cutmix" and f.label_smoothing == 0.1
    assert flagmod.parse(["--mix", "mixup"]).mix == "mixup"
    with pytest.raises(SystemExit):
        flagmod.parse(["--mix=manifold"])
    assert "--mix" in capsys.readouterr().err


@pytest.mark.parametrize("model,extra,what", [
    ("resnet20", ["--mix=mixup"], "--augment cifar"),
    ("resnet20", ["--label_smoothing=0.1"], "--augment cifar"),
    ("resnet20", ["--augment=cifar", "--label_smoothing=1.5"], "label_smoothing"),
    ("cnn", ["--mix=cutmix"], "--augment cifar"),
    ("cnn", ["--augment=cifar", "--mix=cutmix"], "--augment"),
    ("softmax", ["--augment=cifar", "--label_smoothing=0.1"], "--augment"),
])
def test_flags_are_refused_without_the_cifar_recipe(model, extra, what, tmp_path):
    with pytest.raises(ValueError, match=what):
        train.run(model, ["--mode=local", "--device=cpu", "--synthetic", "--num_steps=1", "--batch_size=4",
                          "--save_model_secs=0", "--model_dir=" + str(tmp_path)] + extra, log=lambda *_: None)


def test_augment_eval_clears_both():
    x = np.random.RandomState(4).randint(0, 256, size=(64, 3072)).astype(np.uint8)
    a = cifar.Augment.cifar(x)
    assert (a.mix, a.label_smoothing) == ("none", 0.0)
    import dataclasses

    m = dataclasses.replace(a, mix="cutmix", label_smoothing=0.1)
    e = m.eval()
    assert (e.mix, e.label_smoothing, e.pad, e.flip) == ("none", 0.0, 0, False)
    assert (m.mix, m.label_smoothing) == ("cutmix", 0.1) and np.array_equal(e.mean, a.mean)


# ------------------------------------------------------------------ feeder
class _Prog:
    batch_size = 4
    model = ResNetModel(arch="resnet20")
    input_norm = None


def test_feeder_cpu_yields_the_mirror():
    B, seed = 4, 11
    (tr_x, tr_y), _ = cifar.synthetic_arrays(n_train=40, n_test=8)
    data = DataSets(DataSet(tr_x, tr_y, True, seed), None, None, True)
    twin = DataSet(tr_x, tr_y, True, seed)
    feeder = train.Feeder(data, _Prog(), torch.device("cpu"), augment="cifar", mix="mixup", label_smoothing=0.1)
    mean, inv_std = (torch.from_numpy(a) for a in cifar.channel_stats(tr_x))
    for k in range(3):
        x, y = feeder.next()
        rows = torch.from_numpy(twin.next_batch_indices(B).astype(np.int64))
        A = construct(torch.from_numpy(tr_x), rows, 32, 32, 3, 4, ops.augment_draws(seed, k, B, 4, True), mean, inv_std, f32)
        ex, ey = expected(A, tr_y[rows.numpy()], ops.mix_draws(seed, k, B, 32, 32), "mixup", 0.1, f32)
        assert torch.equal(x.reshape(B, 32, 32, 3), ex) and torch.equal(y, ey), k
    with pytest.raises(ValueError, match="--augment cifar"):
        train.Feeder(data, _Prog(), torch.device("cpu"), mix="mixup")


# ------------------------------------------------------------------- model
def soft_target_loss_matches(device, B, rel):
    """One ResNet-20 compute_grads on a mixed, smoothed batch written by augment_rows together with the
    zeroing of the step accumulators: the program's loss is the soft-target cross-entropy of its own
    logits and label rows (float64 here)."""
    torch.manual_seed(6)
    prog = ResNetModel(arch="resnet20").program(device, B, seed=2)
    (tr_x, tr_y), _ = cifar.synthetic_arrays(n_train=40, n_test=8)
    aug = cifar.Augment.cifar(tr_x)
    mean, inv_std = aug.stats_on(device)
    prog.loss.fill_(123.0)
    prog.correct.fill_(7)
    prog.P.grad.fill_(1.0)
    x = prog.x if prog.x.device.type == "cuda" else torch.empty(B, 32, 32, 3)
    ops.augment_rows(torch.from_numpy(tr_x).to(device), x, 32, 32, 3, pad=4, flip=True, mean=mean, inv_std=inv_std,
                     labels_src=torch.from_numpy(tr_y.astype(np.int32)).to(device), seed=5,
                     counter=torch.zeros(1, dtype=torch.int64, device=device),
                     done=torch.zeros(1, dtype=torch.int32, device=device), zero=prog.step_accumulators(), onehot=prog.y,
                     mix="mixup", label_smoothing=0.1)
    assert all(bool((t == 0).all()) for t in prog.step_accumulators())
    if x is not prog.x:
        prog.x.copy_(x.to(prog.x.dtype))
    y = prog.y.double().cpu()
    assert bool(((y > 0) & (y < 1)).all()) and (y.sum(1) - 1).abs().max().item() <= 2.0 ** -22
    loss = float(prog.compute_grads(zeroed=True)["loss"].item())
    ref = -(y * torch.log_softmax(prog.logits.double().cpu(), 1)).sum(1).mean().item()
    print("loss %.9g  soft-target cross-entropy of the logits %.9g  rel %.3g" % (loss, ref, abs(loss / ref - 1)))
    assert math.isfinite(loss) and abs(loss - ref) <= rel * abs(ref), (loss, ref)
    assert torch.equal(prog.y.double().cpu(), y)


def test_resnet20_loss_is_the_soft_target_cross_entropy_cpu():
    soft_target_loss_matches("cpu", 4, 1e-5)
