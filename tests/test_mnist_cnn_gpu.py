"""End-to-end numerics of the fused MNIST-CNN step program vs torch autograd (fp32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dtfe import ops

pytestmark = pytest.mark.gpu


class _Bf16Point(torch.autograd.Function):
    """Round to bf16 in forward AND backward: mirrors where the kernels store bf16."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


q = _Bf16Point.apply


def _reference_grads(trainer, mask=None, keep=1.0, pre_out=None):
    """``mask`` ([B][FC] bool, the host mirror's dropout mask): h = relu(pre) * mask * float32(1 / keep),
    rounded once as the fc1 epilogue does; ``pre_out`` (list): receives fc1's pre-activation."""
    P, n = trainer.P, trainer.names
    x = trainer.x.float().permute(0, 3, 1, 2).cpu()            # what the kernels consumed
    y = trainer.labels.long().cpu()

    def w(k):
        return P.view(n[k]).detach().cpu().to(torch.bfloat16).float().requires_grad_(True)

    def b(k):
        return P.view(n[k]).detach().cpu().float().requires_grad_(True)

    wc1, wc2, wd1, wo = w("wc1"), w("wc2"), w("wd1"), w("out")
    bc1, bc2, bd1, bo = b("bc1"), b("bc2"), b("bd1"), b("bout")
    # the kernels pool the fp32 accumulators and round the pooled value (argmax on exact values)
    z = F.conv2d(x, wc1.permute(0, 3, 1, 2), bc1, padding=2)
    z = q(F.max_pool2d(F.relu(z), 2))
    z = F.conv2d(z, wc2.permute(0, 3, 1, 2), bc2, padding=2)
    z = q(F.max_pool2d(F.relu(z), 2))
    z = z.permute(0, 2, 3, 1).reshape(x.shape[0], -1)           # NHWC flatten, as the kernels
    pre = z @ wd1.t() + bd1
    if pre_out is not None:
        pre_out.append(pre.detach())
    if mask is None:
        h = F.relu(q(pre))
    else:
        h = q(F.relu(pre) * mask.float() * float(np.float32(1.0) / np.float32(keep)))
    logits = h @ wo.t() + bo
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return loss.item(), {"wc1": wc1.grad, "wc2": wc2.grad, "wd1": wd1.grad, "out": wo.grad,
                         "bc1": bc1.grad, "bc2": bc2.grad, "bd1": bd1.grad, "bout": bo.grad}


def test_cnn_step_matches_autograd():
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    torch.manual_seed(0)
    tr = MnistCnnTrainer(64, "cuda", keep_prob=1.0, seed=3)
    tr.forward_backward()
    torch.cuda.synchronize()
    loss_ref, grads = _reference_grads(tr)
    loss = tr.loss_sum.item() / tr.B
    assert abs(loss - loss_ref) < 2e-2 * max(1.0, abs(loss_ref))
    errs = {}
    for k, gref in grads.items():
        got = tr.gw[k].detach().cpu()
        errs[k] = ((got - gref).norm() / (gref.norm() + 1e-12)).item()
    assert all(e < 3e-2 for e in errs.values()), sorted(errs.items(), key=lambda kv: -kv[1])


def test_cnn_trains_and_graph_replays():
    from dtfe.models.mnist_cnn import MnistCnnTrainer, SyntheticMnist
    from dtfe.utils.graphs import StepGraph

    # a learnable synthetic task: label = brightest of 10 pixel bands
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 64, (4096, 784), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 10, (4096,), generator=g, dtype=torch.int32)
    for i in range(4096):
        band = int(lab[i])
        imgs[i, band * 78:(band + 1) * 78] = 255
    data = SyntheticMnist(0, "cuda", images=imgs, labels=lab)
    tr = MnistCnnTrainer(128, "cuda", data=data, lr=1e-3)
    run = StepGraph(tr.step, warmup=2)
    losses = []
    for _ in range(60):
        run()
        losses.append(tr.loss_sum.item() / tr.B)
    assert run.graph is not None, run.capture_error
    assert losses[-1] < 0.5 * losses[0]
    assert int(tr.global_step.item()) == 60


def test_cnn_repeated_step_grads_do_not_accumulate():
    """Only the atomically-accumulated grads are cleared per step (fused into the batch gather);
    every other gradient must be fully overwritten: the same batch twice -> the same grads,
    and the result matches autograd after a previous step left garbage behind."""
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    tr = MnistCnnTrainer(64, "cuda", keep_prob=1.0, seed=5)
    tr.P.grad.fill_(7.0)            # stale values everywhere
    tr.loss_sum.fill_(3.0)
    ctr0 = int(tr.data_ctr.item())
    tr.forward_backward()
    g1 = tr.P.grad.clone()
    l1 = tr.loss_sum.clone()
    tr.data_ctr.fill_(ctr0)         # same batch again
    tr.forward_backward()
    torch.cuda.synchronize()
    assert torch.allclose(tr.P.grad, g1, rtol=1e-4, atol=1e-6)
    assert torch.allclose(tr.loss_sum, l1, rtol=1e-5)
    loss_ref, grads = _reference_grads(tr)
    assert abs(tr.loss_sum.item() / tr.B - loss_ref) < 2e-2 * max(1.0, abs(loss_ref))
    for k, gref in grads.items():
        got = tr.gw[k].detach().cpu()
        assert ((got - gref).norm() / (gref.norm() + 1e-12)).item() < 3e-2, k


def test_cnn_fused_sampling_conv1_matches_separate_gather():
    """B >= 256: batch sampling + accumulator clearing fused into conv1's forward launch must
    give the same batch, labels, activations and gradients as gather kernel + conv1."""
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    res = {}
    for fused in ("1", "0"):
        tr = MnistCnnTrainer(256, "cuda", keep_prob=1.0, seed=7)
        tr.fused_gather = fused == "1"
        tr.P.grad.fill_(5.0)
        for _ in range(2):            # second step: counter advanced once, stale accumulators cleared
            tr.forward_backward()
        torch.cuda.synchronize()
        res[fused] = dict(x=tr.x.clone(), lab=tr.labels.clone(), p1=tr.p1.clone(), g=tr.P.grad.clone(),
                          ctr=int(tr.data_ctr.item()), loss=tr.loss_sum.clone())
    a, b = res["1"], res["0"]
    assert a["ctr"] == b["ctr"] == 2
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["lab"], b["lab"]) and torch.equal(a["p1"], b["p1"])
    assert torch.allclose(a["g"], b["g"], rtol=1e-4, atol=1e-6)
    assert abs(a["loss"].item() - b["loss"].item()) <= 1e-5 * abs(b["loss"].item())


def _reference_grads_on(trainer, device):
    """_reference_grads with the fp32 oracle on ``device`` (the bench-sized batches)."""
    P, n = trainer.P, trainer.names
    x = trainer.x.float().permute(0, 3, 1, 2).to(device)
    y = trainer.labels.long().to(device)

    def w(k):
        return P.view(n[k]).detach().to(device).to(torch.bfloat16).float().requires_grad_(True)

    def b(k):
        return P.view(n[k]).detach().to(device).float().requires_grad_(True)

    wc1, wc2, wd1, wo = w("wc1"), w("wc2"), w("wd1"), w("out")
    bc1, bc2, bd1, bo = b("bc1"), b("bc2"), b("bd1"), b("bout")
    with torch.backends.cudnn.flags(enabled=True, allow_tf32=False):
        z = F.conv2d(x, wc1.permute(0, 3, 1, 2), bc1, padding=2)
        z = q(F.max_pool2d(F.relu(z), 2))
        z = F.conv2d(z, wc2.permute(0, 3, 1, 2), bc2, padding=2)
        z = q(F.max_pool2d(F.relu(z), 2))
        z = z.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        h = F.relu(q(z @ wd1.t() + bd1))
        logits = h @ wo.t() + bo
        loss = F.cross_entropy(logits, y)
        loss.backward()
    return loss.item(), {"wc1": wc1.grad, "wc2": wc2.grad, "wd1": wd1.grad, "out": wo.grad,
                         "bc1": bc1.grad, "bc2": bc2.grad, "bd1": bd1.grad, "bout": bo.grad}


@pytest.mark.parametrize("B", [512, 1024])
def test_cnn_bench_shaped_step_matches_autograd(B):
    """The headline configuration itself (bench.py: B=1024 per GPU, fused gather+conv1 launch,
    split-K head wgrad with splits=8, conv2 blocks=128 on the side branch), dropout off, against
    fp32 autograd of the same bf16-rounded network."""
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    tr = MnistCnnTrainer(B, "cuda", keep_prob=1.0, seed=11)
    assert tr.fused_gather and tr.par
    tr.P.grad.fill_(3.0)               # stale values: every gradient must be overwritten / cleared
    tr.forward_backward()
    torch.cuda.synchronize()
    loss_ref, grads = _reference_grads_on(tr, "cuda")
    loss = tr.loss_sum.item() / tr.B
    assert abs(loss - loss_ref) < 2e-2 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    errs = {k: ((tr.gw[k].detach().float() - g).norm() / (g.norm() + 1e-12)).item() for k, g in grads.items()}
    assert all(e < 3e-2 for e in errs.values()), sorted(errs.items(), key=lambda kv: -kv[1])


def test_cnn_adam_step_matches_torch_adam_tf1_form():
    """One fused apply_gradients launch over all 3.27 M parameters (master, Adam slots, bf16 and
    transposed bf16 copies) against torch.optim.Adam on the same gradients.  TF1 Adam
    (lr_t = lr*sqrt(1-b2^t)/(1-b1^t), v -= lr_t*m/(sqrt(v)+eps)) is torch's Adam with
    eps_torch = eps / sqrt(1 - b2^t)."""
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    tr = MnistCnnTrainer(1024, "cuda", keep_prob=0.75, seed=13)
    tr.forward_backward()
    torch.cuda.synchronize()
    p0 = tr.P.master.detach().clone()
    g = tr.P.grad.detach().clone()
    tr.opt.step(gscale=1.0)
    torch.cuda.synchronize()
    ref = p0.clone().requires_grad_(True)
    ref.grad = g.clone()
    b1, b2, eps = 0.9, 0.999, 1e-8
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(b1, b2), eps=eps / (1 - b2) ** 0.5)
    opt.step()
    got = tr.P.master.detach()
    mask = g != 0   # padding between variables stays untouched
    err = (got - ref.detach())[mask].abs().max().item()
    assert err < 2e-6, err
    assert torch.equal(got[~mask], p0[~mask])
    # beta powers and global step advanced once
    assert torch.allclose(tr.opt.beta_pow.cpu(), torch.tensor([b1 * b1, b2 * b2]))
    assert int(tr.global_step.item()) == 1
    # bf16 working copies written by the same launch
    P, n = tr.P, tr.names
    for k in ("wc1", "wc2", "wd1", "out"):
        assert torch.equal(P.w16[n[k]], P.view(n[k]).to(torch.bfloat16)), k
    R, T, C = P.spec(n["wc2"]).transpose
    wt = P.view(n["wc2"]).reshape(R, T, C).permute(2, 1, 0).reshape(-1).to(torch.bfloat16)
    assert torch.equal(P.wt16[n["wc2"]], wt)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [256, 1024])
def test_cnn_training_is_bitwise_reproducible(B):
    """Two trainers with the same seed follow the same trajectory bit for bit: every reduction of
    the step (split-K combines, conv weight-gradient partial sums) runs in a fixed order, no
    float atomics - the property the data-parallel replicas_identical check builds on."""
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    outs = []
    for _ in range(2):
        tr = MnistCnnTrainer(B, "cuda", seed=5)
        for _ in range(5):
            tr.step()
        torch.cuda.synchronize()
        outs.append(tr.P.master.clone())
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


def test_cnn_evaluate_matches_argmax_agreement():
    """CnnProgram.evaluate (the Test-Accuracy line) = argmax agreement of the no-dropout forward
    with fp32 autograd's logits on a fixed batch, including a padded last chunk."""
    from dtfe.models.mnist_cnn import MnistCnnModel

    model = MnistCnnModel()
    prog = model.program(torch.device("cuda"), 64, seed=2)
    g = torch.Generator().manual_seed(1)
    n = 100
    imgs = torch.rand(n, 784, generator=g).cuda()
    lab = torch.nn.functional.one_hot(torch.randint(0, 10, (n,), generator=g), 10).float().cuda()
    acc = prog.evaluate(imgs, lab)
    c = prog.core
    assert c.loss_sum.item() == 0.0 and int(c.correct.item()) == 0
    hits = 0
    for lo in range(0, n, 64):
        m = min(64, n - lo)
        idx = torch.arange(lo, lo + 64).clamp_max(n - 1)
        prog.load_batch((imgs[idx.cuda()], lab[idx.cuda()]))
        c.forward(keep=1.0, logits=c.logits)
        torch.cuda.synchronize()
        _, logits_ref = _reference_forward(c)
        hits += int((logits_ref[:m].argmax(1).cuda() == lab[lo:lo + m].argmax(1)).sum())
    # the bf16 forward can flip a near-tie: allow one row of slack in 100
    assert abs(acc * n - hits) <= 1, (acc, hits / n)


def _reference_forward(trainer):
    P, n = trainer.P, trainer.names
    x = trainer.x.float().permute(0, 3, 1, 2).cpu()

    def w(k):
        return P.view(n[k]).detach().cpu().to(torch.bfloat16).float()

    def b(k):
        return P.view(n[k]).detach().cpu().float()

    z = F.conv2d(x, w("wc1").permute(0, 3, 1, 2), b("bc1"), padding=2)
    z = q(F.max_pool2d(F.relu(z), 2))
    z = F.conv2d(z, w("wc2").permute(0, 3, 1, 2), b("bc2"), padding=2)
    z = q(F.max_pool2d(F.relu(z), 2))
    z = z.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    h = q(F.relu(z @ w("wd1").t() + b("bd1")))
    return h, h @ w("out").t() + b("bout")


def test_cnn_fp32_step_matches_fp32_autograd():
    """--dtype fp32: the exact-fp32 MFMA step (conv_f32.hip convs, fp32 dense GEMMs, softmax-xent)
    against fp32 autograd of the same network on the CPU, dropout off: <= 1e-4 relative."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cnn_cpu import _batch, autograd_f32
    from dtfe.models.mnist_cnn import MnistCnnModel

    m = MnistCnnModel()
    m.set_dtype("fp32")
    prog = m.program(torch.device("cuda"), 128, seed=3)
    prog.core.keep = 1.0
    x, y = _batch(128, seed=2)
    prog.load_batch((x.cuda(), y.cuda()))
    prog.P.grad.fill_(9.0)             # stale values: stored gradients overwritten, accumulated ones cleared
    met = prog.compute_grads()
    torch.cuda.synchronize()
    core = prog.core
    cpu = type("C", (), {})()
    cpu.P = type("P", (), {"view": staticmethod(lambda k: core.P.view(k).cpu())})()
    cpu.names, cpu.x, cpu.labels = core.names, core.x.cpu(), core.labels.cpu()
    loss_ref, grads, _ = autograd_f32(cpu)
    assert abs(met["loss"].item() - loss_ref) <= 1e-5 * abs(loss_ref), (met["loss"].item(), loss_ref)
    errs = {k: ((core.gw[k].cpu() - g).norm() / (g.norm() + 1e-12)).item() for k, g in grads.items()}
    assert all(e <= 1e-4 for e in errs.values()), sorted(errs.items(), key=lambda kv: -kv[1])


def test_cnn_fp32_local_run_trains(capsys, tmp_path):
    """train.run with --dtype fp32 on the GPU (local mode, hipGraph-captured step): loss lines and
    the Test-Accuracy line print, the global step advances."""
    from dtfe import train

    rc = train.run("cnn", ["--mode=local", "--device=cuda", "--synthetic", "--num_steps=4", "--dtype=fp32",
                           "--batch_size=64", "--save_model_secs=0", "--model_dir=" + str(tmp_path / "ck")])
    out = capsys.readouterr().out
    assert rc == 0
    assert "Global step 4 Local step 3" in out and "Test-Accuracy: " in out, out[-2000:]


# ---------------------------------------------------------------------------
# dropout on (keep 0.75, the headline setting): sampled rows, dropout mask and gradients of whole
# steps against the host mirror of the device RNG (ops.hash_u32 / ops.hash_uniform) - the contract
# written in MnistCnnTrainer.forward's docstring
N_IMAGES = 5000


def _mirror_mask(seed, step, B, keep):
    """[B][1024] bool (True = kept): fc1's dropout mask at counter value ``step``."""
    n = B * 1024
    u = ops.hash_uniform(seed, np.uint64(step * n) + np.arange(n, dtype=np.uint64))
    return torch.from_numpy(u < np.float32(keep)).reshape(B, 1024)


def _mirror_rows(seed, step, B):
    h = ops.hash_u32(seed, np.uint64(step * B) + np.arange(B, dtype=np.uint64))
    return torch.from_numpy((h % np.uint32(N_IMAGES)).astype(np.int64))


def _id_dataset():
    """5000 random images whose pixels 0 and 1 carry the row id in base 128 (exact after the / 255
    and bf16 round trip of the gather), labels id % 10."""
    from dtfe.models.mnist_cnn import SyntheticMnist

    g = torch.Generator().manual_seed(21)
    imgs = torch.randint(0, 256, (N_IMAGES, 784), generator=g, dtype=torch.uint8)
    ids = torch.arange(N_IMAGES)
    imgs[:, 0] = (ids // 128).to(torch.uint8)
    imgs[:, 1] = (ids % 128).to(torch.uint8)
    return SyntheticMnist(0, "cuda", images=imgs, labels=(ids % 10).to(torch.int32))


def _sampled_ids(x):
    b = torch.round(x.reshape(x.shape[0], -1)[:, :2].float().cpu() * 255).long()
    return b[:, 0] * 128 + b[:, 1]


def _f32_reference(core, mask=None, keep=1.0, pre_out=None):
    """test_cnn_cpu.autograd_f32 on a CPU copy of a GPU fp32 trainer's parameters and batch."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cnn_cpu import autograd_f32

    cpu = type("C", (), {})()
    cpu.P = type("P", (), {"view": staticmethod(lambda k: core.P.view(k).cpu())})()
    cpu.names, cpu.x, cpu.labels = core.names, core.x.cpu(), core.labels.cpu()
    loss, grads, _ = autograd_f32(cpu, mask=mask, keep=keep, pre_out=pre_out)
    return loss, grads


def _check_mask_on_h(h, kept, pre):
    """h == 0 wherever the mirror drops; h != 0 wherever it keeps and the reference pre-activation
    is clearly positive (> 1e-2 of its maximum) - a class that must hold >= 1/4 of the elements."""
    pos = pre > 1e-2 * pre.max()
    assert pos.float().mean().item() >= 0.25
    h = h.float().cpu()
    assert bool((h[~kept] == 0).all()), "kept %d elements the mirror drops" % int((h[~kept] != 0).sum())
    assert bool((h[kept & pos] != 0).all()), "dropped %d elements the mirror keeps" % int((h[kept & pos] == 0).sum())


def _grad_errs(tr, grads):
    return {k: ((tr.gw[k].detach().float().cpu() - g).norm() / (g.norm() + 1e-12)).item() for k, g in grads.items()}


@pytest.mark.parametrize("kind,B", [("bf16", 64), ("bf16", 256), ("fp32", 64)])
def test_cnn_dropout_step_matches_mirror_and_autograd(kind, B):
    """Three training steps at keep 0.75 (B = 64: separate gather; B = 256: sampling fused into conv1;
    fp32 trainer): at step s the sampled rows and the dropout mask are the mirror's at counter value s,
    the counter advances once per step, loss and all eight gradients equal autograd with the mirror's
    mask after fc1's ReLU (the dropout-off tests' tolerances).  Negative control: the mask of the
    neighbouring counter value misses fc1's weight gradient by more than 10x the tolerance."""
    from dtfe.models.mnist_cnn import MnistCnnF32Trainer, MnistCnnTrainer

    keep = 0.75
    cls, ref, ltol, gtol = ((MnistCnnTrainer, _reference_grads, 2e-2, 3e-2) if kind == "bf16" else
                            (MnistCnnF32Trainer, _f32_reference, 1e-5, 1e-4))
    tr = cls(B, "cuda", keep_prob=keep, seed=3, data=_id_dataset())
    if kind == "bf16":
        assert tr.fused_gather and tr.par
    for s in range(3):
        assert int(tr.data_ctr.item()) == s
        tr.P.grad.fill_(3.0)
        tr.forward_backward()
        torch.cuda.synchronize()
        assert int(tr.data_ctr.item()) == s + 1, "the counter advances once per training step"
        rows = _mirror_rows(tr.seed + 1, s, B)
        assert torch.equal(_sampled_ids(tr.x), rows), s
        assert torch.equal(tr.labels.cpu().long(), rows % 10), s
        kept = _mirror_mask(tr.seed + 2, s, B, keep)
        pre = []
        loss_ref, grads = ref(tr, mask=kept, keep=keep, pre_out=pre)
        _check_mask_on_h(tr.h, kept, pre[0])
        loss = tr.loss_sum.item() / B
        assert abs(loss - loss_ref) <= ltol * (max(1.0, abs(loss_ref)) if kind == "bf16" else abs(loss_ref)), \
            (s, loss, loss_ref)
        errs = _grad_errs(tr, grads)
        assert all(e < gtol for e in errs.values()), (s, sorted(errs.items(), key=lambda kv: -kv[1]))
    for wrong in (1, 3):   # the last step ran at counter value 2
        _, grads = ref(tr, mask=_mirror_mask(tr.seed + 2, wrong, B, keep), keep=keep)
        err = _grad_errs(tr, grads)["wd1"]
        assert err > 10 * gtol, (wrong, err)


def test_cnn_fused_sampling_matches_separate_gather_with_dropout():
    """test_cnn_fused_sampling_conv1_matches_separate_gather at keep 0.75: the separate-gather path is
    the fused launch's oracle with dropout on too - same batch, same dropout mask (h bitwise equal),
    same gradients, and the same counter value after each step."""
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    res = {}
    for fused in ("1", "0"):
        tr = MnistCnnTrainer(256, "cuda", keep_prob=0.75, seed=7)
        tr.fused_gather = fused == "1"
        tr.P.grad.fill_(5.0)
        for _ in range(2):
            tr.forward_backward()
        torch.cuda.synchronize()
        res[fused] = dict(x=tr.x.clone(), lab=tr.labels.clone(), p1=tr.p1.clone(), h=tr.h.clone(),
                          g=tr.P.grad.clone(), ctr=int(tr.data_ctr.item()), loss=tr.loss_sum.clone())
    a, b = res["1"], res["0"]
    assert a["ctr"] == b["ctr"] == 2
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["lab"], b["lab"]) and torch.equal(a["p1"], b["p1"])
    assert torch.equal(a["h"], b["h"])
    assert bool((a["h"] == 0).float().mean().item() > 0.25)   # dropout is on
    assert torch.allclose(a["g"], b["g"], rtol=1e-4, atol=1e-6)
    assert abs(a["loss"].item() - b["loss"].item()) <= 1e-5 * abs(b["loss"].item())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_cnn_program_dropout_stream_and_evaluate(dtype):
    """CnnProgram (batches from the caller): the k-th loaded batch (k = 1, 2, ...) has the mirror's mask
    at counter value k, and only load_batch advances the counter; evaluate() leaves the counter
    where it was, runs without dropout, and the next training step's mask is the one it has anyway."""
    from dtfe.models.mnist_cnn import MnistCnnModel

    B, keep = 64, 0.75
    m = MnistCnnModel()
    m.set_dtype(dtype)
    prog = m.program(torch.device("cuda"), B, seed=2)
    core = prog.core
    assert core.keep == keep
    ref = _reference_grads if dtype == "bf16" else _f32_reference
    g = torch.Generator().manual_seed(8)

    def batch(n):
        x = torch.rand(n, 784, generator=g)
        y = F.one_hot(torch.randint(0, 10, (n,), generator=g), 10).float()
        return x.cuda(), y.cuda()

    def train_step(k):
        prog.load_batch(batch(B))
        assert int(core.data_ctr.item()) == k
        prog.compute_grads()
        torch.cuda.synchronize()
        assert int(core.data_ctr.item()) == k
        kept = _mirror_mask(core.seed + 2, k, B, keep)
        pre = []
        ref(core, mask=kept, keep=keep, pre_out=pre)
        _check_mask_on_h(core.h, kept, pre[0])

    train_step(1)
    train_step(2)
    prog.evaluate(*batch(100))
    torch.cuda.synchronize()
    assert int(core.data_ctr.item()) == 2
    pre = []
    ref(core, pre_out=pre)                      # core.x: the last evaluation chunk; keep = 1.0 there
    _check_mask_on_h(core.h, torch.ones(B, 1024, dtype=torch.bool), pre[0])
    train_step(3)
