"""The host mirror of the kernels' counter-based RNG (ops.hash_u32 / ops.hash_uniform) and the CPU
reference paths built on it: statistics of the dropout masks the GPU tests compare the kernels with,
the CPU dropout of ops.gemm / ops.bias_act, and the fp32 CNN step with dropout on against autograd
with the mirror's mask."""
import numpy as np
import pytest
import torch

from dtfe import ops
from dtfe.models.mnist_cnn import FC, MnistCnnModel

from test_cnn_cpu import _batch, autograd_f32

BIG = 3_000_000_000  # a step counter above 2^31 (and 2^32 once multiplied by M*N)


def mirror_mask(seed, step, M, N, keep, ldc=None):
    """[M][N] bool, True = kept: the dropout mask of dense_epi at counter value ``step``."""
    ldc = N if ldc is None else ldc
    o = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ldc) + np.arange(N, dtype=np.uint64)[None, :])
    return ops.hash_uniform(seed, o + np.uint64(step * M * N)) < np.float32(keep)


def test_hash_u32_is_the_splitmix_mix():
    """hash_u32 against the same mix in Python integers (no numpy wraparound involved), at
    indices on both sides of 2^32 and 2^63; hash_uniform is its top 24 bits."""
    m64 = (1 << 64) - 1

    def ref(seed, idx):
        z = (seed * 0x9E3779B97F4A7C15 + idx * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & m64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return (z ^ (z >> 31)) & 0xFFFFFFFF

    idx = [0, 1, 2, 63, 64, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, BIG * 65536 + 17, 2**63 + 5, 2**64 - 1]
    for seed in (0, 1, 9, 7919 + 2, 9 ^ 0xA5A5A5A5, 2**63 + 3):
        got = ops.hash_u32(seed, np.array(idx, dtype=np.uint64))
        assert got.dtype == np.uint32
        assert [int(v) for v in got] == [ref(seed, i) for i in idx], seed
        u = ops.hash_uniform(seed, np.array(idx, dtype=np.uint64))
        assert u.dtype == np.float32
        assert [float(v) for v in u] == [(ref(seed, i) >> 8) / 16777216.0 for i in idx]
    assert int(ops.hash_u32(3, 5)) == ref(3, 5)  # scalars too


@pytest.mark.parametrize("shape", [(64, 1024), (256, 1024), (96, 200), (128, 128), (70, 200)])
@pytest.mark.parametrize("keep", [0.5, 0.75, 0.9])
def test_mirror_mask_statistics(shape, keep):
    """The masks are Bernoulli(keep): overall rate within 4 sigma, every row and column within 5 sigma
    of keep for its length, and the masks of consecutive steps agree like independent ones
    (keep^2 + (1 - keep)^2, 4 sigma) - a stream that ignored the step, or striped rows / columns, fails."""
    M, N = shape
    n = M * N
    sd = (keep * (1 - keep)) ** 0.5
    pa = keep * keep + (1 - keep) * (1 - keep)
    for step in (0, 1, 5, BIG):
        m = mirror_mask(9, step, M, N, keep)
        assert abs(m.mean() - keep) <= 4 * sd / n ** 0.5, (step, m.mean())
        assert np.abs(m.mean(0) - keep).max() <= 5 * sd / M ** 0.5, (step, "columns")
        assert np.abs(m.mean(1) - keep).max() <= 5 * sd / N ** 0.5, (step, "rows")
        agree = (m == mirror_mask(9, step + 1, M, N, keep)).mean()
        assert abs(agree - pa) <= 4 * (pa * (1 - pa) / n) ** 0.5, (step, agree)


# hash_uniform(9, U_EQ_IDX) == float32(0.9) exactly (24-bit value 15099494 / 2^24): the first such index
# of seed 9, found by scanning the mirror from 0 (about 4e7 indices; one in 2^24 qualifies)
U_EQ_IDX = 39598221


def test_gemm_cpu_dropout_compares_in_fp32():
    """keep = 0.9 is not an fp32 number: the kernel compares u < float(keep), so the element whose
    u equals float32(0.9) is DROPPED (a comparison with the double 0.9 would keep it), and kept
    values are scaled by the fp32 reciprocal 1.f / keep."""
    k32 = np.float32(0.9)
    assert ops.hash_uniform(9, U_EQ_IDX) == k32 and float(k32) < 0.9
    M, N = 2, 3
    step, o = divmod(U_EQ_IDX, M * N)
    ctr = torch.tensor([step], dtype=torch.int64)
    A = torch.rand(M, 4) + 0.5
    B = torch.rand(N, 4) + 0.5
    out = torch.full((M, N), -1.0)
    ops.gemm(A, B, out, M=M, N=N, K=4, keep=0.9, seed=9, counter=ctr)
    kept = mirror_mask(9, step, M, N, 0.9)
    assert not kept.reshape(-1)[o]
    assert out.reshape(-1)[o].item() == 0.0
    ref = (A @ B.t()) * torch.tensor(float(np.float32(1.0) / k32))
    assert torch.equal(out, torch.where(torch.from_numpy(kept), ref, torch.zeros(M, N)))
    assert int(ctr.item()) == step  # the GEMM reads the counter, it never advances it


@pytest.mark.parametrize("ldc", [50, 56])
def test_gemm_cpu_dropout_index_uses_ldc(ldc):
    """Element (row, col) has stream index step * M*N + row * ldc + col (dense_epi)."""
    M, N, K = 37, 50, 8
    g = torch.Generator().manual_seed(1)
    A = torch.rand(M, K, generator=g) + 0.5
    B = torch.rand(N, K, generator=g) + 0.5
    for step in (None, 0, 5, BIG):
        out = torch.full((M, ldc), -1.0)
        ctr = None if step is None else torch.tensor([step], dtype=torch.int64)
        ops.gemm(A, B, out, M=M, N=N, K=K, ldc=ldc, keep=0.75, seed=4, counter=ctr)
        kept = torch.from_numpy(mirror_mask(4, step or 0, M, N, 0.75, ldc=ldc))
        ref = (A @ B.t()) * torch.tensor(float(np.float32(1.0) / np.float32(0.75)))
        assert torch.equal(out[:, :N], torch.where(kept, ref, torch.zeros(M, N))), step
        assert bool((out[:, N:] == -1.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_act_cpu_applies_dropout(dtype):
    """ops.bias_act's CPU path with keep < 1 = an explicit mask computation, index step * M*N + i."""
    M, N = 37, 50
    g = torch.Generator().manual_seed(2)
    x = torch.rand(M, N, generator=g) + 0.5
    bias = torch.rand(N, generator=g)
    for step in (None, 0, 1, BIG):
        ctr = None if step is None else torch.tensor([step], dtype=torch.int64)
        out = torch.empty(M, N, dtype=dtype)
        ops.bias_act(x, bias, out, ops.ACT_RELU, keep=0.75, seed=6, counter=ctr)
        u = ops.hash_uniform(6, np.arange(M * N, dtype=np.uint64) + np.uint64((step or 0) * M * N))
        kept = torch.from_numpy(u < np.float32(0.75)).reshape(M, N)
        ref = torch.relu(x + bias) * torch.tensor(float(np.float32(1.0) / np.float32(0.75)))
        assert torch.equal(out, torch.where(kept, ref, torch.zeros(M, N)).to(dtype)), step
    assert bool((out == 0).any()) and bool((out != 0).any())
    plain = torch.empty(M, N, dtype=dtype)
    ops.bias_act(x, bias, plain, ops.ACT_RELU)
    assert torch.equal(plain, torch.relu(x + bias).to(dtype))


def test_fp32_cnn_step_with_dropout_matches_autograd():
    """CnnProgram (fp32, CPU reference ops) at keep 0.75: the k-th loaded batch drops where the mirror
    drops at counter value k; loss and all eight gradients equal autograd with that mask inserted
    after fc1's ReLU (test_fp32_cnn_step_matches_autograd's tolerances).  Negative control: the mask
    of the neighbouring counter value misses fc1's weight gradient by more than 10x the tolerance."""
    B, keep = 16, 0.75
    m = MnistCnnModel()
    m.set_dtype("fp32")
    prog = m.program(torch.device("cpu"), B, seed=3)
    core = prog.core
    assert core.keep == keep
    for k in (1, 2):
        prog.load_batch(_batch(B, seed=k))
        assert int(core.data_ctr.item()) == k
        met = prog.compute_grads()
        assert int(core.data_ctr.item()) == k
        kept = torch.from_numpy(mirror_mask(core.seed + 2, k, B, FC, keep))
        pre = []
        loss_ref, grads, _ = autograd_f32(core, mask=kept, keep=keep, pre_out=pre)
        pos = pre[0] > 1e-2 * pre[0].max()
        assert pos.float().mean().item() >= 0.25
        assert bool((core.h[~kept] == 0).all()) and bool((core.h[kept & pos] != 0).all())
        assert abs(met["loss"].item() - loss_ref) <= 1e-5 * abs(loss_ref)
        for name, g in grads.items():
            err = ((core.gw[name] - g).norm() / (g.norm() + 1e-12)).item()
            assert err < 1e-4, (k, name, err)
    wrong = torch.from_numpy(mirror_mask(core.seed + 2, 3, B, FC, keep))
    _, grads, _ = autograd_f32(core, mask=wrong, keep=keep)
    err = ((core.gw["wd1"] - grads["wd1"]).norm() / (grads["wd1"].norm() + 1e-12)).item()
    assert err > 10 * 1e-4, err
