"""Every device user of the counter-based hash RNG (csrc/kernels/common.h) against its host mirror
(ops.hash_u32 / ops.hash_uniform): the dropout mask of each GEMM epilogue engine and of bias_act,
on-device batch sampling, and the GAN's noise.  Expectations come from the mirror and a float64
computation of the same operation, never from another launch of the kernel under test.

Dropout masks are compared EXACTLY over all M*N elements: operands are drawn from U[0.5, 1.5], so
every pre-dropout value is >= 0.25 * K and an output is 0 exactly where the element was dropped."""
import os
import sys

import numpy as np
import pytest
import torch

from dtfe import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rng_streams_cpu import BIG, U_EQ_IDX, mirror_mask  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf = torch.bfloat16
PAD = -7.0  # fill of the output buffer: columns N..ldc-1 must keep it
TOL = {torch.float32: 1e-5, bf: 1e-2}  # of max|ref|, as the GEMM tests of these engines
_OPERANDS = {}


def _operands(M, N, K, dtype):
    """(A [M][K], B [N][K] on the GPU in ``dtype``, float64 A.B^T on the CPU), values in [0.5, 1.5]."""
    key = (M, N, K, dtype)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
        A = (torch.rand(M, K, generator=g) + 0.5).to(dtype)
        B = (torch.rand(N, K, generator=g) + 0.5).to(dtype)
        ref = A.double() @ B.double().t()
        assert ref.min().item() >= 0.25 * K
        _OPERANDS[key] = (A.to(DEV), B.to(DEV), ref)
    return _OPERANDS[key]


def _expect(ref, kept, keep):
    inv = float(np.float32(1.0) / np.float32(keep))
    return torch.where(torch.from_numpy(kept), ref * inv, torch.zeros_like(ref))


def _check(out, N, ref, kept, keep, dropped_value=0.0, shift=0.0):
    """Exact mask over all elements, dropped elements exactly ``dropped_value``, kept values within
    the engine's tolerance of ref * float32(1 / keep) (+ shift), padding columns untouched."""
    got = out[:, :N].double().cpu()
    kept_t = torch.from_numpy(kept)
    assert torch.equal(got != dropped_value, kept_t), \
        "mask differs from the mirror at %d elements" % int(((got != dropped_value) != kept_t).sum())
    assert bool((got[~kept_t] == dropped_value).all())
    exp = _expect(ref, kept, keep) + shift
    err = ((got - exp).abs().max() / ref.abs().max()).item()
    assert err < TOL[out.dtype], err
    assert bool((out[:, N:] == PAD).all()), "stored past column N"


def _run(M, N, K, ldc, op_dtype, out_dtype, tile, keep=0.75, seed=9, step=5, splits=1, **kw):
    A, B, ref = _operands(M, N, K, op_dtype)
    out = torch.full((M, ldc), PAD, device=DEV, dtype=out_dtype)
    ctr = None if step is None else torch.tensor([step], dtype=torch.int64, device=DEV)
    ops.gemm(A, B, out, M=M, N=N, K=K, ldc=ldc, tile=tile, splits=splits, keep=keep, seed=seed, counter=ctr, **kw)
    torch.cuda.synchronize()
    if ctr is not None:
        assert int(ctr.item()) == step, "the GEMM must not advance the counter"
    return out, ref, mirror_mask(seed, step or 0, M, N, keep, ldc=ldc)


DTYPES = [(bf, bf), (bf, torch.float32), (torch.float32, torch.float32), (torch.float32, bf)]


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("N,ldc", [(200, 200), (203, 203), (203, 208)])
def test_dropout_mask_register_staged_tiles(tile, N, ldc):
    """ldc = 200: the 8-column vector stores; ldc = 203: the per-element path; N = 203 in ldc = 208:
    vector stores with a per-element last chunk.  The mask index is step * M*N + row * ldc + col."""
    M, K = 70, 64
    for op_dtype, out_dtype in DTYPES:
        for step in (5, BIG):
            out, ref, kept = _run(M, N, K, ldc, op_dtype, out_dtype, tile, step=step)
            _check(out, N, ref, kept, 0.75)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [bf, torch.float32])
def test_dropout_mask_per_element_branch_equals_vector_branch(tile, dtype):
    """A second output or beta != 0 sends every chunk through dense_epi; the mask must be the one the
    vector branch applies to the same GEMM (both equal the mirror bit for bit)."""
    M, N, K = 70, 200, 64
    vec, ref, kept = _run(M, N, K, N, dtype, dtype, tile)
    _check(vec, N, ref, kept, 0.75)
    out2 = torch.full((M, N), PAD, device=DEV, dtype=torch.float32)
    el, _, _ = _run(M, N, K, N, dtype, dtype, tile, out2=out2, ldc2=N)
    _check(el, N, ref, kept, 0.75)
    _check(out2, N, ref, kept, 0.75)
    assert torch.equal(el == 0, vec == 0)
    # beta: out = dropout(x) + 0.5 * old with old = 2 everywhere -> dropped elements are exactly 1.0
    A, B, _ = _operands(M, N, K, dtype)
    acc = torch.full((M, N), 2.0, device=DEV, dtype=dtype)
    ctr = torch.tensor([5], dtype=torch.int64, device=DEV)
    ops.gemm(A, B, acc, M=M, N=N, K=K, tile=tile, keep=0.75, seed=9, counter=ctr, beta=0.5)
    _check(acc, N, ref, kept, 0.75, dropped_value=1.0, shift=1.0)


@pytest.mark.parametrize("tile", [0, 2])
@pytest.mark.parametrize("N", [200, 203])
def test_dropout_mask_splitk_last_arriver(tile, N):
    """splits = 3 over K = 192: only the split that arrives last runs the epilogue, so the mask (and
    the 1 / keep scale) is applied once to the summed tile."""
    M, K = 70, 192
    for op_dtype, out_dtype in ((bf, bf), (torch.float32, torch.float32)):
        for step in (5, BIG):
            out, ref, kept = _run(M, N, K, N, op_dtype, out_dtype, tile, step=step, splits=3)
            _check(out, N, ref, kept, 0.75)


@pytest.mark.parametrize("tile", [12, 19, ops.FC_TILE])
@pytest.mark.parametrize("out_dtype", [bf, torch.float32])
def test_dropout_mask_glds_tiles(tile, out_dtype):
    M = N = 256
    K = 128
    A, B, _ = _operands(M, N, K, bf)
    assert ops.glds_ok(A, B, M, N, K, tile, K, K)
    for step in (5, BIG):
        out, ref, kept = _run(M, N, K, N, bf, out_dtype, tile, step=step)
        _check(out, N, ref, kept, 0.75)


@pytest.mark.parametrize("out_dtype", [torch.float32, bf])
def test_dropout_mask_small_f32_tile(out_dtype):
    M, N, K = 17, 33, 40
    assert ops.small_f32_ok(M, N, K)
    for keep in (0.75, 0.5, 0.9):
        for step in (5, BIG):
            out, ref, kept = _run(M, N, K, N, torch.float32, out_dtype, ops.TILE_SMALL, keep=keep, step=step)
            _check(out, N, ref, kept, keep)


@pytest.mark.parametrize("tile", [0, ops.TILE_SMALL])
def test_dropout_counter_and_keep_handling(tile):
    """counter=None is step 0; counters 0 and 5 give different masks, each its mirror; keep 0.5 and
    0.9 (compared as float32(0.9)); keep = 1.0 is bitwise the call without dropout arguments."""
    M, N, K = 70, 200, 64
    f = torch.float32
    masks = {}
    for step in (None, 0, 5):
        out, ref, kept = _run(M, N, K, N, f, f, tile, step=step)
        _check(out, N, ref, kept, 0.75)
        masks[step] = kept
    assert np.array_equal(masks[None], masks[0]) and not np.array_equal(masks[0], masks[5])
    for keep in (0.5, 0.9):
        out, ref, kept = _run(M, N, K, N, f, f, tile, keep=keep)
        _check(out, N, ref, kept, keep)
    A, B, _ = _operands(M, N, K, f)
    one, _, _ = _run(M, N, K, N, f, f, tile, keep=1.0)
    plain = torch.full((M, N), PAD, device=DEV)
    ops.gemm(A, B, plain, M=M, N=N, K=K, tile=tile)
    assert torch.equal(one, plain) and bool((plain != 0).all())


@pytest.mark.parametrize("tile", [0, ops.TILE_SMALL])
def test_dropout_keep_is_compared_in_fp32(tile):
    """keep = 0.9 is no fp32 number.  The counter is chosen so that one element's uniform EQUALS
    float32(0.9): the kernel (u < float keep) drops it, as the mirror and the CPU reference do; a
    comparison with the double 0.9 would keep it."""
    M, N, K = 17, 33, 40
    step, o = divmod(U_EQ_IDX, M * N)
    assert ops.hash_uniform(9, U_EQ_IDX) == np.float32(0.9)
    out, ref, kept = _run(M, N, K, N, torch.float32, torch.float32, tile, keep=0.9, seed=9, step=step)
    assert not kept.reshape(-1)[o]
    assert out.reshape(-1)[o].item() == 0.0
    _check(out, N, ref, kept, 0.9)
    A, B, _ = _operands(M, N, K, torch.float32)
    cpu = torch.full((M, N), PAD)
    ops.gemm(A.cpu(), B.cpu(), cpu, M=M, N=N, K=K, keep=0.9, seed=9, counter=torch.tensor([step]))
    assert torch.equal(cpu == 0, out.cpu() == 0)


@pytest.mark.parametrize("out_dtype", [torch.float32, bf])
def test_bias_act_dropout_matches_cpu_reference(out_dtype):
    """bias_act_kernel (n = 1850 is no multiple of the 256-thread workgroup): stream index
    step * M*N + i, against ops.bias_act's CPU path."""
    M, N = 37, 50
    g = torch.Generator().manual_seed(3)
    x = torch.rand(M, N, generator=g) + 0.5
    bias = torch.rand(N, generator=g)
    for step in (0, BIG):
        out = torch.full((M, N), PAD, device=DEV, dtype=out_dtype)
        ctr = torch.tensor([step], dtype=torch.int64, device=DEV)
        ops.bias_act(x.to(DEV), bias.to(DEV), out, ops.ACT_RELU, keep=0.75, seed=6, counter=ctr)
        torch.cuda.synchronize()
        assert int(ctr.item()) == step
        ref = torch.empty(M, N, dtype=out_dtype)
        ops.bias_act(x, bias, ref, ops.ACT_RELU, keep=0.75, seed=6, counter=ctr.cpu())
        u = ops.hash_uniform(6, np.arange(M * N, dtype=np.uint64) + np.uint64(step * M * N))
        kept = torch.from_numpy(u < np.float32(0.75)).reshape(M, N)
        got = out.cpu()
        assert torch.equal(got != 0, kept) and torch.equal(ref != 0, kept), step
        err = ((got.double() - ref.double()).abs().max() / ref.double().abs().max()).item()
        assert err < (1e-6 if out_dtype == torch.float32 else 4e-3), err  # one fp32 ulp / half a bf16 ulp


# ------------------------------------------------------------------ sampling
N_ROWS = 5000


def _id_rows(D, seed=0):
    """uint8 [5000][D] whose first two bytes hold the row id in base 128 (exact after / 255 and a
    bf16 round trip: |error| <= 127 * 2^-9 < 0.25 of a byte step)."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (N_ROWS, D), generator=g, dtype=torch.uint8)
    ids = torch.arange(N_ROWS)
    src[:, 0] = (ids // 128).to(torch.uint8)
    src[:, 1] = (ids % 128).to(torch.uint8)
    return src


def _decode(dst):
    b = torch.round(dst[:, :2].float().cpu() * 255).long()
    return b[:, 0] * 128 + b[:, 1]


def _mirror_rows(seed, step, B):
    return torch.from_numpy((ops.hash_u32(seed, np.uint64(step * B) + np.arange(B, dtype=np.uint64))
                             % np.uint32(N_ROWS)).astype(np.int64))


@pytest.mark.parametrize("B", [64, 37])
@pytest.mark.parametrize("D", [784, 30])
@pytest.mark.parametrize("dtype", [bf, torch.float32])
def test_gather_rows_samples_the_mirror_rows(B, D, dtype):
    """gather_rows(idx=None): row(b) = hash_u32(seed, c * B + b) % n_rows for counter value c, on the
    8-element item path (D = 784) and the wave-per-row path (D = 30); the counter advances by one
    per call with ``done``, not at all without; consecutive calls draw different batches."""
    seed = 11
    src_cpu = _id_rows(D)
    src = src_cpu.to(DEV)
    lab = torch.arange(N_ROWS, dtype=torch.int32, device=DEV)
    lab10 = lab % 10
    tol = 1e-6 if dtype == torch.float32 else 4e-3
    for c in (0, 7, BIG):
        ctr = torch.tensor([c], dtype=torch.int64, device=DEV)
        done = torch.zeros(1, dtype=torch.int32, device=DEV)
        drawn = []
        for call, with_done in enumerate((True, True, False)):
            dst = torch.full((B, D), PAD, device=DEV, dtype=dtype)
            ld = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            oh = torch.full((B, 10), PAD, device=DEV)
            step = c + min(call, 2)
            if call == 0:
                ops.gather_rows(src, dst, None, lab, ld, seed=seed, counter=ctr, done=done)
            else:
                ops.gather_rows(src, dst, None, lab10, ld, seed=seed, counter=ctr, done=done if with_done else None,
                                onehot=oh)
            torch.cuda.synchronize()
            rows = _mirror_rows(seed, step, B)
            assert torch.equal(_decode(dst), rows), (c, call)
            assert torch.equal(ld.cpu().long(), rows if call == 0 else rows % 10), (c, call)
            if call:
                assert torch.equal(oh.cpu(), torch.nn.functional.one_hot(rows % 10, 10).float()), (c, call)
            exp = src_cpu[rows].double() / 255
            assert ((dst.double().cpu() - exp).abs().max() / exp.abs().max()).item() < tol
            assert int(ctr.item()) == step + (1 if with_done else 0), (c, call)
            drawn.append(rows)
        assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])


# --------------------------------------------------------------------- noise
@pytest.mark.parametrize("with_copy", [False, True])
@pytest.mark.parametrize("start", [0, BIG])
def test_uniform_fill_follows_the_mirror(with_copy, start):
    """Call k (counter value k) of uniform_fill is lo + (hi - lo) * hash_uniform(seed ^ 0xA5A5A5A5, k * n + i),
    within one fp32 ulp of max(|lo|, |hi|) (the device may contract the multiply-add)."""
    lo, hi, seed = -1.0, 1.0, 9
    z = torch.empty(128, 100, device=DEV)
    n = z.numel()
    ctr = torch.tensor([start], dtype=torch.int64, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    csrc = torch.rand(64, 100, device=DEV)
    fills = []
    for call in range(2):
        cdst = torch.full((64, 100), PAD, device=DEV)
        ops.uniform_fill(z, lo, hi, seed=seed, counter=ctr, done=done, copy=(csrc, cdst) if with_copy else None)
        torch.cuda.synchronize()
        k = start + call
        u = ops.hash_uniform(seed ^ 0xA5A5A5A5, np.uint64(k * n) + np.arange(n, dtype=np.uint64))
        exp = torch.from_numpy(lo + (hi - lo) * u.astype(np.float64)).reshape(128, 100)
        assert (z.double().cpu() - exp).abs().max().item() <= 2.0 ** -23 * max(abs(lo), abs(hi)), call
        assert int(ctr.item()) == k + 1
        assert torch.equal(cdst, csrc) if with_copy else bool((cdst == PAD).all())
        fills.append(z.clone())
    assert not torch.equal(fills[0], fills[1])
