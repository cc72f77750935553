"""Op layer: thin wrappers over ``torch.ops.dtfe`` (gfx950 HIP kernels).

Every op writes into caller-provided tensors (no allocation inside a step, so
steps are hipGraph-capturable).  GPU tensors always go to the HIP kernels -
if the native library is missing that is an error, never a silent fallback.
CPU tensors take a plain-PyTorch reference path: it exists for the CPU/gloo
plumbing configuration (BASELINE.json config 1), for CPU tests of the
distributed machinery, and as the fp32 oracle the kernel tests compare to.
"""
from __future__ import annotations

import collections
import contextlib
import functools
import math
import os

import numpy as np
import torch

from ._lib import (ACT_CODES, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, KMAJ, OPT_ADAM, OPT_MOMENTUM,
                   OPT_RMSPROP, OPT_SGD, RMAJ, available, load, require)

__all__ = [
    "gemm", "linear_fwd", "conv_fwd", "conv_dgrad", "conv_wgrad", "head_xent", "apply_gradients", "apply_gradients_group", "opt_state",
    "gather_rows", "uniform_fill", "cast_", "softmax_xent", "gan_loss", "mse_sigmoid", "colsum", "act_grad",
    "bias_act", "ACT_NONE", "ACT_RELU", "ACT_SIGMOID", "ACT_TANH", "ACT_CODES", "KMAJ", "RMAJ", "OPT_SGD",
    "OPT_MOMENTUM", "OPT_ADAM", "OPT_RMSPROP", "available", "load", "require", "pick_tile", "split_workspace",
    "TILE_DIMS", "FC_TILE", "TILE_SMALL", "GEMM_KTILE", "GLDS_TILES", "glds_ok", "ones_page", "bn_stats", "bn_apply", "bn_bwd_stats",
    "bn_bwd_apply", "relu_bits", "shortcut_grad_add",
    "gap_fwd", "gap_bwd", "gemm_group", "seq_stage", "wgrad_tallk", "tallk_ws_floats", "maxpool3_fwd", "maxpool3_bwd", "bn_relu_pool3", "pool3_bn_bwd", "imgconv", "imgwgrad", "hash_u32", "hash_uniform",
    "imgconv_shortcut", "dense_head", "WgradReduces", "conv1_wgrad_pooled_f32",
    "head_xent_f32", "gan_disc_head", "gan_head_ws_floats", "epoch_signal", "grad_norm_plan", "grad_sumsq", "scale_",
    "augment_rows", "augment_draws", "AUG_SALT", "mix_draws", "mix_r24", "smoothing_values", "MIX_LAM_SALT", "MIX_BOX_SALT",
    "MIX_ROT_SALT", "MIX_MODES", "epoch_permutation", "shuffled_rows", "SHUF_SALT", "lr_schedule_spec", "lr_schedule_value", "lr_schedule_pack",
    "eval_metrics", "eval_state", "eval_state_dict", "eval_rows_ref",
    "ema_swap", "ema_decay_value", "ema_update_ref",
    "layer_trust", "layer_trust_plan", "lars_trust_ref", "LARS_CHUNK_MAX",
]

_TILES = [(1, 128, 128), (2, 128, 64), (3, 64, 128), (0, 64, 64)]
TILE_DIMS = {0: (64, 64), 1: (128, 128), 2: (128, 64), 3: (64, 128), 4: (32, 32),
             # global_load_lds kernel family (csrc/kernels/gemm_glds.h): bf16, K % 64 == 0, whole tiles
             5: (128, 128), 6: (128, 64), 7: (64, 128), 8: (64, 64),      # 3 k-tiles in flight
             9: (128, 128), 10: (128, 64), 11: (64, 128), 12: (64, 64),   # 2 stages (more WGs per CU)
             13: (16, 16),   # exact-fp32 small-layer kernel (gemm_small.hip): no split-K, in-WG K split
             14: (64, 64), 15: (64, 64), 16: (64, 64),  # 4 / 6 / 8 stages (long-K grids, ~1 WG per CU)
             17: (128, 64), 18: (128, 64),              # 4 / 6 stages
             19: (64, 64), 20: (64, 64), 21: (64, 64),  # 2 / 4 / 2 in-workgroup k-groups (3 / 2 / 4 stages)
             22: (256, 128)}  # 8-wave fc tile (gemm_fc.hip): M % 256, N any (clamped last tile), 3 stages
FC_TILE = 22
GLDS_TILES = (5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 20, 21, 22)
TILE_SMALL = 13
_ONES = {}


def ones_page(device):
    """1 KB of bf16 ones (the bias column of a glds weight-gradient GEMM reads it)."""
    key = torch.device(device)
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones(512, dtype=torch.bfloat16, device=key)
    return t


def glds_ok(A, B, M, N, K, tile, lda, ldb, b_ones_row=-1, a_ones_row=-1, bmode=KMAJ):
    """Host mirror of gemm_glds_eligible: can the global_load_lds tile `tile` run this GEMM?"""
    bm, bn = TILE_DIMS[tile]
    if A.dtype != torch.bfloat16 or B.dtype != torch.bfloat16 or a_ones_row >= 0 or K % 64 or M % bm:
        return False
    if lda % 8 or ldb % 8 or A.data_ptr() % 16 or B.data_ptr() % 16:
        return False
    if tile == FC_TILE:  # mirror of gemm_fc_eligible (csrc/kernels/gemm_fc.hip)
        valid = b_ones_row if b_ones_row >= 0 else N
        if b_ones_row >= 0 and (b_ones_row != N - 1 or b_ones_row % 8):
            return False
        return valid >= 8 and valid % 8 == 0 and (bmode == RMAJ or (N % bn == 0 and b_ones_row < 0))
    if b_ones_row >= 0:
        return b_ones_row == N - 1 and b_ones_row % bn == 0
    return N % bn == 0
GEMM_KTILE = 64  # k-tile depth of the dense GEMM kernels (split-K chunks are multiples of it)
_WS = {}
# Every workspace ever handed out stays alive: a hipGraph captured with an older (smaller)
# buffer keeps its device pointers, and the caching allocator must never recycle that memory.
_WS_RETIRED = []


def split_workspace(device, splits, M, N, tile, private=False):
    """(ws, tile_ctr) for a split-K GEMM with a fused epilogue: fp32 partial tiles
    [splits][tiles][BM*BN] + per-tile arrival counters (zeroed once; the kernel
    resets them).  Cached per device and grown on demand - callers that run
    split-K GEMMs concurrently on several streams must pass their own
    (``private=True``: a fresh pair, not the shared cache)."""
    bm, bn = TILE_DIMS[tile]
    ntiles = math.ceil(M / bm) * math.ceil(N / bn)
    need = splits * ntiles * bm * bn
    if private:
        key = torch.device(device)
        return (torch.empty(need, device=key, dtype=torch.float32),
                torch.zeros(ntiles, device=key, dtype=torch.int32))
    key = torch.device(device)
    ws, ctr = _WS.get(key, (None, None))
    if ws is None or ws.numel() < need or ctr.numel() < ntiles:
        if ws is not None:
            _WS_RETIRED.append((ws, ctr))
        ws = torch.empty(max(need, 0 if ws is None else ws.numel()), device=key, dtype=torch.float32)
        ctr = torch.zeros(max(ntiles, 0 if ctr is None else ctr.numel()), device=key, dtype=torch.int32)
        _WS[key] = (ws, ctr)
    return ws, ctr


def auto_splits(M: int, N: int, K: int, tile: int) -> int:
    """Split-K factor for an under-filled GEMM (few output tiles, long K: the small dense layers
    of the reference models, a weight gradient reducing over T*B rows) so the grid reaches
    ~256 workgroups; the last-arriving split runs the fused epilogue (deterministic order).
    Uses the shared per-device workspace: GEMMs issued concurrently on several streams must not
    rely on it (pass splits / workspace explicitly)."""
    if tile == TILE_SMALL:
        return 1
    bm, bn = TILE_DIMS[tile]
    tiles = math.ceil(M / bm) * math.ceil(N / bn)
    if tiles >= 128 or K < 4 * GEMM_KTILE:
        return 1
    return max(1, min(math.ceil(256 / tiles), K // (2 * GEMM_KTILE), 16))


def small_f32_ok(M: int, N: int, K: int) -> bool:
    """The small-layer fp32 kernel wins where the output has at most ~1M elements (<= 4096
    16x16 tiles) and K is short enough for register-direct operands (reference GAN /
    autoencoder layers: 1.7-10 us -> ~2-3 us each); DTFE_GEMM_SMALL=0 disables it."""
    return _SMALL_ON and math.ceil(M / 16) * math.ceil(N / 16) <= 4096 and K <= 2048


_SMALL_ON = os.environ.get("DTFE_GEMM_SMALL", "1") != "0"


def pick_tile(M: int, N: int) -> int:
    """Largest MFMA tile that still yields >= one workgroup per CU (256 CUs)."""
    if M <= 32 and N <= 32:
        return 4
    for tid, bm, bn in _TILES:
        if math.ceil(M / bm) * math.ceil(N / bn) >= 256:
            return tid
    # small outputs: 32x32 tiles quadruple the workgroups of 64x64 (split-K adds more if K allows)
    return 4 if math.ceil(M / 64) * math.ceil(N / 64) < 64 else 0


# --------------------------------------------------------------- references
def hash_u32(seed, idx):
    """Host mirror of the kernels' counter-based RNG (common.h hash_u32): splitmix-style 64-bit mix
    of (seed, element index), low 32 bits, as a numpy uint32 (array-shaped like ``idx``).  Batch
    sampling takes it modulo the row count: row(b) = hash_u32(seed, step * B + b) % n_rows."""
    with np.errstate(over="ignore"):
        z = (np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) * np.uint64(0x9E3779B97F4A7C15)
             + np.asarray(idx, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03) + np.uint64(0x632BE59BD9B4E019))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def hash_uniform(seed, idx):
    """Host mirror of common.h hash_uniform: the top 24 bits of hash_u32 -> fp32 uniform [0, 1)."""
    return (hash_u32(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


AUG_SALT = 0xC1FA5A17D00D5EED  # csrc/kernels/augment.h: the crop / flip draws' stream is hash_u32(seed ^ AUG_SALT, .)
AUG_MAX_PAD = 15


def augment_draws(seed, step, B, pad, flip):
    """Host mirror of augment_rows' per-sample draws at counter value ``step``: (dy, dx, flipped),
    int64 / int64 / bool arrays [B].  h = hash_u32(seed ^ AUG_SALT, step * B + b), span = 2 * pad + 1:
    dx = h % span, dy = (h / span) % span, flipped = flip and bit 0 of h / span^2."""
    m64 = 0xFFFFFFFFFFFFFFFF
    i = np.uint64((int(step) * int(B)) & m64) + np.arange(B, dtype=np.uint64)
    h = hash_u32((int(seed) & m64) ^ AUG_SALT, i).astype(np.int64)
    span = 2 * int(pad) + 1
    dx = h % span
    dy = (h // span) % span
    flipped = ((h // (span * span)) & 1).astype(bool) & bool(flip)
    return dy, dx, flipped


# csrc/kernels/augment.h: the streams of mixup's / CutMix's lambda, CutMix's box centre and the partner rotation
MIX_LAM_SALT = 0x4D1C5EEDB1E2D0A7
MIX_BOX_SALT = 0xB0C5CE27E4A1F00D
MIX_ROT_SALT = 0x9A27E4F00D5EED13
MIX_MODES = {"none": 0, "mixup": 1, "cutmix": 2}
MixDraws = collections.namedtuple("MixDraws", "shift partner k lam box lam_box")


def mix_r24(k):
    """CutMix's box scale for the 24-bit draw k: floor(sqrt((2^24 - k) * 2^24)) = floor(2^24 * sqrt(1 - lam)),
    an exact integer (math.isqrt; the kernel corrects a double-precision root against r^2 <= v < (r + 1)^2)."""
    return math.isqrt(((1 << 24) - int(k)) << 24)


def mix_draws(seed, step, B, H, W):
    """Host mirror of augment_rows' mixing draws for the batch at counter value ``step`` (augment.h), i = step * B + b:
    ``shift`` = 1 + hash_u32(seed ^ MIX_ROT_SALT, step) % (B - 1) and ``partner`` [B] = (b + shift) % B, a rotation
    without a fixed point; ``k`` [B] = hash_u32(seed ^ MIX_LAM_SALT, i) >> 8 and ``lam`` [B] float32 = k * 2^-24
    (mixup's weight of slot b; Uniform[0, 1) = Beta(1, 1)); CutMix's ``box`` (y0, y1, x0, x1), int64 [B] each:
    half-sides rw = (W * mix_r24(k)) >> 24, rh alike, centre cx = hb % W, cy = (hb / W) % H of
    hb = hash_u32(seed ^ MIX_BOX_SALT, i), clipped to the image; ``lam_box`` [B] float32 =
    float32(H * W - box area) * float32(1 / float32(H * W)), the label weight of slot b under CutMix."""
    B, H, W = int(B), int(H), int(W)
    if B < 2 or H < 1 or W < 1:
        raise ValueError("mix_draws: needs B >= 2 and H, W >= 1 (got B = %d, %d x %d)" % (B, H, W))
    m64 = 0xFFFFFFFFFFFFFFFF
    seed, s = int(seed) & m64, int(step) & m64
    i = np.uint64((s * B) & m64) + np.arange(B, dtype=np.uint64)
    shift = 1 + int(hash_u32(seed ^ MIX_ROT_SALT, np.uint64(s))) % (B - 1)
    partner = (np.arange(B, dtype=np.int64) + shift) % B
    k = (hash_u32(seed ^ MIX_LAM_SALT, i) >> np.uint32(8)).astype(np.int64)
    lam = k.astype(np.float32) * np.float32(2.0 ** -24)
    r24 = np.array([mix_r24(v) for v in k], dtype=np.int64)
    rw, rh = (W * r24) >> 24, (H * r24) >> 24
    hb = hash_u32(seed ^ MIX_BOX_SALT, i).astype(np.int64)
    cx, cy = hb % W, (hb // W) % H
    x0, x1 = np.maximum(cx - rw // 2, 0), np.minimum(cx + rw // 2, W)
    y0, y1 = np.maximum(cy - rh // 2, 0), np.minimum(cy + rh // 2, H)
    inv_hw = np.float32(1.0) / np.float32(H * W)
    lam_box = (H * W - (x1 - x0) * (y1 - y0)).astype(np.float32) * inv_hw
    return MixDraws(shift, partner, k, lam, (y0, y1, x0, x1), lam_box)


def smoothing_values(label_smoothing, ncls):
    """(on, off) of a label row under label smoothing E, in float32 as the binding computes them:
    off = E / ncls, on = (1 - E) + off; E = 0 gives exactly (1, 0)."""
    e = np.float32(label_smoothing)
    off = e / np.float32(ncls)
    return np.float32(1.0) - e + off, off


SHUF_SALT = 0x5EED0FE90C45A1D3  # csrc/kernels/common.h: the epoch permutations' key is seed ^ SHUF_SALT


def _perm_index(key, epoch, n, i):
    """common.h perm_index on arrays: ``epoch`` and ``i`` broadcast together (uint64), one ``n``."""
    m64 = 0xFFFFFFFFFFFFFFFF
    n = int(n)
    bits = max(2, ((n - 1).bit_length() + 1) & ~1)
    h = np.uint64(bits // 2)
    mask = np.uint64((1 << (bits // 2)) - 1)
    epoch, x = np.broadcast_arrays(np.asarray(epoch, dtype=np.uint64), np.asarray(i, dtype=np.uint64))
    e = epoch << np.uint64(18)  # (wraps modulo 2^64, as on the device)
    x = x.copy()
    walk = np.ones(x.shape, dtype=bool)  # the elements still outside [0, n) - all of them take the first pass
    while walk.any():
        L, R, ew = x[walk] >> h, x[walk] & mask, e[walk]
        for r in range(4):
            L, R = R, L ^ (hash_u32(key & m64, ew | np.uint64(r << 16) | R).astype(np.uint64) & mask)
        x[walk] = (L << h) | R
        walk = x >= np.uint64(n)
    return x.astype(np.int64)


def epoch_permutation(seed, epoch, n):
    """Host mirror of the device's epoch shuffle (common.h perm_index): the permutation of [0, n),
    1 <= n <= 2^31, that epoch ``epoch`` of the stream ``seed`` visits, int64 [n], bit-exact.

    A balanced Feistel network over the smallest even-width power-of-two domain holding n, cycle-walked:
    bits = bit length of n - 1 rounded up to even and at least 2, h = bits / 2, mask = 2^h - 1; one pass
    splits x into (L, R) = (x >> h, x & mask) and runs 4 rounds r = 0..3 of
        (L, R) <- (R, L ^ (hash_u32(key, epoch << 18 | r << 16 | R) & mask)),   key = seed ^ SHUF_SALT,
    giving x' = L << h | R; element i is the first value below n among pass(i), pass(pass(i)), ...
    (epoch << 18 wraps modulo 2^64)."""
    n = int(n)
    if not 1 <= n <= 1 << 31:
        raise ValueError("epoch_permutation: 1 <= n <= 2^31, got %d" % n)
    m64 = 0xFFFFFFFFFFFFFFFF
    return _perm_index((int(seed) & m64) ^ SHUF_SALT, np.uint64(int(epoch) & m64), n, np.arange(n, dtype=np.uint64))


def shuffled_rows(seed, counter, B, n):
    """Host mirror of the epoch-exact batch sampling (gather_rows / augment_rows ``shuffle=True``): the
    rows of the batch at counter value ``counter``, int64 [B].  Position p = counter * B + b reads
    epoch_permutation(seed, p // n, n)[p % n]: every row once per epoch, a batch that straddles an epoch
    boundary stitched from the tail of one epoch and the head of the next (B > n spans several)."""
    n = int(n)
    if not 1 <= n <= 1 << 31:
        raise ValueError("shuffled_rows: 1 <= n <= 2^31, got %d" % n)
    m64 = 0xFFFFFFFFFFFFFFFF
    p = np.uint64((int(counter) * int(B)) & m64) + np.arange(int(B), dtype=np.uint64)
    e = p // np.uint64(n)
    return _perm_index((int(seed) & m64) ^ SHUF_SALT, e, n, p - e * np.uint64(n))


def _sampled_rows(seed, counter, B, n, shuffle):
    """The rows a launch without ``idx`` samples at counter value ``counter`` (torch int64 [B])."""
    if shuffle:
        return torch.from_numpy(shuffled_rows(seed, counter, B, n))
    i = np.uint64((int(counter) * int(B)) & 0xFFFFFFFFFFFFFFFF) + np.arange(int(B), dtype=np.uint64)
    return torch.from_numpy((hash_u32(seed, i) % np.uint32(n)).astype(np.int64))


def _dropout_ref(x, idx, keep, seed, base):
    """The kernels' dropout on the CPU: element with stream index ``base + idx`` is kept where its
    fp32 uniform is < float32(keep), and scaled by the fp32 reciprocal 1.f / keep (fp32 product)."""
    k = np.float32(keep)
    u = hash_uniform(seed, np.asarray(idx, dtype=np.uint64).reshape(-1) + np.uint64(base))
    kept = torch.from_numpy(u < k).reshape(x.shape)
    inv = torch.tensor(float(np.float32(1.0) / k), dtype=torch.float32)
    return torch.where(kept, x.float() * inv, torch.zeros_like(x, dtype=torch.float32))


def _act_ref(x, act):
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    if act == ACT_TANH:
        return torch.tanh(x)
    return x


def _act_grad_from_out_ref(y, act):
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == ACT_SIGMOID:
        return y * (1 - y)
    if act == ACT_TANH:
        return 1 - y * y
    return torch.ones_like(y)


def _mat(t, mode, rows, K, ld):
    """Logical [rows, K] fp32 view of an operand given its mode/leading dim."""
    flat = t.reshape(-1).float()
    if mode == KMAJ:
        idx = torch.arange(rows).unsqueeze(1) * ld + torch.arange(K).unsqueeze(0)
    else:
        idx = torch.arange(K).unsqueeze(0) * ld + torch.arange(rows).unsqueeze(1)
    return flat[idx]


# --------------------------------------------------------------------- GEMM
def gemm(A, B, out, *, M, N, K, amode=KMAJ, lda=None, bmode=KMAJ, ldb=None, ldc=None, bias=None, bias_axis=0,
         act=ACT_NONE, alpha=1.0, beta=0.0, atomic=False, splits=1, tile=None, aux=None, ld_aux=None, aux_act=0,
         b_ones_row=-1, keep=1.0, seed=0, counter=None, pooled=None, argmax=None, PH=0, PW=0, PC=0, out2=None,
         ldc2=0, out2_trans=False, bias_out=None, workspace=None, a_ones_row=-1, group=None):
    """out[M,N] = epilogue( A(m,k) . B(n,k) ).

    A(m,k) = A[m*lda+k] (KMAJ) or A[k*lda+m] (RMAJ); likewise B(n,k).
    Epilogue order: alpha*acc, +bias, act, dropout(keep), *act'(aux), [unpool | +beta*out], store.
    b_ones_row >= 0 makes B row n=b_ones_row all ones; with bias_out that output
    column goes to bias_out[m] (a weight-gradient GEMM producing the bias gradient).
    a_ones_row = M-1 is the transpose: A's last row reads as ones and output row M-1 goes to
    bias_out[n] (W[in][out] weight gradients: the bias gradient without a column-sum launch).
    splits > 1 without atomic: split-K whose last-arriving split runs the fused
    epilogue (workspace = (ws, tile_ctr), default: a per-device cached one).
    group: a ``gemm_group`` this GEMM joins if it fits (it then leaves with the group's launch);
    without one, or if it does not fit, it launches now.
    """
    if lda is None:
        lda = K if amode == KMAJ else M
    if ldb is None:
        ldb = K if bmode == KMAJ else N
    if ldc is None:
        ldc = N
    if ld_aux is None:
        ld_aux = ldc
    if out.is_cuda:
        if tile is None and A.dtype == torch.float32 and pooled is None and splits == 1 and \
                small_f32_ok(M, N, K):
            tile = TILE_SMALL
        if tile is None:
            tile = pick_tile(M, N)
            if splits == 1 and not atomic and workspace is None:
                splits = auto_splits(M, N, K, tile)
        ws = ctr = None
        if splits > 1 and not atomic:
            ws, ctr = workspace if workspace is not None else split_workspace(out.device, splits, M, N, tile)
        require().gemm(A, amode, lda, B, bmode, ldb, M, N, K, out, ldc, bias, bias_axis, act, alpha, beta, atomic,
                       splits, tile, aux, ld_aux, aux_act, b_ones_row, keep, seed, counter, pooled, argmax, PH, PW,
                       PC, out2, ldc2, out2_trans, bias_out, ws, ctr, a_ones_row,
                       ones_page(out.device) if tile in GLDS_TILES else None, group)
        return out
    # CPU reference
    if a_ones_row >= 0:
        assert a_ones_row == M - 1, "CPU reference: a_ones_row must be the last row"
        a = torch.cat([_mat(A, amode, M - 1, K, lda), torch.ones(1, K)], 0)
    else:
        a = _mat(A, amode, M, K, lda)
    if b_ones_row >= 0:
        b = _mat(B, bmode, b_ones_row, K, ldb) if b_ones_row > 0 else torch.zeros(0, K)
        b = torch.cat([b, torch.ones(1, K), _mat_tail(B, bmode, b_ones_row + 1, N, K, ldb)], 0)
    else:
        b = _mat(B, bmode, N, K, ldb)
    acc = a @ b.t()
    if bias_out is not None and a_ones_row >= 0:
        if atomic:
            bias_out += alpha * acc[a_ones_row]
        else:
            bias_out.copy_(alpha * acc[a_ones_row])
        acc = acc[:a_ones_row]
        M = a_ones_row
    elif bias_out is not None:
        if atomic:
            bias_out += alpha * acc[:, b_ones_row]
        else:
            bias_out.copy_(alpha * acc[:, b_ones_row])
        keep_cols = [c for c in range(N) if c != b_ones_row]
        acc = acc[:, keep_cols]
        N = len(keep_cols)
    oflat = out.view(-1)
    oidx = torch.arange(M).unsqueeze(1) * ldc + torch.arange(N).unsqueeze(0)
    if atomic:
        oflat[oidx] += (alpha * acc).to(out.dtype)
        return out
    x = alpha * acc
    if bias is not None:
        x = x + (bias.float().view(1, -1) if bias_axis == 0 else bias.float().view(-1, 1))
    x = _act_ref(x, act)
    if keep < 1.0:
        step = int(counter.reshape(-1)[0].item()) if counter is not None else 0
        oidx0 = torch.arange(M).unsqueeze(1) * ldc + torch.arange(N).unsqueeze(0)
        x = _dropout_ref(x, oidx0.numpy(), keep, seed, step * M * N)
    if aux is not None:
        aidx = torch.arange(M).unsqueeze(1) * ld_aux + torch.arange(N).unsqueeze(0)
        x = x * _act_grad_from_out_ref(aux.reshape(-1).float()[aidx], aux_act)
    if pooled is not None:
        _unpool_ref(x.reshape(-1), pooled, argmax, PH, PW, PC, out)
        return out
    if beta != 0.0:
        x = x + beta * oflat[oidx].float()
    oflat[oidx] = x.to(out.dtype)
    if out2 is not None:
        o2 = out2.view(-1)
        idx2 = (torch.arange(N).unsqueeze(0) * ldc2 + torch.arange(M).unsqueeze(1)) if out2_trans else \
            (torch.arange(M).unsqueeze(1) * ldc2 + torch.arange(N).unsqueeze(0))
        o2[idx2] = x.to(out2.dtype)
    return out


def _mat_tail(t, mode, r0, rows, K, ld):
    """Rows r0..rows-1 of the logical [rows, K] operand (those that exist in memory)."""
    if r0 >= rows:
        return torch.zeros(0, K)
    flat = t.reshape(-1).float()
    r = torch.arange(r0, rows)
    if mode == KMAJ:
        idx = r.unsqueeze(1) * ld + torch.arange(K).unsqueeze(0)
    else:
        idx = torch.arange(K).unsqueeze(0) * ld + r.unsqueeze(1)
    return flat[idx]


def _unpool_ref(g, pooled, argmax, PH, PW, C, dz):
    """Route pooled-grad g (flat [B*PH*PW*C]) to argmax positions, ReLU-masked by pooled>0."""
    Bn = g.numel() // (PH * PW * C)
    g = g.view(Bn, PH, PW, C) * (pooled.view(Bn, PH, PW, C).float() > 0)
    am = argmax.view(Bn, PH, PW, C).long()
    full = torch.zeros(Bn, PH, 2, PW, 2, C)
    for q in range(4):
        full[:, :, q >> 1, :, q & 1, :] = torch.where(am == q, g, torch.zeros_like(g))
    dz.view(-1)[:] = full.reshape(-1).to(dz.dtype)


def linear_fwd(x, w_kn, b, out, act=ACT_NONE):
    """TF-layout dense layer: out = act(x[M,K] . W[K,N] + b)."""
    M, K = x.shape[0], x.shape[-1]
    N = w_kn.shape[1]
    return gemm(x, w_kn, out, M=M, N=N, K=K, amode=KMAJ, bmode=RMAJ, ldb=N, bias=b, act=act)


# -------------------------------------------------------------------- conv
def _conv_geom_args(g):
    return (g["B"], g["H"], g["W"], g["C"], g["Cout"], g["OH"], g["OW"], g["KH"], g["KW"], g["stride"], g["pad"])


def conv_fwd(x, w, bias, y, argmax, g, pool=False, act=ACT_RELU, stats=None):
    """NHWC conv (+bias, act, optional fused 2x2 max-pool writing argmax).  ``stats`` (f32 [2][Cout],
    zeroed): also accumulate the BatchNorm statistics of y exactly as ``bn_stats`` does (the
    implicit-GEMM path computes them from its epilogue tiles: no separate pass over y)."""
    if y.is_cuda:
        require().conv_fwd(x, w, bias, y, argmax, *_conv_geom_args(g), pool, act, stats)
        return y
    if stats is not None:
        conv_fwd(x, w, bias, y, argmax, g, pool, act)
        bn_stats(y, stats)
        return y
    xt = x.float().view(g["B"], g["H"], g["W"], g["C"]).permute(0, 3, 1, 2)
    wt = w.float().view(g["Cout"], g["KH"], g["KW"], g["C"]).permute(0, 3, 1, 2)
    z = torch.nn.functional.conv2d(xt, wt, bias.float() if bias is not None else None, stride=g["stride"],
                                   padding=g["pad"])
    z = _act_ref(z, act)
    if pool:
        p, idx = _pool_ref(z)
        y.view(-1)[:] = p.permute(0, 2, 3, 1).reshape(-1).to(y.dtype)
        if argmax is not None:
            argmax.view(-1)[:] = idx.permute(0, 2, 3, 1).reshape(-1).to(argmax.dtype)
    else:
        y.view(-1)[:] = z.permute(0, 2, 3, 1).reshape(-1).to(y.dtype)
    return y


def _pool_ref(z):
    """2x2/2 max pool of NCHW z; returns (pooled, argmax in 0..3 = dy*2+dx, first max wins)."""
    Bn, C, H, W = z.shape
    win = z.view(Bn, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C, H // 2, W // 2, 4)
    p, idx = win.max(dim=-1)
    # torch.max returns the first maximal index on ties
    return p, idx


def _unpooled_nhwc(pooled, argmax, B, H, W, C):
    """Full-resolution NHWC tensor holding pooled[w] at argmax position of each 2x2 window."""
    out = torch.zeros(B * H * W * C)
    _unpool_ref(pooled.reshape(-1).float(), torch.ones(B, H // 2, W // 2, C), argmax, H // 2, W // 2, C, out)
    return out.view(B, H, W, C)


def _bn_src_ref(src, bn_src, eps, momentum, save):
    """CPU oracle of a BN + ReLU formed on a conv's source (bn_src = [stats, gamma, beta, mean,
    invstd, moving_mean, moving_var]): bn_apply's output."""
    st, g, b, m, i, mm, mv = bn_src
    h = torch.empty_like(src)
    kw = dict(mean=m, invstd=i, moving_mean=mm, moving_var=mv) if save else {}
    bn_apply(src, st, g, b, h, eps=eps, momentum=momentum, act=ACT_RELU, **kw)
    return h


def imgconv(w, y, *, B, SH, SW, CS, OH, OW, N, KH, KW, stride=1, pad=0, src=None, src_pooled=None,
            src_argmax=None, bias=None, argmax=None, relu_mask=None, flip_taps=False, act=ACT_NONE, pool=False,
            dil=1, bn_src=None, bn_eps=1e-3, bn_momentum=0.99, bn_save=False):
    """Whole-image LDS convolution (small feature maps): forward (+bias/act/pool) or, with
    flip_taps and pad = K-1-pad, the data gradient of a stride-1 conv (w = Wt [cin][tap][cout]).
    The source may be un-pooled on load from (src_pooled, src_argmax), or dilated (``dil``: source
    pixel (y, x) at (y*dil, x*dil), zeros between - the data gradient of a stride-``dil`` conv).
    Returns y.  (The output BatchNorm statistics accumulated in the staged epilogue with a
    last-arriver fold measured 11-12 us slower per conv than the 4.5-6.7 us bn_stats pass it replaced -
    ResNet-20 1.312 vs 1.192 ms/step - and was removed in round 6: profiles/r6_resnet20_ostats_ab.txt.)"""
    if y.is_cuda:
        require().imgconv(src, src_pooled, src_argmax, w, bias, y, argmax, relu_mask, B, SH, SW, CS, OH, OW,
                          N, KH, KW, stride, pad, flip_taps, act, pool, dil, bn_src=bn_src, bn_eps=bn_eps,
                          bn_momentum=bn_momentum, bn_save=bn_save)
        return y
    if bn_src is not None:  # BN + ReLU formed on the source (the kernel does it while staging)
        src = _bn_src_ref(src, bn_src, bn_eps, bn_momentum, bn_save)
    s = src.float().view(B, SH, SW, CS) if src is not None else _unpooled_nhwc(src_pooled, src_argmax, B, SH, SW, CS)
    if dil > 1:
        sd = torch.zeros(B, SH * dil, SW * dil, CS)
        sd[:, ::dil, ::dil, :] = s
        s = sd
    wt = w.float().view(N, KH, KW, CS)
    if flip_taps:
        wt = wt.flip(1, 2)
    z = torch.nn.functional.conv2d(s.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2),
                                   bias.float() if bias is not None else None, stride=stride, padding=pad)
    z = z[:, :, :OH, :OW]
    z = _act_ref(z, act)
    if pool:
        p, idx = _pool_ref(z)
        y.view(-1)[:] = p.permute(0, 2, 3, 1).reshape(-1).to(y.dtype)
        if argmax is not None:
            argmax.view(-1)[:] = idx.permute(0, 2, 3, 1).reshape(-1).to(argmax.dtype)
        return y
    flat = z.permute(0, 2, 3, 1).reshape(-1)
    if relu_mask is not None:
        flat = flat * (relu_mask.reshape(-1).float() > 0)
    y.view(-1)[:] = flat.to(y.dtype)
    return y


def conv12_gather_fwd(images, labels_src, seed, counter, done, labels_dst, x, w1, b1, p1, a1, zero, w2, b2, p2, a2):
    """MNIST CNN forward up to fc1 in ONE persistent launch (GPU only, B >= 256; a missing kernel is an
    error): the step's batch sampling (``conv1_gather_fwd``'s arguments: uint8 ``images`` [rows][784],
    ``labels_src``, ``seed``, ``counter``; ``done`` empty = the counter is advanced later in the step;
    ``zero``: up to 4 accumulators cleared), conv1 + bias + ReLU + 2x2 max-pool -> ``p1`` / ``a1``, conv2 +
    bias + ReLU + 2x2 max-pool -> ``p2`` / ``a2``.  Bit-identical to conv1_gather_fwd followed by conv2's
    imgconv (csrc/kernels/imgconv12_fused.hip)."""
    if not p2.is_cuda:
        raise RuntimeError("conv12_gather_fwd: GPU only (the CPU path runs gather_rows and imgconv)")
    require().conv12_gather_fwd(images, labels_src, seed, counter, done, labels_dst, x, w1, b1, p1, a1, list(zero),
                                w2, b2, p2, a2)


def imgconv_shortcut(w, dx, g, sc_stride, *, src, **geom) -> bool:
    """Data gradient of a whole-image conv (flipped taps over ``src`` = dY, ``geom`` as for
    imgconv(flip_taps=True)) with the option-A shortcut's gradient added in the same launch:
    dx[:, ::s, ::s, :] += g[..., :N] (ops.shortcut_grad_add).  Returns True when the launch added it
    (the persistent kernel's LDS-staged epilogue); False: only dx was written and the caller adds
    the shortcut gradient.  The CPU path does both (the oracle)."""
    if dx.is_cuda:
        k = geom
        return bool(require().imgconv(src, None, None, w, None, dx, None, None, k["B"], k["SH"], k["SW"], k["CS"],
                                      k["OH"], k["OW"], k["N"], k["KH"], k["KW"], k.get("stride", 1), k.get("pad", 0),
                                      True, ACT_NONE, False, k.get("dil", 1), g, sc_stride))
    imgconv(w, dx, src=src, flip_taps=True, **geom)
    shortcut_grad_add(g, dx, sc_stride)
    return True


_WG_WS = {}


def wgrad_ws_floats(N: int, KC: int) -> int:
    """Floats of the weight-gradient partial-sum workspace (256 workgroup slabs) - mirrors
    imgwgrad_ws_floats in csrc/kernels/imgwgrad_persist.hip (the register-layout slabs of the
    persistent kernel: 8 waves x CTW column tiles x MT row tiles x 64 lanes x 4, + db)."""
    MT, CTW = (4, 7) if N > 32 else (2, 9)
    return 256 * max(N * KC + N, 8 * CTW * MT * 256 + (N + 3) // 4 * 4)


def wgrad_workspace(device, numel):
    """Cached fp32 partial-sum buffer for the persistent weight-gradient kernel
    (per device, grown on demand; single-stream use)."""
    key = torch.device(device)
    ws = _WG_WS.get(key)
    if ws is None or ws.numel() < numel:
        if ws is not None:
            _WS_RETIRED.append((ws,))  # may be referenced by a captured graph
        ws = torch.empty(numel, device=key, dtype=torch.float32)
        _WG_WS[key] = ws
    return ws


class WgradReduces(list):
    """The partial-slab reduces that ``imgwgrad(defer=self)`` calls left out (each call its own
    workspace), launched together by ``flush``.  It holds the tensors themselves, so nothing a
    pending reduce points at can be freed underneath it."""

    def add(self, ws, dw, db, scale, desc):
        self.append((ws, dw, db, float(scale), list(desc)))

    def flush(self) -> int:  # ONE grouped launch on the current stream; returns how many it summed
        n = len(self)
        if n:
            ws, dw, db, scale, desc = (list(v) for v in zip(*self))
            self.clear()
            require().wgrad_reduce_group(ws, dw, db, scale, sum(desc, []))
        return n


def imgwgrad(src, dw, db, *, B, SH, SW, CS, OH, OW, N, KH, KW, stride=1, pad=0, dy=None, dy_pooled=None,
             dy_argmax=None, scale=1.0, workspace=None, max_blocks=0, bn_src=None, bn_eps=1e-3, defer=None):
    """dW[n][tap][c] += scale * sum_p dY[p][n] src[p*stride-pad+tap][c]; db += scale * sum dY.
    On the GPU the persistent kernel stores per-workgroup partials in `workspace`
    (default: a cached per-device buffer) and a second kernel sums them - or, with ``defer`` a
    WgradReduces (and a workspace of the call's own), that sum joins the collector's next flush."""
    if dw.is_cuda:
        if workspace is None and (CS % 16 == 0 or CS == 1):
            workspace = wgrad_workspace(dw.device, wgrad_ws_floats(N, KH * KW * CS))
        deferred = defer is not None and defer is not False
        desc = require().imgwgrad(src, dy, dy_pooled, dy_argmax, dw, db, B, SH, SW, CS, OH, OW, N, KH, KW, stride,
                                  pad, scale, workspace, max_blocks, bn_src=bn_src, bn_eps=bn_eps, defer=deferred)
        if desc:  # (empty: the kernel that ran had no reduce to leave out)
            defer.add(workspace, dw, db, scale, desc)
        return
    if bn_src is not None:  # the source's BN + ReLU (nothing saved: the forward did)
        src = _bn_src_ref(src, bn_src, bn_eps, 0.99, False)
    d = dy.float().view(B, OH, OW, N) if dy is not None else _unpooled_nhwc(dy_pooled, dy_argmax, B, OH, OW, N)
    gw = torch.nn.grad.conv2d_weight(src.float().view(B, SH, SW, CS).permute(0, 3, 1, 2), (N, CS, KH, KW),
                                     d.permute(0, 3, 1, 2), stride=stride, padding=pad)
    dw.view(-1)[:] += scale * gw.permute(0, 2, 3, 1).reshape(-1)
    if db is not None:
        db += scale * d.sum(dim=(0, 1, 2))


def conv_dgrad(dy, wt, dx, g, pooled=None, argmax=None, relu_mask=None, accumulate=False, bn_bwd=None,
               acc_src=None):
    """dX of an NHWC conv (wt = W laid out [C][KH][KW][Cout]); optional un-pool epilogue, or a
    ReLU mask (dx = mask > 0 ? dx : 0) when the consumer un-pools itself.  ``accumulate``:
    dx += dX (implicit-GEMM path: C and Cout multiples of 64); with ``acc_src = (src, bits)``
    dx = dX + src * bit instead (bits: relu_bits layout) - dx's old contents are not read.
    ``bn_bwd``: the consuming BatchNorm's backward statistics of the final dx, ``(x, y, mean,
    invstd, gamma, beta, stats, act)`` with ``bn_bwd_stats`` semantics - computed in the
    implicit-GEMM epilogue (no separate pass over dx and x), or by a statistics pass after the launch."""
    if dx.is_cuda:
        b = bn_bwd or (None,) * 7 + (0,)
        src, bits = acc_src or (None, None)
        require().conv_dgrad(dy, wt, dx, *_conv_geom_args(g), pooled, argmax, relu_mask, accumulate, *b, src, bits)
        return dx
    if acc_src is not None:
        src, bits = acc_src
        R, C = dx.numel() // dx.shape[-1], dx.shape[-1]
        dx.copy_((src.float().reshape(R, C) * _unbits(bits, R, C)).reshape(dx.shape).to(dx.dtype))
        return conv_dgrad(dy, wt, dx, g, pooled, argmax, relu_mask, True, bn_bwd)
    if bn_bwd is not None:
        conv_dgrad(dy, wt, dx, g, pooled, argmax, relu_mask, accumulate)
        x, y, mean, invstd, gamma, beta, stats, act = bn_bwd
        bn_bwd_stats(dx, y, x, mean, invstd, stats, act, gamma=gamma, beta=beta)
        return dx
    if accumulate:
        old = dx.float().clone()
        conv_dgrad(dy, wt, dx, g, pooled, argmax, relu_mask)
        dx.copy_((dx.float() + old).to(dx.dtype))
        return dx
    dyt = dy.float().view(g["B"], g["OH"], g["OW"], g["Cout"]).permute(0, 3, 1, 2)
    w = wt.float().view(g["C"], g["KH"], g["KW"], g["Cout"]).permute(3, 0, 1, 2)
    dxt = torch.nn.grad.conv2d_input((g["B"], g["C"], g["H"], g["W"]), w, dyt, stride=g["stride"], padding=g["pad"])
    flat = dxt.permute(0, 2, 3, 1).reshape(-1)
    if pooled is not None:
        _unpool_ref(flat, pooled, argmax, g["H"], g["W"], g["C"], dx)
    else:
        if relu_mask is not None:
            flat = flat * (relu_mask.reshape(-1).float() > 0)
        dx.view(-1)[:] = flat.to(dx.dtype)
    return dx


def conv_wgrad(dz, x, dw, db, g, scale=1.0):
    """dW[Cout][KH][KW][C] += scale * sum dz (x) im2col(x);  db += scale * sum dz."""
    if dw.is_cuda:
        require().conv_wgrad(dz, x, dw, db, *_conv_geom_args(g), scale)
        return dw
    xt = x.float().view(g["B"], g["H"], g["W"], g["C"]).permute(0, 3, 1, 2)
    dzt = dz.float().view(g["B"], g["OH"], g["OW"], g["Cout"]).permute(0, 3, 1, 2)
    gw = torch.nn.grad.conv2d_weight(xt, (g["Cout"], g["C"], g["KH"], g["KW"]), dzt, stride=g["stride"],
                                     padding=g["pad"])
    dw.view(-1)[:] += scale * gw.permute(0, 2, 3, 1).reshape(-1)
    if db is not None:
        db += scale * dzt.sum(dim=(0, 2, 3))
    return dw


def conv1_wgrad_pooled_f32(dp, argmax, x, dw, db, g, scale=1.0, dy=None):
    """MNIST conv1 weight gradient at fp32 (C = 1, 32 channels, 3x3 / 5x5 SAME, stride 1) from the
    POOLED gradient dp [B][H/2][W/2][32] (ReLU mask applied) and the pool's argmax bytes:
    dW += scale * sum_q dp[q][n] * x[argmax pixel of q + tap], db += scale * sum dp - the gradient of
    un-pool + conv_wgrad without the un-pooled tensor (GPU: conv1_wgrad_pooled_f32_kernel).  Other
    shapes, and the CPU oracle: un-pool into ``dy`` [B][H][W][32] (allocated if None) + conv_wgrad."""
    B, H, W, K = g["B"], g["H"], g["W"], g["KH"]
    if dw.is_cuda:
        ws = wgrad_workspace(dw.device, B * (32 * 25 + 32))
        if require().conv1_wgrad_pooled_f32(dp, argmax, x, dw, db, ws, B, H, W, K, scale):
            return dw
    if dy is None:
        dy = torch.empty(B, H, W, dp.shape[-1], device=dp.device, dtype=torch.float32)
    unpool_f32(dp, argmax, dy)
    return conv_wgrad(dy, x, dw, db, g, scale)


def unpool_f32(g, argmax, out):
    """out[B][2PH][2PW][C] (fp32) = g routed to the argmax position of each 2x2 window, zeros
    elsewhere (the max-pool gradient; the ReLU mask is already in g)."""
    B, PH, PW, C = g.shape
    if g.is_cuda:
        require().unpool_f32(g, argmax, out, B, PH, PW, C)
        return out
    _unpool_ref(g.reshape(-1).float(), torch.ones(B, PH, PW, C), argmax, PH, PW, C, out)
    return out


def transpose_taps_f32(w, out, O, T, C):
    """out[C][T][O] = w[O][T][C] (a conv weight laid out for its data gradient)."""
    if w.is_cuda:
        require().transpose_taps_f32(w, out, O, T, C)
        return out
    out.view(-1)[:] = w.reshape(O, T, C).permute(2, 1, 0).reshape(-1)
    return out


# -------------------------------------------------------------------- head
def head_xent_f32(h, w, b, labels, dz, dl, loss_sum, correct, logits=None, scale=1.0, inv_keep=1.0,
                  step_counter=None) -> bool:
    """fp32 fused classifier head (GPU, NC = 10, K = 1024): logits (optional), softmax-xent sums into
    loss_sum / correct, dlogit rows fp32 [B][NC] into ``dl``, dZ = (dlogit . W) * inv_keep * (h > 0),
    step_counter += 1 - one launch.  False (nothing done): CPU tensors or another shape - the caller
    runs the GEMM + softmax_xent + GEMM chain, which is also this kernel's oracle."""
    if not h.is_cuda:
        return False
    return bool(require().head_xent_f32(h, w, b, labels, dz, dl, loss_sum, correct, logits, scale, inv_keep,
                                        step_counter))


def head_xent(h, w, b, labels, dz, dl, loss_sum, correct, logits=None, scale=1.0, inv_keep=1.0, step_counter=None,
              parts=None):
    """Per-row classifier head: logits, softmax-xent (loss/correct sums), dlogit rows (bf16 [B][ld] into
    ``dl``) and dZ = (dlogit . W) * inv_keep * (h > 0).  dW/db come from a wgrad GEMM over ``dl``.
    ``step_counter`` (int64 [1], optional) is advanced by one.  ``parts`` (fp32 [>= 2 * ceil(B/4)],
    optional): the loss / hit sums of each 4-row workgroup are stored there instead of being added
    to ``loss_sum`` / ``correct``; ``head_wgrad(..., parts=...)`` folds them in (no atomics)."""
    if h.is_cuda:
        require().head_xent(h, w, b, labels, dz, dl, loss_sum, correct, logits, scale, inv_keep, step_counter, parts)
        return
    if step_counter is not None:
        step_counter += 1
    hf, wf = h.float(), w.float()
    lg = hf @ wf.t() + (b.float() if b is not None else 0)
    if logits is not None:
        logits.copy_(lg)
    lse = torch.logsumexp(lg, dim=1)
    lab = labels.long()
    rows = lse - lg.gather(1, lab[:, None])[:, 0]
    hits = (lg.argmax(1) == lab).float()
    if parts is not None:
        n = (len(lab) + 3) // 4
        pad = 4 * n - len(lab)
        parts[:n] = torch.nn.functional.pad(rows, (0, pad)).view(n, 4).sum(1)
        parts[n:2 * n] = torch.nn.functional.pad(hits, (0, pad)).view(n, 4).sum(1)
    else:
        if loss_sum is not None:
            loss_sum += rows.sum()
        if correct is not None:
            correct += hits.sum().to(correct.dtype)
    p = torch.softmax(lg, dim=1)
    p[torch.arange(len(lab)), lab] -= 1
    d = p * scale
    dl.zero_()
    dl[:, : d.shape[1]] = d.to(dl.dtype)
    g = (d @ wf) * (hf > 0).float() * inv_keep
    dz.copy_(g.to(dz.dtype))


def head_wgrad(dl, h, dw, db, nc, scale=1.0, parts=None, loss_sum=None, correct=None, group=None):
    """Classifier-head weight / bias gradient, stored: dw[c][:K] = scale * sum_b dl[b][c] h[b][:],
    db[c] = scale * sum_b dl[b][c] (one workgroup per 8 columns over the whole batch, fixed order).
    ``parts``: head_xent's per-workgroup loss / hit partials, summed by the bias workgroup into
    ``loss_sum`` / ``correct`` (needs ``db``).  ``group``: a ``gemm_group`` to join (as ``gemm``)."""
    if h.is_cuda:
        require().head_wgrad(dl, h, dw, db, nc, scale, parts, loss_sum, correct, group)
        return
    d = dl[:, :nc].float()
    dw[:, : h.shape[1]] = (scale * (d.t() @ h.float())).to(dw.dtype)
    if db is not None:
        db.copy_((scale * d.sum(0)).to(db.dtype))
    if parts is not None:
        n = (h.shape[0] + 3) // 4
        loss_sum += parts[:n].sum()
        correct += parts[n:2 * n].sum().to(correct.dtype)


@contextlib.contextmanager
def gemm_group(anchor):
    """Grouped launch: yields a group; the ``gemm`` / ``head_wgrad`` calls that pass it as ``group=``
    join it (glds tile 12 or 22, bf16, one split; fp32 small tile; a head weight gradient - a call
    that does not fit launches at once, as do all calls without ``group=``) and leave as ONE kernel
    launch when the block ends: the head weight gradient, then the (KMAJ, RMAJ) and (RMAJ, RMAJ)
    GEMMs (any other mix launches one by one, in the order added); of the small-tile GEMMs (the
    GAN / autoencoder layers) a (RMAJ, RMAJ) weight gradient and a (KMAJ, KMAJ) data gradient as
    one paired launch.  A block that raises launches none of its group (the calls that did not
    join have run).  The group holds its pieces' tensors until then.
    CPU tensors (``anchor``): yields None, the ops run eagerly."""
    if not anchor.is_cuda:
        yield None
        return
    require()
    grp = torch.classes.dtfe.GemmGroup()
    try:
        yield grp
    except BaseException:
        grp.clear()
        raise
    grp.launch()


# --------------------------------------------------------------- optimizer
def opt_state(kind, p, segs, work, done, s1=None, s2=None, beta1=0.0, beta2=0.0, eps=0.0, momentum=0.0, rho=0.0,
              beta_pow=None, global_step=None, wd=None, sched=None, lr_out=None, nesterov=False, decay=False,
              ema=None, ema_decay=0.0, ema_num_updates=False, ema_out=None, seg_lr=None):
    """An optimizer bound to the native side (torch.classes.dtfe.OptState): everything that holds for its
    life, checked once - the tensors' device, dtype and length, every segment inside ``p``, every work item
    inside its segment - with the plan packed into a device blob.  apply_gradients then takes only what varies.
    ``segs``: rows (off, R, T, C, w16 address, wt16 address); ``work``: rows (kind, seg, t, r0, c0, start,
    count); ``wd``: the coupled L2 weight decay of each segment (nseg floats; None = none) - sequences or CPU
    tensors.  ``done``: the zeroed 4-byte counter the kernel's workgroups count themselves on.
    ``sched``: the blob of lr_schedule_pack - the kernel evaluates it at ``global_step`` and uses the result
    in place of the launch's ``lr``; ``lr_out``: a device float32 scalar that receives the rate a launch used.
    ``nesterov``: TF1 ApplyMomentum's use_nesterov form (momentum only).  ``decay``: launch the kernels'
    weight-decay instantiation (some ``wd`` is non-zero); without it ``wd`` is ignored.
    ``ema``: the shadow buffer of an exponential moving average (float32, as long as ``p``, same offsets):
    every launch also updates it from the values it stores, with ``ema_decay`` or - ``ema_num_updates`` -
    ``min(ema_decay, (1 + n) / (10 + n))`` at the global step after the launch's advance (ema_decay_value);
    ``ema_out``: a device float32 scalar that receives the decay a launch used.  ema_swap exchanges the two.
    ``seg_lr``: a device float32 vector, one factor per segment (momentum only): a launch's rate for a segment's
    elements is its rate times ``seg_lr[seg]`` as it stands when the launch runs (layer_trust's ``trust``)."""
    require()
    table = lambda t, cols: torch.as_tensor(t, dtype=torch.int64).reshape(len(t), cols)
    if wd is not None:
        wd = torch.as_tensor(wd, dtype=torch.float32)
    return torch.classes.dtfe.OptState(int(kind), p, s1, s2, beta1, beta2, eps, momentum, rho, beta_pow, global_step,
                                       done, table(segs, 6), table(work, 7), wd, sched, lr_out, bool(nesterov),
                                       bool(decay), ema, float(ema_decay), bool(ema_num_updates), ema_out, seg_lr)


@functools.lru_cache(None)
def _direct(name):
    """The library's op ``name`` without torch.ops' Python wrapper: for an op that takes a custom class the
    wrapper walks every argument of every call (a pytree scan for fake script objects, about 10 us - more
    than the rest of an eager apply launch's host cost) before it enters the dispatcher.  Converting the
    object argument costs about as much again; a method of the object pays neither."""
    op = getattr(require(), name)
    return getattr(op.default, "_op", op)


def apply_gradients(state, g, g16, gscale, lr, gs_inc, wait_done=None, wait_seen=None, wait_segs=0, clip_scale=None):
    """One launch of an ``opt_state``: exactly one of ``g`` (float32) / ``g16`` (bfloat16), contiguous, on the
    state's GPU and at least as long as its ``p``; ``lr`` is read per launch.
    The launch's items of the var-list segments in bit mask ``wait_segs`` wait (on the device) until
    ``wait_done`` exceeds ``wait_seen`` - a gradient produced on another stream that signals with
    epoch_signal(wait_done) instead of a stream join; the launch's last workgroup advances ``wait_seen``.
    ``clip_scale``: a device float32 scalar multiplied into ``gscale`` by the kernel (grad_sumsq's scale)."""
    # (the op torch.ops.dtfe.apply_gradients(state, ...) as the state's method: the cheaper call, see _direct)
    state.apply(g, g16, gscale, lr, gs_inc, wait_done, wait_seen, wait_segs, clip_scale)


def apply_gradients_group(states, g, g16, gscale, lrs, gs_incs, clip_scales=None):
    """Up to four ``opt_state`` of one kind (and none with a schedule or an EMA) over disjoint var lists in ONE launch,
    each with its own rate, step increment and (``clip_scales``: a list with None where there is none) clip scale."""
    _direct("apply_gradients_group")(states, g, g16, gscale, lrs, gs_incs, clip_scales)


def ema_swap(state):
    """Exchange the masters of an ``opt_state``'s var list with their EMA shadows and rewrite the bf16 working
    copies (natural and transposed) from the new masters - one launch over the optimizer's plan; slots, step
    and counters are untouched, and a second swap restores every buffer bit for bit.  Capturable."""
    state.ema_swap()


def ema_decay_value(decay, num_updates, n):
    """The decay an apply uses, as numpy float32: the host mirror of the kernel's ema_decay_eval.  Without
    ``num_updates`` it is ``decay``; with it, ``min(decay, (1 + n) / (10 + n))`` where ``n`` is the global step
    AFTER the apply's advance (tf.train.ExponentialMovingAverage(decay, num_updates=global_step), run after
    minimize).  One float32 division, IEEE-rounded on both sides: the two agree bit for bit."""
    f = np.float32
    d = f(decay)
    if not num_updates:
        return d
    n = int(n)
    r = f(f(1 + n) / f(10 + n))
    return r if r < d else d


def ema_update_ref(shadow, value, d):
    """One EMA update of numpy float32 arrays, the host mirror of the kernel's ema_update (TF1
    assign_moving_average): ``shadow - (shadow - value) * (1 - d)``, every operation rounded once."""
    f = np.float32
    shadow, value = np.asarray(shadow, dtype=f), np.asarray(value, dtype=f)
    omd = f(f(1) - f(d))
    with np.errstate(all="ignore"):
        return (shadow - ((shadow - value) * omd).astype(f)).astype(f)


# learning-rate schedules (csrc/kernels/optim.h LrSchedule / lr_schedule_eval)
LR_CONSTANT, LR_PIECEWISE, LR_LINEAR = 0, 1, 2
LR_MAX_BOUNDS = 8


def lr_schedule_spec(lr=0.0, boundaries=(), values=(), decay_steps=0, end=0.0, warmup_steps=0):
    """The validated description of a schedule, as a dict of float32 / int fields:
    ``boundaries`` / ``values`` - tf.train.piecewise_constant (``values[i]`` while
    ``boundaries[i-1] < step <= boundaries[i]``, the last value beyond); ``decay_steps`` / ``end`` -
    tf.train.polynomial_decay with power 1 and no cycling, from ``lr`` to ``end``; neither - the constant
    ``lr``.  ``warmup_steps`` W multiplies the rate by ``(step + 1) / W`` while ``step < W``.
    The reciprocals are rounded to float32 here, once: kernel and mirror multiply by the same value."""
    f = np.float32
    boundaries, values = [int(b) for b in boundaries], [float(v) for v in values]
    decay_steps, warmup_steps = int(decay_steps or 0), int(warmup_steps or 0)
    if (boundaries or values) and decay_steps:
        raise ValueError("lr schedule: piecewise-constant (boundaries/values) and linear decay (decay_steps) "
                         "are mutually exclusive")
    if boundaries or values:
        if len(values) != len(boundaries) + 1:
            raise ValueError("lr schedule: %d boundaries need %d values, got %d"
                             % (len(boundaries), len(boundaries) + 1, len(values)))
        if not 1 <= len(boundaries) <= LR_MAX_BOUNDS:
            raise ValueError("lr schedule: 1 to %d boundaries, got %d" % (LR_MAX_BOUNDS, len(boundaries)))
        if any(b < 0 or b >= 2 ** 31 for b in boundaries) or any(y <= x for x, y in zip(boundaries, boundaries[1:])):
            raise ValueError("lr schedule: boundaries must be strictly increasing steps, got %r" % (boundaries,))
        kind = LR_PIECEWISE
    elif decay_steps:
        if not 1 <= decay_steps < 2 ** 31:
            raise ValueError("lr schedule: decay_steps must be >= 1, got %r" % (decay_steps,))
        kind = LR_LINEAR
    else:
        kind = LR_CONSTANT
    if not 0 <= warmup_steps < 2 ** 31:
        raise ValueError("lr schedule: warmup_steps must be >= 0, got %r" % (warmup_steps,))
    return {"kind": kind, "bounds": boundaries, "values": [f(v) for v in values], "lr": f(lr), "end": f(end),
            "decay_steps": decay_steps, "inv_decay": f(1) / f(decay_steps) if decay_steps else f(0),
            "warmup": warmup_steps, "inv_warmup": f(1) / f(warmup_steps) if warmup_steps else f(0)}


def lr_schedule_value(spec, step):
    """The rate at ``step`` as numpy float32: the host mirror of the kernel's lr_schedule_eval, operation
    for operation (integer compares; fp32 +, -, *, each rounded once), so the two agree bit for bit."""
    f = np.float32
    step = int(step)
    v = spec["lr"]
    if spec["kind"] == LR_PIECEWISE:
        i = 0
        while i < len(spec["bounds"]) and step > spec["bounds"][i]:
            i += 1
        v = spec["values"][i]
    elif spec["kind"] == LR_LINEAR:
        t = f(min(step, spec["decay_steps"]))
        v = f(f(spec["lr"] - spec["end"]) * f(f(1) - f(t * spec["inv_decay"]))) + spec["end"]
    if step < spec["warmup"]:
        v = f(v * f(f(step + 1) * spec["inv_warmup"]))
    return f(v)


def lr_schedule_pack(spec, device_like):
    """The device struct (a uint8 blob) of a lr_schedule_spec, for opt_state's ``sched``."""
    return require().lr_schedule_pack(spec["kind"], spec["bounds"], [float(v) for v in spec["values"]],
                                      float(spec["lr"]), float(spec["end"]), spec["decay_steps"],
                                      float(spec["inv_decay"]), spec["warmup"], float(spec["inv_warmup"]), device_like)


GRAD_CHUNK_MAX = 8192  # csrc/kernels/gradnorm.h


def grad_norm_plan(segs, master):
    """The (offset, count) chunk table of a global gradient norm: ``segs`` = [(offset, numel)] of a var
    list's variables in the flat buffer of ``master``, cut into chunks of at most GRAD_CHUNK_MAX elements
    (a transposed variable is a flat range like any other).  The chunks cover exactly those elements:
    no padding, no variable outside the list.  int64 [nchunk, 2] on master's device."""
    rows = []
    for off, n in segs:
        off, n = int(off), int(n)
        if off < 0 or n < 0 or off + n > master.numel():
            raise ValueError("grad_norm_plan: segment (%d, %d) outside a buffer of %d" % (off, n, master.numel()))
        rows += [[off + st, min(GRAD_CHUNK_MAX, n - st)] for st in range(0, n, GRAD_CHUNK_MAX)]
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2).to(master.device)


def _plan_cat(t, plan):
    rows = plan.tolist()
    return torch.cat([t[o:o + n] for o, n in rows]) if rows else t[:0]


def grad_sumsq(g, g16, gscale, clip_norm, plan, partials, ticket, out, max_blocks=0):
    """out[0] = sqrt(sum over the plan of (gscale * g)^2), out[1] = clip_norm / max(out[0], clip_norm) (the
    factor of tf.clip_by_global_norm; 1 when the norm is within clip_norm).  Exactly one of ``g`` (fp32) /
    ``g16`` (bf16).  GPU: one launch, bitwise reproducible whatever the grid (``max_blocks`` caps it, for
    tests); ``partials`` (fp32, one per chunk) and ``ticket`` (zeroed int32) are its scratch."""
    if out.is_cuda:
        require().grad_sumsq(g, g16, gscale, clip_norm, plan, partials, ticket, out, max_blocks)
        return
    x = _plan_cat(g if g is not None else g16, plan).double() * float(np.float32(gscale))
    norm = np.float32(math.sqrt(float((x * x).sum())))
    c = np.float32(clip_norm)
    out[0] = float(norm)
    out[1] = float(c / norm) if c > 0 and norm > c else 1.0


def scale_(t, scale, plan):
    """t[i] *= scale[0] (a device scalar) over the chunks of ``plan`` (grad_norm_plan), in place."""
    if t.is_cuda:
        require().scale_(t, scale, plan)
        return
    for o, n in plan.tolist():
        t[o:o + n] *= scale[0]


LARS_CHUNK_MAX = 8192  # csrc/kernels/lars.h


def layer_trust_plan(segs, master, chunk=0):
    """The tables of a layer_trust launch.  ``segs`` = [(seg, offset, numel)] of the adaptive variables in the
    flat buffer of ``master`` (seg: the variable's index in the optimizer's var list), cut into chunks of at
    most ``chunk`` elements (0: LARS_CHUNK_MAX; a multiple of 1024 up to it).  The largest chunk is the
    measured choice at both ends (profiles/lars_apply.txt): ResNet-20's 0.27 M elements make only 35 workgroups
    of it, yet 2048- and 1024-element chunks - 4 and 8 times the workgroups - ran 1.1 and 1.4 times as long,
    every further workgroup costing a ticket and a partial more than its share of the read saves; at
    ResNet-50's 25.5 M they ran 2.0 and 3.4 times as long.
    The chunks cover exactly those elements: no padding, no other variable.  Returns (plan, ranges, limit):
    plan int64 [nchunk, 3] rows (seg, offset, count), ranges int32 [nadapt, 3] rows (seg, first chunk,
    chunks) - both on master's device - and limit, the end of the last element the plan reads."""
    if not chunk:
        chunk = LARS_CHUNK_MAX
    if chunk < 1024 or chunk > LARS_CHUNK_MAX or chunk % 1024:
        raise ValueError("layer_trust_plan: chunk is a multiple of 1024 up to %d, got %r" % (LARS_CHUNK_MAX, chunk))
    rows, ranges, limit, seen = [], [], 0, set()
    for seg, off, n in segs:
        seg, off, n = int(seg), int(off), int(n)
        if off < 0 or n < 1 or off + n > master.numel():
            raise ValueError("layer_trust_plan: segment (%d, %d) outside a buffer of %d" % (off, n, master.numel()))
        if seg < 0 or seg >= 2 ** 31 or seg in seen:
            raise ValueError("layer_trust_plan: segment index %d is negative or listed twice" % seg)
        seen.add(seg)
        first = len(rows)
        rows += [[seg, off + st, min(chunk, n - st)] for st in range(0, n, chunk)]
        ranges.append([seg, first, len(rows) - first])
        limit = max(limit, off + n)
    if len(rows) >= 2 ** 31:
        raise ValueError("layer_trust_plan: too many chunks")
    return (torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(master.device),
            torch.tensor(ranges, dtype=torch.int32).reshape(-1, 3).to(master.device), limit)


def lars_trust_ref(sum_w, sum_g, eeta, wd, eps, clip_scale=None):
    """The trust ratio of one variable as numpy float32 from its two sums of squares: the host mirror of the
    kernel's lars_trust_eval (tf.contrib.opt.LARSOptimizer.compute_lr), operation for operation -
    ``eeta * |w| / (|g| + wd * |w| + eps)`` when both norms are positive, else 1; ``clip_scale`` (a global-norm
    clip's factor) multiplies ``|g|`` first.  One IEEE square root per norm and one IEEE division, every
    other operation rounded once: the two agree bit for bit."""
    f = np.float32
    with np.errstate(all="ignore"):
        wn, gn = np.sqrt(f(sum_w)), np.sqrt(f(sum_g))
        if clip_scale is not None:
            gn = f(gn * f(clip_scale))
        if not (wn > 0 and gn > 0):
            return f(1)
        return f(f(f(eeta) * wn) / f(f(gn + f(f(wd) * wn)) + f(eps)))


def layer_trust(p, g, g16, gscale, plan, ranges, limit, wd, eeta, eps, clip_scale, partials, ticket, sums, trust,
                max_blocks=0):
    """LARS: for every adaptive variable (``plan`` / ``ranges`` / ``limit``: layer_trust_plan) ``sums[seg]`` =
    (sum of p^2 over the fp32 master, sum of (gscale * g)^2) and ``trust[seg]`` = lars_trust_ref of the two
    with ``wd[seg]``; the other entries of ``sums`` and ``trust`` are not written.  Exactly one of ``g``
    (fp32) / ``g16`` (bf16).  GPU: one launch, bitwise reproducible whatever the grid (``max_blocks`` caps it,
    for tests); ``partials`` (fp32, two per chunk) and ``ticket`` (zeroed int32) are its scratch.  CPU: float32
    sums, the same mirror."""
    if p.is_cuda:
        require().layer_trust(p, g, g16, gscale, plan, ranges, limit, wd, eeta, eps, clip_scale, partials, ticket,
                              sums, trust, max_blocks)
        return
    f = np.float32
    x = g if g is not None else g16.float()
    rows = plan.tolist()
    clip = None if clip_scale is None else float(clip_scale[0])
    for seg, first, n in ranges.tolist():
        idx = torch.cat([torch.arange(o, o + c) for _s, o, c in rows[first:first + n]])
        sw = (p[idx] * p[idx]).sum(dtype=torch.float32)
        gs = x[idx] * float(f(gscale))
        sg = (gs * gs).sum(dtype=torch.float32)
        sums.view(-1)[2 * seg], sums.view(-1)[2 * seg + 1] = float(sw), float(sg)
        trust[seg] = float(lars_trust_ref(f(sw), f(sg), eeta, f(wd[seg]), eps, clip))


# the words of an evaluation state (csrc/kernels/eval.h EvalState): int64, the last one a float64's bits
EVAL_CURSOR, EVAL_N, EVAL_COUNT, EVAL_HITS1, EVAL_HITSK, EVAL_BAD, EVAL_LOSS = range(7)
EVAL_STATE_WORDS = 7


def eval_state(device, n=0):
    """A zeroed evaluation state for a pass over ``n`` examples: int64 [EVAL_STATE_WORDS] on ``device``."""
    st = torch.zeros(EVAL_STATE_WORDS, dtype=torch.int64)
    st[EVAL_N] = int(n)
    return st.to(device)


def eval_state_dict(state) -> dict:
    """The state's words as Python numbers (one device-to-host copy)."""
    w = state.cpu()
    out = {k: int(w[i]) for i, k in enumerate(("cursor", "n", "count", "hits1", "hitsk", "bad_labels"))}
    out["loss_sum"] = float(w[EVAL_LOSS:EVAL_LOSS + 1].view(torch.float64)[0])
    return out


def eval_rows_ref(z, t, k):
    """eval_metrics' per-row results on the host, float32 numpy: (loss, hit1, hitk, bad) of logits ``z``
    [R][NC] and labels ``t`` [R].  rank = #{j: z[j] > z[t]} + #{j < t: z[j] == z[t]}; hit1 = rank == 0,
    hitk = rank < k, both False for a NaN target or a label outside [0, NC) (``bad``).  loss =
    (max + log(sum(exp(z - max)))) - z[t] in float32, exp and log rounded once from float64."""
    z = np.asarray(z, dtype=np.float32)
    t = np.asarray(t).astype(np.int64)
    R, NC = z.shape
    bad = (t < 0) | (t >= NC)
    tc = np.where(bad, 0, t)
    zt = np.where(bad, np.float32(0), z[np.arange(R), tc]).astype(np.float32)
    j = np.arange(NC).reshape(1, NC)
    with np.errstate(invalid="ignore", over="ignore"):
        rank = ((z > zt[:, None]) | ((z == zt[:, None]) & (j < t[:, None]))).sum(1)
        ranked = ~bad & ~np.isnan(zt)
        mx = np.fmax.reduce(z, axis=1, initial=-np.inf).astype(np.float32)
        e = np.exp((z - mx[:, None]).astype(np.float32).astype(np.float64)).astype(np.float32)
        se = e.sum(1, dtype=np.float32)
        lse = (mx + np.log(se.astype(np.float64)).astype(np.float32)).astype(np.float32)
        loss = (lse - zt).astype(np.float32)
    return loss, ranked & (rank == 0), ranked & (rank < k), bad


def eval_metrics(logits, labels, k, state, idx=None, ws=None, ticket=None):
    """One chunk of an evaluation pass whose totals live in ``state`` (eval_state): with B = logits.shape[0]
    and valid = clamp(n - cursor * B, 0, B), rows [0, valid) of fp32 ``logits`` [B][NC] and int32 ``labels``
    [B] are scored (eval_rows_ref) and added - count, top-1 hits, top-``k`` hits, bad labels, and the losses
    in row order in float64 - then the cursor advances and ``idx`` (int32 [B], optional) receives the next
    chunk's rows min(cursor * B + b, n - 1).  Rows from ``valid`` on may hold anything; valid == 0 changes
    nothing.  GPU: one launch, no host sync, bitwise reproducible; ``ws`` (int32 [2B]) and ``ticket``
    (zeroed int32) are its scratch."""
    B, NC = logits.shape
    if not 1 <= int(k) <= NC:
        raise ValueError("eval_metrics: 1 <= k <= NC, got k = %d for %d classes" % (k, NC))
    if logits.is_cuda:
        require().eval_metrics(logits, labels, int(k), state, idx, ws, ticket)
        return
    cursor, n = int(state[EVAL_CURSOR]), int(state[EVAL_N])
    valid = max(0, min(B, n - cursor * B))
    if valid == 0:
        return
    loss, hit1, hitk, bad = eval_rows_ref(logits[:valid].numpy(), labels[:valid].numpy(), int(k))
    state[EVAL_COUNT] += valid
    state[EVAL_HITS1] += int(hit1.sum())
    state[EVAL_HITSK] += int(hitk.sum())
    state[EVAL_BAD] += int(bad.sum())
    acc = state[EVAL_LOSS:EVAL_LOSS + 1].view(torch.float64)
    s = np.float64(acc[0].item())
    for v in loss[~bad]:  # in row order, one float64 add per row: the kernel's fold
        s = s + np.float64(v)
    acc[0] = float(s)
    state[EVAL_CURSOR] = cursor + 1
    if idx is not None:
        idx[:B] = torch.arange((cursor + 1) * B, (cursor + 2) * B).clamp_max(n - 1).to(idx.dtype)


# ------------------------------------------------------------- elementwise
def tallk_ws_floats(M: int, N: int, splits: int) -> int:
    """Partial-slab floats of wgrad_tallk (mirrors tallk_ws_floats in csrc/kernels/wgrad_tallk.hip)."""
    return splits * ((M + 1 + 15) // 16 * 16) * N


def wgrad_tallk(A, lda, B, ldb, M, N, K, out, ldc=None, bias=None, splits=32, scale=1.0, workspace=None):
    """Exact-fp32 weight gradient of a long reduction: out[m][n] = scale * sum_k A[k*lda+m] B[k*ldb+n]
    (stored), bias[n] = scale * sum_k B[k*ldb+n] (the LSTM kernel / bias gradient over T*B rows).
    GPU: K split over `splits` workgroups per 64-column slab + a fixed-order partial reduce."""
    ldc = N if ldc is None else ldc
    if out.is_cuda:
        ws = workspace if workspace is not None else wgrad_workspace(out.device, tallk_ws_floats(M, N, splits))
        require().wgrad_tallk(A, lda, B, ldb, M, N, K, out, ldc, bias, ws, splits, scale)
        return out
    a = torch.as_strided(A.reshape(-1), (K, M), (lda, 1)).double()
    b = torch.as_strided(B.reshape(-1), (K, N), (ldb, 1)).double()
    torch.as_strided(out.view(-1), (M, N), (ldc, 1)).copy_((scale * (a.t() @ b)).float())
    if bias is not None:
        bias.copy_((scale * b.sum(0)).float())
    return out


def seq_stage(x, xh, T, I, y_src, y_dst, zero=()):
    """LSTM batch staging (one launch on the GPU): xh[t, b, :I] = x[b, t*I:(t+1)*I] (image row t
    is timestep t), xh[0, :, I:] = 0 (h_{-1}), y_dst = y_src, and the tensors in ``zero`` (up to 4
    accumulators) cleared."""
    if xh.is_cuda:
        require().seq_stage(x.reshape(-1).contiguous(), xh, int(T), int(I), y_src.reshape(-1).contiguous(),
                            y_dst, list(zero))
        return
    B = xh.shape[1]
    xh[:, :, :I].copy_(x.reshape(B, T, I).transpose(0, 1))
    xh[0, :, I:].zero_()
    y_dst.copy_(y_src.reshape(y_dst.shape))
    for z in zero:
        z.zero_()


def gather_rows(src, dst, idx=None, labels_src=None, labels_dst=None, seed=0, counter=None, done=None, zero=(),
                onehot=None, shuffle=False):
    """dst[b] = src[row(b)] (+ labels); ``zero``: up to 4 contiguous tensors cleared in the same
    launch (a step's accumulators), saving one fill kernel each; ``onehot``: f32 [B][ncls] one-hot
    rows of the gathered labels, also written in the same launch.  ``idx`` None samples the rows at
    counter value s: with replacement, hash_u32(seed, s * B + b) % n_rows, or with ``shuffle=True`` one
    permutation of the rows per epoch, shuffled_rows(seed, s, B, n_rows)."""
    if shuffle and idx is not None:
        raise ValueError("gather_rows: shuffle=True samples the rows itself, it takes no idx")
    if dst.is_cuda:
        require().gather_rows(src, dst, idx, labels_src, labels_dst, seed, counter, done, list(zero), onehot,
                              bool(shuffle))
        return dst
    for z in zero:
        z.zero_()
    if idx is None:  # the kernel's on-device sampling, from the host mirror
        s = int(counter.reshape(-1)[0].item()) if counter is not None else 0
        idx = _sampled_rows(seed, s, dst.shape[0], src.shape[0], shuffle)
        if counter is not None and done is not None:  # the kernel's ticket needs both
            counter += 1
    if onehot is not None:
        onehot.zero_()
        onehot.scatter_(1, labels_src[idx.long()].long().unsqueeze(1), 1.0)
    rows = src[idx.long()]
    if src.dtype == torch.uint8:
        rows = rows.float() / 255.0
    dst.copy_(rows.reshape(dst.shape).to(dst.dtype))
    if labels_dst is not None:
        labels_dst.copy_(labels_src[idx.long()])
    return dst


def _augment_check(src, dst, H, W, C, pad, mean, inv_std):
    """The argument checks of torch.ops.dtfe.augment_rows, as ValueError on either device."""
    H, W, C, pad = int(H), int(W), int(C), int(pad)
    if src.dtype not in (torch.uint8, torch.float32) or dst.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("augment_rows: src must be uint8 or f32, dst f32 or bf16 (got %s -> %s)" % (src.dtype, dst.dtype))
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("augment_rows: src and dst must be contiguous")
    if src.device != dst.device:
        raise ValueError("augment_rows: src on %s, dst on %s" % (src.device, dst.device))
    if min(H, W, C) < 1 or src.dim() != 2 or src.shape[0] < 1 or src.shape[1] != H * W * C:
        raise ValueError("augment_rows: src %s is not [n_rows][H*W*C = %d]" % (tuple(src.shape), H * W * C))
    if dst.dim() < 1 or dst.shape[0] < 1 or dst.numel() != dst.shape[0] * H * W * C:
        raise ValueError("augment_rows: dst %s does not hold [B][%d][%d][%d]" % (tuple(dst.shape), H, W, C))
    if not (0 <= pad <= AUG_MAX_PAD and pad < min(H, W)):
        raise ValueError("augment_rows: pad %d: needs 0 <= pad <= %d and pad < min(H, W)" % (pad, AUG_MAX_PAD))
    if (mean is None) != (inv_std is None):
        raise ValueError("augment_rows: mean and inv_std come together")
    for t in (mean, inv_std):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous()
                              or t.device != dst.device):
            raise ValueError("augment_rows: mean / inv_std must be contiguous f32 [C = %d] on %s" % (C, dst.device))


def _mix_check(mix, label_smoothing, B, labels_src, onehot):
    """The mixing / smoothing argument checks of torch.ops.dtfe.augment_rows, as ValueError on either device."""
    if mix not in MIX_MODES:
        raise ValueError("augment_rows: mix is one of %s, not %r" % (", ".join(MIX_MODES), mix))
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError("augment_rows: label_smoothing must lie in [0, 1), got %r" % (label_smoothing,))
    if (mix != "none" or label_smoothing > 0) and (onehot is None or labels_src is None):
        raise ValueError("augment_rows: mix / label_smoothing write soft label rows: they need onehot and labels_src")
    if mix != "none" and B < 2:
        raise ValueError("augment_rows: mix=%r needs a batch of B >= 2, dst holds %d" % (mix, B))


def augment_rows(src, dst, H, W, C, pad=0, flip=False, mean=None, inv_std=None, idx=None, labels_src=None,
                 labels_dst=None, seed=0, counter=None, done=None, zero=(), onehot=None, shuffle=False, mix="none",
                 label_smoothing=0.0):
    """gather_rows for image rows [n_rows][H*W*C] (uint8 scaled by 1/255, or f32) -> dst [B][H][W][C]
    (f32 / bf16) with the input transforms in the same launch.  Sample b at counter value s draws
    (dy, dx, flipped) = augment_draws(seed, s, B, pad, flip)[b] and
        dst[b, y, x, c] = img(y + dy - pad, (W - 1 - x if flipped else x) + dx - pad, c)
    with img() = 0 outside the image (the border is zero AFTER standardisation: the mean colour) and
    (v - mean[c]) * inv_std[c] in fp32 inside it (``mean`` None: v).  Rows, labels, one-hot rows, zero
    ranges and the (seed, counter, done) ticket are gather_rows'; ``idx`` None samples the rows
    hash_u32(seed, s * B + b) % n_rows, or with ``shuffle=True`` shuffled_rows(seed, s, B, n_rows) (the
    draws do not depend on the mode).  pad = 0, flip off, no statistics: gather_rows bit for bit.

    ``label_smoothing`` E in [0, 1): the rows of ``onehot`` hold (on, off) = smoothing_values(E, ncls) instead
    of (1, 0).  ``mix`` "mixup" / "cutmix" (B >= 2): with d = mix_draws(seed, s, B, H, W) and A the batch as
    above, slot b is blended with slot d.partner[b] - mixup: fl(fl(lam * A[b]) + fl((1 - lam) * A[partner]));
    cutmix: A[partner] inside the slot's box of the output, A[b] outside - and its label row is
    fl(fl(w * t_b) + fl((1 - w) * t_partner)) with w = d.lam or d.lam_box: every product and sum rounded to
    float32 on its own.  ``labels_dst`` stays slot b's own label."""
    _augment_check(src, dst, H, W, C, pad, mean, inv_std)
    if shuffle and idx is not None:
        raise ValueError("augment_rows: shuffle=True samples the rows itself, it takes no idx")
    _mix_check(mix, label_smoothing, dst.shape[0], labels_src, onehot)
    H, W, C, pad = int(H), int(W), int(C), int(pad)
    if dst.is_cuda:
        require().augment_rows(src, dst, H, W, C, pad, bool(flip), mean, inv_std, idx, labels_src, labels_dst, seed,
                               counter, done, list(zero), onehot, bool(shuffle), MIX_MODES[mix], float(label_smoothing))
        return dst
    B = dst.shape[0]
    s = int(counter.reshape(-1)[0].item()) if counter is not None else 0
    if idx is not None:
        rows = idx.reshape(-1)[:B].long()
    else:
        rows = _sampled_rows(seed, s, B, src.shape[0], shuffle)
    dy, dx, fl = (torch.from_numpy(a) for a in augment_draws(seed, s, B, pad, flip))
    img = src[rows].reshape(B, H, W, C)
    if src.dtype == torch.uint8:  # the kernel's load: byte * (1.f / 255.f), one fp32 rounding
        img = img.float() * torch.tensor(float(np.float32(1.0) / np.float32(255.0)))
    if mean is not None:
        img = (img - mean.reshape(1, 1, 1, C)) * inv_std.reshape(1, 1, 1, C)
    ys = torch.arange(H).reshape(1, H) + (dy.reshape(B, 1) - pad)
    x = torch.arange(W).reshape(1, W)
    xs = torch.where(fl.reshape(B, 1), W - 1 - x, x) + (dx.reshape(B, 1) - pad)
    inside = ((ys >= 0) & (ys < H)).reshape(B, H, 1, 1) & ((xs >= 0) & (xs < W)).reshape(B, 1, W, 1)
    got = img[torch.arange(B).reshape(B, 1, 1), ys.clamp(0, H - 1).reshape(B, H, 1), xs.clamp(0, W - 1).reshape(B, 1, W)]
    out = torch.where(inside, got, torch.zeros((), dtype=got.dtype))
    if mix != "none":  # the partner's transformed image is slot partner[b]'s: nothing new is drawn for it
        d = mix_draws(seed, s, B, H, W)
        partner = torch.from_numpy(d.partner)
        if mix == "mixup":
            w = torch.from_numpy(d.lam)
            own, other = out * w.reshape(B, 1, 1, 1), out[partner] * (1.0 - w).reshape(B, 1, 1, 1)
            out = own + other  # three rounded operations, never addcmul / lerp
        else:
            w = torch.from_numpy(d.lam_box)
            y0, y1, x0, x1 = (torch.from_numpy(v).reshape(B, 1) for v in d.box)
            yy, xx = torch.arange(H).reshape(1, H), torch.arange(W).reshape(1, W)
            box = ((yy >= y0) & (yy < y1)).reshape(B, H, 1, 1) & ((xx >= x0) & (xx < x1)).reshape(B, 1, W, 1)
            out = torch.where(box, out[partner], out)
    dst.copy_(out.reshape(dst.shape).to(dst.dtype))
    if labels_dst is not None:
        labels_dst.copy_(labels_src[rows])
    if onehot is not None:
        on, off = smoothing_values(label_smoothing, onehot.shape[1])
        t = torch.full(onehot.shape, float(off))
        t.scatter_(1, labels_src[rows].long().unsqueeze(1), float(on))
        if mix != "none":
            own, other = t * w.reshape(B, 1), t[partner] * (1.0 - w).reshape(B, 1)
            t = own + other
        onehot.copy_(t)
    for z in zero:
        z.zero_()
    if counter is not None and done is not None:  # the kernel's ticket needs both
        counter += 1
    return dst


def uniform_fill(out, lo, hi, seed=0, counter=None, done=None, copy=None):
    """out ~ U(lo, hi) from the device hash RNG (advances ``counter``); ``copy=(src, dst)``: an fp32
    copy issued in the same launch (batch staging next to the noise)."""
    if out.is_cuda:
        src, dst = copy if copy is not None else (None, None)
        require().uniform_fill(out, lo, hi, seed, counter, done, src, dst)
        return out
    if copy is not None:
        copy[1].copy_(copy[0])
    out.uniform_(lo, hi)
    return out


def cast_(src, dst):
    if dst.is_cuda:
        require().cast_(src, dst)
    else:
        dst.copy_(src.to(dst.dtype))
    return dst


def softmax_xent(logits, labels_i=None, labels_oh=None, scale=1.0, dlogits=None, loss_rows=None, loss_sum=None,
                 correct=None, probs=None):
    if logits.is_cuda:
        require().softmax_xent(logits, labels_i, labels_oh, scale, dlogits, loss_rows, loss_sum, correct, probs)
        return
    y = labels_oh.float() if labels_oh is not None else \
        torch.nn.functional.one_hot(labels_i.long(), logits.shape[1]).float()
    lse = torch.logsumexp(logits, 1, keepdim=True)
    p = torch.exp(logits - lse)
    rows = (y * (lse - logits)).sum(1)
    if dlogits is not None:
        dlogits.copy_((p - y) * scale)
    if loss_rows is not None:
        loss_rows.copy_(rows)
    if loss_sum is not None:
        loss_sum += rows.sum()
    if correct is not None:
        correct += (logits.argmax(1) == y.argmax(1)).sum().to(correct.dtype)
    if probs is not None:
        probs.copy_(p)


def gan_loss(d_real, d_fake, gen_loss, disc_loss, dz_real_disc, dz_fake_disc, dz_fake_gen, clamp_eps=0.0):
    if d_real.is_cuda:
        require().gan_loss(d_real, d_fake, gen_loss, disc_loss, dz_real_disc, dz_fake_disc, dz_fake_gen, clamp_eps)
        return
    B = d_real.numel()
    pr, pf = d_real.view(-1), d_fake.view(-1)
    if clamp_eps > 0:
        lr_, lf, lq = torch.log(pr.clamp_min(clamp_eps)), torch.log(pf.clamp_min(clamp_eps)), \
            torch.log((1 - pf).clamp_min(clamp_eps))
    else:
        lr_, lf, lq = torch.log(pr), torch.log(pf), torch.log(1 - pf)
    gen_loss.fill_(-lf.mean().item())
    disc_loss.fill_(-(lr_ + lq).mean().item())
    dz_real_disc.view(-1).copy_(-(1 - pr) / B)
    dz_fake_disc.view(-1).copy_(pf / B)
    dz_fake_gen.view(-1).copy_(-(1 - pf) / B)


def epoch_signal(ctr):
    """ctr += 1 on the current stream (after the producer that a later apply_gradients(wait_done=ctr) waits for)."""
    require().epoch_signal(ctr)


def gan_head_ws_floats(B: int, DH: int) -> int:
    """Workspace floats of gan_disc_head (mirrors gan_head_ws_floats in csrc/kernels/head.hip)."""
    return max(1, min(256, (B + 3) // 4)) * 260 + 4


def gan_disc_head(d1, w, b, p, dlog, dlog_g, gw, gb, dd1, ddf, gen_loss, disc_loss, ws=None, clamp_eps=0.0) -> bool:
    """The GAN discriminator's output layer + both GAN losses + their gradients down to the hidden layer
    (csrc/kernels/head.h GanHeadArgs): d1 [2B][DH] (real rows, then fake rows), w = Wd2 [DH] (, b = bd2):
    p = sigmoid(d1 w + b) [2B], gen_loss / disc_loss (stored), dlog [2B], dlog_g [B], gw = dWd2 / gb = dbd2
    (stored), dd1 = dlog w^T relu'(d1) [2B][DH], ddf = dlog_g w^T relu'(d1_fake) [B][DH].  GPU: one launch
    (``ws``: gan_head_ws_floats zeroed floats, reused), returns False when the shape is not covered.  The CPU
    path is the fp32 oracle (the gemm + gan_loss chain it replaces)."""
    if d1.is_cuda:
        return bool(require().gan_disc_head(d1, w, b, p, dlog, dlog_g, gw, gb, dd1, ddf, gen_loss, disc_loss, ws,
                                            clamp_eps))
    B = d1.shape[0] // 2
    wv = w.reshape(-1)
    z = d1 @ wv + (b.reshape(()) if b is not None else 0.0)
    pp = torch.sigmoid(z)
    dl = torch.empty(2 * B, dtype=d1.dtype)
    dg = torch.empty(B, dtype=d1.dtype)
    gan_loss(pp[:B], pp[B:], gen_loss, disc_loss, dl[:B], dl[B:], dg, clamp_eps=clamp_eps)
    if p is not None:
        p.view(-1).copy_(pp)
    if dlog is not None:
        dlog.view(-1).copy_(dl)
    if dlog_g is not None:
        dlog_g.view(-1).copy_(dg)
    gw.view(-1).copy_(d1.t() @ dl)
    if gb is not None:
        gb.view(-1).copy_(dl.sum().reshape(1))
    mask = (d1 > 0).to(d1.dtype)
    dd1.copy_(dl[:, None] * wv[None, :] * mask)
    ddf.copy_(dg[:, None] * wv[None, :] * mask[B:])
    return True


MSE_WS_FLOATS = 132  # csrc/kernels/elementwise.h MSE_WS_FLOATS (128 partials + ticket)


def mse_sigmoid(y, t, loss, dz, ws=None):
    """loss = mean((y - t)^2), dz = d loss / d logit of y = sigmoid(logit).  ``ws`` (GPU, MSE_WS_FLOATS
    zeroed floats, reused every step): one launch whose last workgroup stores the loss (no memset node,
    bitwise-reproducible loss) instead of a memset + per-workgroup atomics."""
    if y.is_cuda:
        require().mse_sigmoid(y, t, loss, dz, ws)
        return
    n = y.numel()
    d = y - t
    loss.fill_((d * d).mean().item())
    dz.copy_(2 * d / n * y * (1 - y))


def dense_head(feat16, w, bias, y, logits, loss_sum, correct, dw, db, dfeat16, scale, w_fmajor=False,
               store=False, dl_out=None) -> bool:
    """A small dense classifier head, forward and backward in one launch (GPU: one workgroup; False when
    it does not fit): logits = feat W^T + b, softmax cross-entropy against one-hot y (loss_sum +=,
    correct +=), dlogits = (p - y) * scale, dw += dlogits^T feat, db += column sums, dfeat16 =
    dlogits W (in feat's dtype: bf16 or fp32).  ``w_fmajor``: W and dw are [F][NC] (a TF Variable of
    shape (in, out)) instead of [NC][F]; ``store``: dw / db are stored, not accumulated.  ``dl_out``
    (fp32 [B][NC]): the dlogits rows are written there, and dfeat16 may be None (the consumer forms it:
    lstm_seq_bwd(dl=...)).  The CPU path is the fp32 oracle."""
    if feat16.is_cuda:
        return bool(require().dense_head(feat16, w, bias, y, logits, loss_sum, correct, dw, db, dfeat16, scale,
                                         w_fmajor, store, dl_out))
    f = feat16.float()
    wf = w.float().t() if w_fmajor else w.float()   # [NC][F]
    lg = f @ wf.t() + (bias.float() if bias is not None else 0.0)
    if logits is not None:
        logits.copy_(lg)
    dl = torch.empty_like(lg)
    softmax_xent(lg, labels_oh=y, scale=scale, dlogits=dl, loss_sum=loss_sum, correct=correct)
    g = dl.t() @ f
    g = g.t() if w_fmajor else g
    if store:
        dw.copy_(g)
    else:
        dw += g
    if db is not None:
        if store:
            db.copy_(dl.sum(0))
        else:
            db += dl.sum(0)
    if dl_out is not None:
        dl_out.copy_(dl)
    if dfeat16 is not None:
        dfeat16.copy_((dl @ wf).to(dfeat16.dtype))
    return True


def colsum(x, M, N, ld, db, scale=1.0):
    if x.is_cuda:
        require().colsum(x, M, N, ld, db, scale)
        return
    idx = torch.arange(M).unsqueeze(1) * ld + torch.arange(N).unsqueeze(0)
    db += scale * x.reshape(-1).float()[idx].sum(0)


def act_grad(dy, y, dz, act):
    if dy.is_cuda:
        require().act_grad(dy, y, dz, act)
        return
    dz.copy_(dy * _act_grad_from_out_ref(y, act))


def bias_act(x, bias, out, act, keep=1.0, seed=0, counter=None):
    if x.is_cuda:
        require().bias_act(x, bias, out, act, keep, seed, counter)
        return
    v = _act_ref(x.float() + (bias.float() if bias is not None else 0), act)
    if keep < 1.0:  # bias_act_kernel: stream index step * M*N + i over the flat [M][N] tensor
        step = int(counter.reshape(-1)[0].item()) if counter is not None else 0
        v = _dropout_ref(v, np.arange(v.numel()), keep, seed, step * v.numel())
    out.copy_(v.to(out.dtype))


# -------------------------------------------------------------------- LSTM
def lstm_cell_fwd(gates, act, c_prev, c, h_out, ld_h, forget_bias=1.0):
    """TF BasicLSTMCell step on pre-activation gates [B,4H] (order i, j, f, o)."""
    if gates.is_cuda:
        require().lstm_cell_fwd(gates, act, c_prev, c, h_out, ld_h, forget_bias)
        return
    H = c.shape[1]
    i, j, f, o = gates.split(H, dim=1)
    si, tj, sf, so = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + forget_bias), torch.sigmoid(o)
    cn = (c_prev * sf if c_prev is not None else 0) + si * tj
    c.copy_(cn)
    act.copy_(torch.cat([si, tj, sf, so], dim=1))
    h_out.copy_(torch.tanh(cn) * so)  # h_out is a [B, H] (possibly strided) view


def lstm_cell_bwd(act, c_prev, c, dh, dh2, dc_next, dgates, dc_prev):
    if act.is_cuda:
        require().lstm_cell_bwd(act, c_prev, c, dh, dh2, dc_next, dgates, dc_prev)
        return
    H = c.shape[1]
    si, tj, sf, so = act.split(H, dim=1)
    d = (dh if dh is not None else 0) + (dh2 if dh2 is not None else 0)
    tc = torch.tanh(c)
    dc = (dc_next if dc_next is not None else 0) + d * so * (1 - tc * tc)
    cp = c_prev if c_prev is not None else torch.zeros_like(c)
    dgates.copy_(torch.cat([dc * tj * si * (1 - si), dc * si * (1 - tj * tj), dc * cp * sf * (1 - sf),
                            d * tc * so * (1 - so)], dim=1))
    dc_prev.copy_(dc * sf)


# ------------------------------------------------------------- batch norm
# NHWC bf16 activations viewed as [R][C]; stats are fp32 [2][C] accumulators the
# caller zeroes: forward (sum, sum of squares) of x - x[row 0] (per-channel shift),
# backward (sum g, sum g*xhat).
def _rows(t):
    return t.reshape(-1, t.shape[-1]).float()


def bn_stats(x, stats):
    if x.is_cuda:
        require().bn_stats(x, stats)
        return
    r = _rows(x)
    C = r.shape[1]
    d = r - r[0]  # shifted by row 0 (as the kernel) against E[x^2]-E[x]^2 cancellation
    stats[:C] += d.sum(0)
    stats[C:] += (d * d).sum(0)


def _bn_params(stats, R, eps, shift):
    C = stats.numel() // 2
    d = stats[:C] / R
    var = (stats[C:] / R - d * d).clamp_min(0)
    return shift + d, torch.rsqrt(var + eps), var


def _shortcut_view(res, OH, OW, C, rstride):
    """option-A shortcut read: res[:, ::s, ::s, :] zero-padded to C channels (NHWC fp32)."""
    r = res.float()[:, ::rstride, ::rstride, :][:, :OH, :OW, :]
    if r.shape[-1] < C:
        r = torch.nn.functional.pad(r, (0, C - r.shape[-1]))
    return r


def bn_apply(x, stats, gamma, beta, out, *, mean=None, invstd=None, moving_mean=None, moving_var=None, eps=1e-3,
             momentum=0.99, act=ACT_RELU, res=None, rstride=1, mask_out=None, res_bn=None):
    """out = act(gamma * (x - mean) * invstd + beta [+ shortcut(res)]) with batch statistics from
    ``stats``; stores mean/invstd and updates the moving averages (TF momentum convention).
    ``mask_out`` (ReLU): uint8 [R][C/8] bit mask of out > 0, which the backward ops take in place
    of ``y`` (``relu_bits``).  ``res_bn`` = [stats, gamma, beta, mean, invstd, moving_mean,
    moving_var] of the residual's own BatchNorm (a projection shortcut, no activation): ``res`` is
    then that BN's raw input, normalised here exactly as its own bn_apply would store it, and that
    BN's mean / invstd / moving averages are saved / updated here too."""
    OH, OW = (x.shape[1], x.shape[2]) if x.dim() == 4 else (1, 1)
    if x.is_cuda:
        require().bn_apply(x, stats, gamma, beta, mean, invstd, moving_mean, moving_var, eps, momentum, act, res,
                           rstride, OH, OW, out, mask_out, res_bn)
        return out
    if res_bn is not None:
        rs, rg, rb, rm, ri, rmm, rmv = res_bn
        r_out = torch.empty_like(res)
        bn_apply(res, rs, rg, rb, r_out, mean=rm, invstd=ri, moving_mean=rmm, moving_var=rmv, eps=eps,
                 momentum=momentum, act=ACT_NONE)
        res = r_out
    r = _rows(x)
    R, C = r.shape
    m, inv, var = _bn_params(stats, R, eps, r[0])
    if mean is not None:
        mean.copy_(m)
    if invstd is not None:
        invstd.copy_(inv)
    if moving_mean is not None:
        unb = var * R / max(R - 1, 1)
        moving_mean.mul_(momentum).add_(m * (1 - momentum))
        moving_var.mul_(momentum).add_(unb * (1 - momentum))
    y = (r - m) * inv * gamma.float() + beta.float()
    if res is not None:
        y = y + _shortcut_view(res, OH, OW, C, rstride).reshape(R, C)
    out.copy_(_act_ref(y, act).reshape(out.shape).to(out.dtype))
    if mask_out is not None:
        mask_out.copy_(relu_bits(out))
    return out


def relu_bits(y):
    """uint8 [R][C/8] bit mask of y > 0 (bit e of byte (r, j) = channel 8 j + e) - the layout
    bn_apply(mask_out=...) writes."""
    r = _rows(y) > 0
    R, C = r.shape
    w = (1 << torch.arange(8, device=r.device, dtype=torch.int32))
    return (r.reshape(R, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


def _unbits(m, R, C):
    e = torch.arange(8, device=m.device, dtype=torch.int32)
    return ((m.reshape(R, C // 8, 1).to(torch.int32) >> e) & 1).reshape(R, C).bool()


def bn_infer(x, gamma, beta, moving_mean, moving_var, out, *, eps=1e-3, act=ACT_RELU, res=None, rstride=1):
    """Inference-mode BatchNorm (TF ``training=False``): out = act(gamma * (x - moving_mean) *
    rsqrt(moving_var + eps) + beta [+ shortcut(res)]); nothing is updated."""
    OH, OW = (x.shape[1], x.shape[2]) if x.dim() == 4 else (1, 1)
    if x.is_cuda:
        require().bn_infer(x, gamma, beta, moving_mean, moving_var, eps, act, res, rstride, OH, OW, out)
        return out
    r = _rows(x)
    R, C = r.shape
    inv = torch.rsqrt(moving_var.float() + eps)
    y = (r - moving_mean.float()) * inv * gamma.float() + beta.float()
    if res is not None:
        y = y + _shortcut_view(res, OH, OW, C, rstride).reshape(R, C)
    out.copy_(_act_ref(y, act).reshape(out.shape).to(out.dtype))
    return out


def _masked_grad(dy, y, act, x=None, mean=None, invstd=None, gamma=None, beta=None):
    g = _rows(dy)
    if act != ACT_NONE:
        if y is None:  # ReLU mask recomputed from the pre-normalisation input (no residual in the forward)
            scale = gamma.float() * invstd
            pre = _rows(x) * scale + (beta.float() - mean * scale)
            return g * (pre > 0)
        if y.dtype == torch.uint8:  # bn_apply's bit mask of the ReLU output
            return g * _unbits(y, g.shape[0], g.shape[1])
        g = g * _act_grad_from_out_ref(_rows(y), act)
    return g


def bn_bwd_stats(dy, y, x, mean, invstd, stats, act=ACT_RELU, gamma=None, beta=None, res_bn=None):
    """stats += (sum g, sum g*xhat), g = dy*act'(y).  With y=None and act=ReLU the mask is
    recomputed from x (the forward had no residual add): pass gamma and beta.  ``res_bn`` = [x2,
    mean2, invstd2, stats2] (y a uint8 ReLU bit mask): the same pass also adds (sum g, sum g*xhat2)
    into stats2 - a projection shortcut's BN, whose gradient is this g."""
    if x.is_cuda:
        require().bn_bwd_stats(dy, y, x, mean, invstd, stats, act, gamma, beta, res_bn)
        return
    g = _masked_grad(dy, y, act, x, mean, invstd, gamma, beta)
    xh = (_rows(x) - mean) * invstd
    C = g.shape[1]
    stats[:C] += g.sum(0)
    stats[C:] += (g * xh).sum(0)
    if res_bn is not None:
        x2, m2, i2, s2 = res_bn
        s2[:C] += g.sum(0)
        s2[C:] += (g * ((_rows(x2) - m2) * i2)).sum(0)


def bn_bwd_apply(dy, y, x, mean, invstd, gamma, stats, dx, *, act=ACT_RELU, dres=None, dgamma=None, dbeta=None,
                 beta=None):
    """dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)), g = dy*act'(y); dgamma/dbeta += sums;
    dres = g (gradient of an added shortcut).  y=None + beta: ReLU mask from x (see bn_bwd_stats)."""
    if x.is_cuda:
        require().bn_bwd_apply(dy, y, x, mean, invstd, gamma, stats, act, dx, dres, dgamma, dbeta, beta)
        return dx
    g = _masked_grad(dy, y, act, x, mean, invstd, gamma, beta)
    R, C = g.shape
    xh = (_rows(x) - mean) * invstd
    d = gamma.float() * invstd * (g - stats[:C] / R - xh * stats[C:] / R)
    dx.copy_(d.reshape(dx.shape).to(dx.dtype))
    if dres is not None:
        dres.copy_(g.reshape(dres.shape).to(dres.dtype))
    if dgamma is not None:
        dgamma += stats[C:]
    if dbeta is not None:
        dbeta += stats[:C]
    return dx


def shortcut_grad_add(g, dx, stride=1):
    """dx[:, ::s, ::s, :XC] += g[..., :XC] (gradient of the option-A identity shortcut)."""
    if dx.is_cuda:
        require().shortcut_grad_add(g, dx, stride)
        return dx
    XC = dx.shape[-1]
    OH, OW = g.shape[1], g.shape[2]
    v = dx[:, ::stride, ::stride, :][:, :OH, :OW, :]
    v.copy_((v.float() + g[..., :XC].float()).to(dx.dtype))
    return dx


def gap_fwd(x, y):
    if x.is_cuda:
        require().gap_fwd(x, y)
        return y
    y.copy_(x.float().mean(dim=(1, 2)).reshape(y.shape).to(y.dtype))
    return y


def gap_bwd(dy, dx):
    if dx.is_cuda:
        require().gap_bwd(dy, dx)
        return dx
    B, H, W, C = dx.shape
    dx.copy_((dy.float().reshape(B, 1, 1, C) / (H * W)).expand(B, H, W, C).to(dx.dtype))
    return dx


def maxpool3_fwd(x, y, am):
    """3x3 / stride 2 / pad 1 max pool (NHWC) with the window argmax (0..8, first max wins)."""
    if x.is_cuda:
        require().maxpool3_fwd(x, y, am)
        return y
    B, H, W, C = x.shape
    xp = torch.nn.functional.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), value=-3.0e38)
    cols = torch.nn.functional.unfold(xp, 3, stride=2)  # [B, C*9, L]
    OH, OW = y.shape[1], y.shape[2]
    cols = cols.view(B, C, 9, OH * OW)
    v, i = cols.max(dim=2)
    y.copy_(v.view(B, C, OH, OW).permute(0, 2, 3, 1).to(y.dtype))
    am.copy_(i.view(B, C, OH, OW).permute(0, 2, 3, 1).to(am.dtype))
    return y


def bn_relu_pool3(x, stats, gamma, beta, y, am, *, mean=None, invstd=None, moving_mean=None, moving_var=None,
                  eps=1e-3, momentum=0.99):
    """bn_apply(act=ReLU) + maxpool3_fwd in one pass: the pooled output ``y`` and argmax ``am`` of
    the normalised map, which is never stored; mean / invstd / moving averages as bn_apply.  Bit-
    identical to the two-op sequence (the ResNet-50 stem)."""
    if x.is_cuda:
        require().bn_relu_pool3(x, stats, gamma, beta, mean, invstd, moving_mean, moving_var, eps, momentum, y, am)
        return y
    h = torch.empty_like(x)
    bn_apply(x, stats, gamma, beta, h, mean=mean, invstd=invstd, moving_mean=moving_mean, moving_var=moving_var,
             eps=eps, momentum=momentum, act=ACT_RELU)
    return maxpool3_fwd(h, y, am)


def pool3_bn_bwd(dp, am, x, mean, invstd, gamma, beta, stats, dx, *, dgamma=None, dbeta=None):
    """maxpool3_bwd + bn_bwd_stats + bn_bwd_apply (ReLU mask recomputed from x) without the unpooled
    gradient: ``dp`` / ``am`` are the pooled gradient and argmax, ``x`` the BN input, ``stats`` the
    zeroed [2][C] backward accumulators; dx, dgamma / dbeta (+=) as bn_bwd_apply (the ResNet-50 stem)."""
    if dx.is_cuda:
        require().pool3_bn_bwd(dp, am, x, mean, invstd, gamma, beta, stats, dx, dgamma, dbeta)
        return dx
    d = maxpool3_bwd(dp, am, torch.empty_like(x))
    bn_bwd_stats(d, None, x, mean, invstd, stats, ACT_RELU, gamma=gamma, beta=beta)
    bn_bwd_apply(d, None, x, mean, invstd, gamma, stats, dx, act=ACT_RELU, dgamma=dgamma, dbeta=dbeta, beta=beta)
    return dx


def maxpool3_bwd(dy, am, dx):
    if dx.is_cuda:
        require().maxpool3_bwd(dy, am, dx)
        return dx
    B, H, W, C = dx.shape
    OH, OW = dy.shape[1], dy.shape[2]
    cols = torch.zeros(B, C, 9, OH * OW)
    g = dy.float().permute(0, 3, 1, 2).reshape(B, C, 1, OH * OW)
    cols.scatter_(2, am.long().permute(0, 3, 1, 2).reshape(B, C, 1, OH * OW), g)
    d = torch.nn.functional.fold(cols.view(B, C * 9, OH * OW), (H + 2, W + 2), 3, stride=2)[:, :, 1:H + 1, 1:W + 1]
    dx.copy_(d.permute(0, 2, 3, 1).to(dx.dtype))
    return dx
