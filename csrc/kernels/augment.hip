// Batch gather with the image input transforms of the CIFAR recipe in the same launch: random crop
// of the zero-padded image, random horizontal flip, per-channel standardisation (augment.h has the
// definition).  One workgroup per image stages the source row in LDS with aligned vector loads and
// forms 8-element output chunks from it: with C = 3 a chunk straddles pixels, a flip reverses pixels
// (not channels) and a dx shift moves the source by C * dx elements, so the reads of a chunk are
// unaligned - in LDS that costs nothing, from global memory it would break every vector load.
#include "augment.h"

// (v - mean) * inv_std is specified as a subtraction and a multiplication, each rounded, and
// v = byte * (1 / 255) is rounded before the subtraction: no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace dtfe {

namespace {

// 384 threads = the 384 8-element chunks of a 32x32x3 image: one chunk per thread, one pass (with 256
// half the waves ran a second pass on the workgroup's critical path: 6.78 -> 5.94 us per B = 128 launch
// beside gather_rows' 5.2, profiles/augment.txt)
constexpr int AUG_THREADS = 384;
constexpr int AUG_LDS_BYTES = 16384;  // one source image: 32x32x3 uint8 = 3 KiB, fp32 = 12 KiB
constexpr int AUG_LDS_MAX_C = 64;     // channel statistics staged next to it

struct Draw { long r; int dy, dx; bool flipped; };

// Row: the stream of gather_rows.  Crop offsets and flip: one draw of the salted stream per sample.
// h is uniform over 2^32 values and span^2 * 2 <= 1922, so for pad <= 15 the probability of every
// dx, dy and flip value is within 2^-22 of uniform (the modulo bias).
// SHUF (idx null, SAMPLE_SHUFFLE): the row comes from the epoch permutation; `row` >= 0 hands in one
// that was resolved already.
template <bool SHUF>
__device__ __forceinline__ Draw aug_draw(const AugmentArgs& a, int b, int64_t step, long row = -1) {
  const uint64_t i = (uint64_t)step * a.B + b;
  Draw w;
  if (SHUF) w.r = row >= 0 ? row : shuffled_row(a.seed, step, a.B, a.n_rows, b);
  else w.r = a.idx ? (long)a.idx[b] : (long)(hash_u32(a.seed, i) % (uint32_t)a.n_rows);
  const uint32_t span = 2u * a.pad + 1u;
  const uint32_t h = hash_u32(a.seed ^ AUG_SALT, i);
  w.dx = (int)(h % span);
  w.dy = (int)((h / span) % span);
  w.flipped = a.flip && ((h / (span * span)) & 1u);
  return w;
}

__device__ __forceinline__ float standardise(float v, float mean, float inv_std) { return (v - mean) * inv_std; }

// every workgroup has read *counter (and used it) before it arrives; the last one advances it: the
// ticket of gather_rows (elementwise.hip), relaxed agent-scope atomics, no data handed over
__device__ __forceinline__ void aug_advance_counter(int64_t* counter, uint32_t* done) {
  if (!counter || !done) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_fetch_add((unsigned long long*)counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// one-hot label rows, zero ranges, counter ticket: the tail both kernels share (grid-strided).
// SHUF: the kernels wrote the one-hot rows where they had the sample's row at hand.
template <bool SHUF>
__device__ __forceinline__ void aug_tail(const AugmentArgs& a, int64_t step) {
  const long tid = (long)blockIdx.x * AUG_THREADS + threadIdx.x, nth = (long)gridDim.x * AUG_THREADS;
  if (a.onehot && !SHUF) {
    const long n = (long)a.B * a.ncls;
    for (long i = tid; i < n; i += nth) {
      const int b = (int)(i / a.ncls);
      const int c = (int)(i - (long)b * a.ncls);
      a.onehot[i] = a.labels_src[aug_draw<false>(a, b, step).r] == c ? 1.f : 0.f;
    }
  }
  for (int z = 0; z < a.nz; ++z)
    for (long i = tid; i < a.zlen[z]; i += nth) a.zptr[z][i] = 0u;
  aug_advance_counter(a.counter, a.done);
}

// D % 8 == 0, one image <= AUG_LDS_BYTES, C <= AUG_LDS_MAX_C, src / dst 16-byte aligned
template <bool U8, bool BF, bool SHUF>
__global__ __launch_bounds__(AUG_THREADS) void augment_rows_lds_kernel(AugmentArgs a) {
  __shared__ u32x4_t img4[AUG_LDS_BYTES / 16];
  __shared__ float stat[2 * AUG_LDS_MAX_C];
  __shared__ int row_s;  // SHUF: the image's source row, resolved by thread 0
  uint8_t* img = reinterpret_cast<uint8_t*>(img4);
  const int64_t step = a.counter ? *a.counter : 0;
  const int D = a.H * a.W * a.C;
  const int nbytes = D * (U8 ? 1 : 4);  // a multiple of 8 (uint8) or 32 (fp32)
  const bool stats = a.mean != nullptr;
  if (stats && (int)threadIdx.x < a.C) {
    stat[threadIdx.x] = a.mean[threadIdx.x];
    stat[AUG_LDS_MAX_C + threadIdx.x] = a.inv_std[threadIdx.x];
  }
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    if (SHUF) {  // once per image: thread 0 walks the permutation, the workgroup reads the row from LDS
      if (threadIdx.x == 0) row_s = (int)shuffled_row(a.seed, step, a.B, a.n_rows, b);
      __syncthreads();  // (the barrier that ends the previous image keeps its readers ahead of this store)
    }
    const Draw w = aug_draw<SHUF>(a, b, step, SHUF ? (long)row_s : -1);
    if (a.labels_dst && threadIdx.x == 0) a.labels_dst[b] = a.labels_src[w.r];
    if (SHUF && a.onehot) {
      const int lab = a.labels_src[w.r];
      for (int c = threadIdx.x; c < a.ncls; c += AUG_THREADS) a.onehot[(long)b * a.ncls + c] = lab == c ? 1.f : 0.f;
    }
    const uint8_t* row = reinterpret_cast<const uint8_t*>(a.src) + w.r * (long)nbytes;
    if ((nbytes & 15) == 0) {
      for (int i = threadIdx.x * 16; i < nbytes; i += AUG_THREADS * 16)
        *reinterpret_cast<u32x4_t*>(img + i) = *reinterpret_cast<const u32x4_t*>(row + i);
    } else {  // uint8 rows of 8 (mod 16) bytes start 8-byte aligned only
      for (int i = threadIdx.x * 8; i < nbytes; i += AUG_THREADS * 8)
        *reinterpret_cast<u32x2_t*>(img + i) = *reinterpret_cast<const u32x2_t*>(row + i);
    }
    __syncthreads();
    for (int d = threadIdx.x * 8; d < D; d += AUG_THREADS * 8) {
      const int p = d / a.C;
      int c = d - p * a.C;
      int y = p / a.W;
      int x = p - y * a.W;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // d + e < D: y stays below H
        const int ys = y + w.dy - a.pad;
        const int xs = (w.flipped ? a.W - 1 - x : x) + w.dx - a.pad;
        float t = 0.f;
        if ((unsigned)ys < (unsigned)a.H && (unsigned)xs < (unsigned)a.W) {
          const int s = (ys * a.W + xs) * a.C + c;  // < D
          t = U8 ? (float)img[s] * (1.f / 255.f) : reinterpret_cast<const float*>(img)[s];
          if (stats) t = standardise(t, stat[c], stat[AUG_LDS_MAX_C + c]);
        }
        v[e] = t;
        if (++c == a.C) {
          c = 0;
          if (++x == a.W) { x = 0; ++y; }
        }
      }
      const long o = (long)b * D + d;
      if (BF) {
        *reinterpret_cast<u32x4_t*>(reinterpret_cast<bf16*>(a.dst) + o) =
            u32x4_t{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                    pack_bf16x2(v[6], v[7])};
      } else {
        f32x4_t* q = reinterpret_cast<f32x4_t*>(reinterpret_cast<float*>(a.dst) + o);
        q[0] = f32x4_t{v[0], v[1], v[2], v[3]};
        q[1] = f32x4_t{v[4], v[5], v[6], v[7]};
      }
    }
    __syncthreads();  // the next image's staging overwrites img
  }
  aug_tail<SHUF>(a, step);
}

// any shape (224x224x3, odd D): one thread per output element, correct rather than fast
// SHUF: the rows [b0, b0 + cnt) of the workgroup's next AUG_THREADS elements are resolved once, one per
// thread, into LDS (gather_rows' window); the element with d == 0 writes its sample's one-hot row.
template <bool SHUF>
__global__ __launch_bounds__(AUG_THREADS) void augment_rows_elem_kernel(AugmentArgs a) {
  __shared__ int rows[SHUF ? AUG_THREADS : 1];
  const int64_t step = a.counter ? *a.counter : 0;
  const long D = (long)a.H * a.W * a.C;
  const long n = (long)a.B * D;
  for (long base = (long)blockIdx.x * AUG_THREADS; base < n; base += (long)gridDim.x * AUG_THREADS) {
    const long i = base + threadIdx.x;
    int b0 = 0;
    if (SHUF) {  // (base is uniform: every thread meets the barriers)
      const long last = base + AUG_THREADS - 1 < n - 1 ? base + AUG_THREADS - 1 : n - 1;
      b0 = (int)(base / D);
      const int cnt = (int)(last / D) - b0 + 1;
      __syncthreads();
      if ((int)threadIdx.x < cnt) rows[threadIdx.x] = (int)shuffled_row(a.seed, step, a.B, a.n_rows, b0 + (int)threadIdx.x);
      __syncthreads();
    }
    if (i >= n) continue;
    const int b = (int)(i / D);
    const int d = (int)(i - (long)b * D);
    const Draw w = aug_draw<SHUF>(a, b, step, SHUF ? (long)rows[b - b0] : -1);
    if (a.labels_dst && d == 0) a.labels_dst[b] = a.labels_src[w.r];
    if (SHUF && a.onehot && d == 0) {
      const int lab = a.labels_src[w.r];
      for (int c = 0; c < a.ncls; ++c) a.onehot[(long)b * a.ncls + c] = lab == c ? 1.f : 0.f;
    }
    const int p = d / a.C, c = d - p * a.C;
    const int y = p / a.W, x = p - y * a.W;
    const int ys = y + w.dy - a.pad;
    const int xs = (w.flipped ? a.W - 1 - x : x) + w.dx - a.pad;
    float t = 0.f;
    if ((unsigned)ys < (unsigned)a.H && (unsigned)xs < (unsigned)a.W) {
      const long s = w.r * D + ((long)(ys * a.W + xs) * a.C + c);
      t = a.src_dtype == 0 ? (float)reinterpret_cast<const uint8_t*>(a.src)[s] * (1.f / 255.f)
                           : reinterpret_cast<const float*>(a.src)[s];
      if (a.mean) t = standardise(t, a.mean[c], a.inv_std[c]);
    }
    if (a.dst_dtype == 1) reinterpret_cast<float*>(a.dst)[i] = t;
    else reinterpret_cast<bf16*>(a.dst)[i] = f2bf(t);
  }
  aug_tail<SHUF>(a, step);
}

}  // namespace

void launch_augment_rows(const AugmentArgs& a, hipStream_t s) {
  const long D = (long)a.H * a.W * a.C;
  const long esz = a.src_dtype == 0 ? 1 : 4;
  const bool shuf = !a.idx && a.sample == SAMPLE_SHUFFLE;
  const bool lds = D % 8 == 0 && D * esz <= AUG_LDS_BYTES && a.C <= AUG_LDS_MAX_C &&
                   ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)a.dst & 15) == 0;
  if (lds) {
    long blocks = a.B < 1 ? 1 : a.B;
    if (blocks > 2048) blocks = 2048;
    const dim3 g((unsigned)blocks), t(AUG_THREADS);
#define AUG_LDS_LAUNCH(U8, BF)                                                                          \
  do {                                                                                                  \
    if (shuf) hipLaunchKernelGGL((augment_rows_lds_kernel<U8, BF, true>), g, t, 0, s, a);               \
    else hipLaunchKernelGGL((augment_rows_lds_kernel<U8, BF, false>), g, t, 0, s, a);                   \
  } while (0)
    if (a.src_dtype == 0) {
      if (a.dst_dtype == 2) AUG_LDS_LAUNCH(true, true);
      else AUG_LDS_LAUNCH(true, false);
    } else {
      if (a.dst_dtype == 2) AUG_LDS_LAUNCH(false, true);
      else AUG_LDS_LAUNCH(false, false);
    }
#undef AUG_LDS_LAUNCH
    return;
  }
  long blocks = ((long)a.B * D + AUG_THREADS - 1) / AUG_THREADS;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  if (shuf) hipLaunchKernelGGL(augment_rows_elem_kernel<true>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, s, a);
  else hipLaunchKernelGGL(augment_rows_elem_kernel<false>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, s, a);
}

}  // namespace dtfe
