// Batch gather with the image input transforms of the CIFAR recipe in the same launch: random crop
// of the zero-padded image, random horizontal flip, per-channel standardisation (augment.h has the
// definition).  One workgroup per image stages the source row in LDS with aligned vector loads and
// forms 8-element output chunks from it: with C = 3 a chunk straddles pixels, a flip reverses pixels
// (not channels) and a dx shift moves the source by C * dx elements, so the reads of a chunk are
// unaligned - in LDS that costs nothing, from global memory it would break every vector load.
// Mixup / CutMix stage the partner's image next to the slot's and form each chunk from both.
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

// the transformed pixel A(y, x, c) of the definition under draw w: from an image staged in LDS ...
template <bool U8>
__device__ __forceinline__ float lds_pixel(const AugmentArgs& a, const uint8_t* img, const float* stat, bool stats,
                                           const Draw& w, int y, int x, int c) {
  const int ys = y + w.dy - a.pad;
  const int xs = (w.flipped ? a.W - 1 - x : x) + w.dx - a.pad;
  float t = 0.f;
  if ((unsigned)ys < (unsigned)a.H && (unsigned)xs < (unsigned)a.W) {
    const int s = (ys * a.W + xs) * a.C + c;  // < D
    t = U8 ? (float)img[s] * (1.f / 255.f) : reinterpret_cast<const float*>(img)[s];
    if (stats) t = standardise(t, stat[c], stat[AUG_LDS_MAX_C + c]);
  }
  return t;
}

// ... and from source row w.r in global memory
__device__ __forceinline__ float global_pixel(const AugmentArgs& a, const Draw& w, long D, int y, int x, int c) {
  const int ys = y + w.dy - a.pad;
  const int xs = (w.flipped ? a.W - 1 - x : x) + w.dx - a.pad;
  float t = 0.f;
  if ((unsigned)ys < (unsigned)a.H && (unsigned)xs < (unsigned)a.W) {
    const long s = w.r * D + ((long)(ys * a.W + xs) * a.C + c);
    t = a.src_dtype == 0 ? (float)reinterpret_cast<const uint8_t*>(a.src)[s] * (1.f / 255.f)
                         : reinterpret_cast<const float*>(a.src)[s];
    if (a.mean) t = standardise(t, a.mean[c], a.inv_std[c]);
  }
  return t;
}

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

// an unmixed label row's element: 1 / 0, or with SMOOTH (label smoothing) the host's two values
template <bool SMOOTH>
__device__ __forceinline__ float label_value(const AugmentArgs& a, bool hit) {
  return hit ? (SMOOTH ? a.smooth_on : 1.f) : (SMOOTH ? a.smooth_off : 0.f);
}

// one-hot label rows, zero ranges, counter ticket: the tail both kernels share (grid-strided).
// SHUF: the kernels wrote the one-hot rows where they had the sample's row at hand.
template <bool SHUF, bool SMOOTH>
__device__ __forceinline__ void aug_tail(const AugmentArgs& a, int64_t step) {
  const long tid = (long)blockIdx.x * AUG_THREADS + threadIdx.x, nth = (long)gridDim.x * AUG_THREADS;
  if (a.onehot && !SHUF) {
    const long n = (long)a.B * a.ncls;
    for (long i = tid; i < n; i += nth) {
      const int b = (int)(i / a.ncls);
      const int c = (int)(i - (long)b * a.ncls);
      a.onehot[i] = label_value<SMOOTH>(a, a.labels_src[aug_draw<false>(a, b, step).r] == c);
    }
  }
  for (int z = 0; z < a.nz; ++z)
    for (long i = tid; i < a.zlen[z]; i += nth) a.zptr[z][i] = 0u;
  aug_advance_counter(a.counter, a.done);
}

// D % 8 == 0, one image <= AUG_LDS_BYTES, C <= AUG_LDS_MAX_C, src / dst 16-byte aligned
template <bool U8, bool BF, bool SHUF, bool SMOOTH>
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
      for (int c = threadIdx.x; c < a.ncls; c += AUG_THREADS) a.onehot[(long)b * a.ncls + c] = label_value<SMOOTH>(a, lab == c);
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
        v[e] = lds_pixel<U8>(a, img, stat, stats, w, y, x, c);
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
  aug_tail<SHUF, SMOOTH>(a, step);
}

// any shape (224x224x3, odd D): one thread per output element, correct rather than fast
// SHUF: the rows [b0, b0 + cnt) of the workgroup's next AUG_THREADS elements are resolved once, one per
// thread, into LDS (gather_rows' window); the element with d == 0 writes its sample's one-hot row.
template <bool SHUF, bool SMOOTH>
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
      for (int c = 0; c < a.ncls; ++c) a.onehot[(long)b * a.ncls + c] = label_value<SMOOTH>(a, lab == c);
    }
    const int p = d / a.C, c = d - p * a.C;
    const int y = p / a.W, x = p - y * a.W;
    const float t = global_pixel(a, w, D, y, x, c);
    if (a.dst_dtype == 1) reinterpret_cast<float*>(a.dst)[i] = t;
    else reinterpret_cast<bf16*>(a.dst)[i] = f2bf(t);
  }
  aug_tail<SHUF, SMOOTH>(a, step);
}

// ---- mixup / CutMix (augment.h): kernels of their own, so that the two above stay what they were

// slot b's partner p, its label weight w (lam, or lam' of the box) and, for CutMix, the box in output coordinates
struct Mix { int p; float w; int y0, y1, x0, x1; };

__device__ __forceinline__ int mix_partner(const AugmentArgs& a, int b, int64_t step) {
  const uint32_t shift = 1u + hash_u32(a.seed ^ MIX_ROT_SALT, (uint64_t)step) % (uint32_t)(a.B - 1);
  const uint32_t p = (uint32_t)b + shift;  // < 2 B <= 2^32 - 2
  return (int)(p >= (uint32_t)a.B ? p - (uint32_t)a.B : p);
}

__device__ __forceinline__ Mix mix_draw(const AugmentArgs& a, int mode, int b, int64_t step) {
  const uint64_t i = (uint64_t)step * a.B + b;
  Mix m;
  m.p = mix_partner(a, b, step);
  m.y0 = m.y1 = m.x0 = m.x1 = 0;
  const uint32_t k = hash_u32(a.seed ^ MIX_LAM_SALT, i) >> 8;
  if (mode == MIX_MIXUP) {
    m.w = (float)k * (1.0f / 16777216.0f);
    return m;
  }
  // r = floor(sqrt(v)), v <= 2^48 exact as a double; the double root only proposes, the integers decide
  const uint64_t v = (uint64_t)(16777216u - k) << 24;
  uint64_t r = (uint64_t)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  const int rw = (int)(((uint64_t)a.W * r) >> 24), rh = (int)(((uint64_t)a.H * r) >> 24);  // r <= 2^24: rw <= W
  const uint32_t hb = hash_u32(a.seed ^ MIX_BOX_SALT, i);
  const int cx = (int)(hb % (uint32_t)a.W), cy = (int)((hb / (uint32_t)a.W) % (uint32_t)a.H);
  m.x0 = cx - rw / 2 > 0 ? cx - rw / 2 : 0;
  m.x1 = cx + rw / 2 < a.W ? cx + rw / 2 : a.W;
  m.y0 = cy - rh / 2 > 0 ? cy - rh / 2 : 0;
  m.y1 = cy + rh / 2 < a.H ? cy + rh / 2 : a.H;
  m.w = (float)((long)a.H * a.W - (long)(m.x1 - m.x0) * (m.y1 - m.y0)) * a.inv_hw;
  return m;
}

// element c of the mixed label row: three roundings, as a mixed pixel
__device__ __forceinline__ float mix_label(const AugmentArgs& a, float w, int lab, int labp, int c) {
  return w * label_value<true>(a, lab == c) + (1.f - w) * label_value<true>(a, labp == c);
}

// augment_rows_lds_kernel's conditions; the slot's image and its partner's are staged side by side.
// The label rows need both labels: written here for every sampling mode, the tail writes none.
template <bool U8, bool BF, bool SHUF, int MIX>
__global__ __launch_bounds__(AUG_THREADS) void augment_mix_lds_kernel(AugmentArgs a) {
  __shared__ u32x4_t img4[2][AUG_LDS_BYTES / 16];  // both regions 16-byte aligned: the same staging stores
  __shared__ float stat[2 * AUG_LDS_MAX_C];
  __shared__ int row_s[2];  // SHUF: the source rows of the slot and of its partner
  uint8_t* img = reinterpret_cast<uint8_t*>(img4[0]);
  uint8_t* imgp = reinterpret_cast<uint8_t*>(img4[1]);
  const int64_t step = a.counter ? *a.counter : 0;
  const int D = a.H * a.W * a.C;
  const int nbytes = D * (U8 ? 1 : 4);
  const bool stats = a.mean != nullptr;
  if (stats && (int)threadIdx.x < a.C) {
    stat[threadIdx.x] = a.mean[threadIdx.x];
    stat[AUG_LDS_MAX_C + threadIdx.x] = a.inv_std[threadIdx.x];
  }
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const Mix m = mix_draw(a, MIX, b, step);
    if (SHUF) {  // once per image, in two waves side by side: neither chunk loop walks a permutation
      if (threadIdx.x == 0) row_s[0] = (int)shuffled_row(a.seed, step, a.B, a.n_rows, b);
      if (threadIdx.x == 64) row_s[1] = (int)shuffled_row(a.seed, step, a.B, a.n_rows, m.p);
      __syncthreads();  // (the barrier that ends the previous image keeps its readers ahead of these stores)
    }
    const Draw w = aug_draw<SHUF>(a, b, step, SHUF ? (long)row_s[0] : -1);
    const Draw wp = aug_draw<SHUF>(a, m.p, step, SHUF ? (long)row_s[1] : -1);
    const int lab = a.labels_src[w.r], labp = a.labels_src[wp.r];
    if (a.labels_dst && threadIdx.x == 0) a.labels_dst[b] = lab;
    for (int c = threadIdx.x; c < a.ncls; c += AUG_THREADS) a.onehot[(long)b * a.ncls + c] = mix_label(a, m.w, lab, labp, c);
    const uint8_t* row = reinterpret_cast<const uint8_t*>(a.src) + w.r * (long)nbytes;
    const uint8_t* rowp = reinterpret_cast<const uint8_t*>(a.src) + wp.r * (long)nbytes;
    if ((nbytes & 15) == 0) {
      for (int i = threadIdx.x * 16; i < nbytes; i += AUG_THREADS * 16) {
        *reinterpret_cast<u32x4_t*>(img + i) = *reinterpret_cast<const u32x4_t*>(row + i);
        *reinterpret_cast<u32x4_t*>(imgp + i) = *reinterpret_cast<const u32x4_t*>(rowp + i);
      }
    } else {  // uint8 rows of 8 (mod 16) bytes start 8-byte aligned only
      for (int i = threadIdx.x * 8; i < nbytes; i += AUG_THREADS * 8) {
        *reinterpret_cast<u32x2_t*>(img + i) = *reinterpret_cast<const u32x2_t*>(row + i);
        *reinterpret_cast<u32x2_t*>(imgp + i) = *reinterpret_cast<const u32x2_t*>(rowp + i);
      }
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
        if (MIX == MIX_MIXUP) {
          v[e] = m.w * lds_pixel<U8>(a, img, stat, stats, w, y, x, c) +
                 (1.f - m.w) * lds_pixel<U8>(a, imgp, stat, stats, wp, y, x, c);
        } else {  // one read, from the image the box assigns to (y, x)
          const bool in = y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1;
          v[e] = lds_pixel<U8>(a, in ? imgp : img, stat, stats, in ? wp : w, y, x, c);
        }
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
    __syncthreads();  // the next image's staging overwrites both regions
  }
  aug_tail<true, false>(a, step);
}

// any shape: one thread per output element draws its slot's mix again, correct rather than fast.
// SHUF: the window of rows as in augment_rows_elem_kernel, and next to it the partners' rows.
template <bool SHUF>
__global__ __launch_bounds__(AUG_THREADS) void augment_mix_elem_kernel(AugmentArgs a) {
  __shared__ int rows[SHUF ? 2 * AUG_THREADS : 1];
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
      if ((int)threadIdx.x < cnt) {
        const int bt = b0 + (int)threadIdx.x;
        rows[threadIdx.x] = (int)shuffled_row(a.seed, step, a.B, a.n_rows, bt);
        rows[AUG_THREADS + threadIdx.x] = (int)shuffled_row(a.seed, step, a.B, a.n_rows, mix_partner(a, bt, step));
      }
      __syncthreads();
    }
    if (i >= n) continue;
    const int b = (int)(i / D);
    const int d = (int)(i - (long)b * D);
    const Mix m = mix_draw(a, a.mix, b, step);
    const Draw w = aug_draw<SHUF>(a, b, step, SHUF ? (long)rows[b - b0] : -1);
    const Draw wp = aug_draw<SHUF>(a, m.p, step, SHUF ? (long)rows[AUG_THREADS + b - b0] : -1);
    if (d == 0) {
      const int lab = a.labels_src[w.r], labp = a.labels_src[wp.r];
      if (a.labels_dst) a.labels_dst[b] = lab;
      for (int c = 0; c < a.ncls; ++c) a.onehot[(long)b * a.ncls + c] = mix_label(a, m.w, lab, labp, c);
    }
    const int p = d / a.C, c = d - p * a.C;
    const int y = p / a.W, x = p - y * a.W;
    float t;
    if (a.mix == MIX_MIXUP) {
      t = m.w * global_pixel(a, w, D, y, x, c) + (1.f - m.w) * global_pixel(a, wp, D, y, x, c);
    } else {
      const bool in = y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1;
      t = global_pixel(a, in ? wp : w, D, y, x, c);
    }
    if (a.dst_dtype == 1) reinterpret_cast<float*>(a.dst)[i] = t;
    else reinterpret_cast<bf16*>(a.dst)[i] = f2bf(t);
  }
  aug_tail<true, false>(a, step);
}

template <bool U8, bool BF, bool SHUF>
void launch_lds(const AugmentArgs& a, bool smooth, dim3 g, hipStream_t s) {
  const dim3 t(AUG_THREADS);
  if (a.mix == MIX_MIXUP) hipLaunchKernelGGL((augment_mix_lds_kernel<U8, BF, SHUF, MIX_MIXUP>), g, t, 0, s, a);
  else if (a.mix == MIX_CUTMIX) hipLaunchKernelGGL((augment_mix_lds_kernel<U8, BF, SHUF, MIX_CUTMIX>), g, t, 0, s, a);
  else if (smooth) hipLaunchKernelGGL((augment_rows_lds_kernel<U8, BF, SHUF, true>), g, t, 0, s, a);
  else hipLaunchKernelGGL((augment_rows_lds_kernel<U8, BF, SHUF, false>), g, t, 0, s, a);
}

template <bool SHUF>
void launch_elem(const AugmentArgs& a, bool smooth, dim3 g, hipStream_t s) {
  const dim3 t(AUG_THREADS);
  if (a.mix != MIX_NONE) hipLaunchKernelGGL(augment_mix_elem_kernel<SHUF>, g, t, 0, s, a);
  else if (smooth) hipLaunchKernelGGL((augment_rows_elem_kernel<SHUF, true>), g, t, 0, s, a);
  else hipLaunchKernelGGL((augment_rows_elem_kernel<SHUF, false>), g, t, 0, s, a);
}

}  // namespace

void launch_augment_rows(const AugmentArgs& a, hipStream_t s) {
  const long D = (long)a.H * a.W * a.C;
  const long esz = a.src_dtype == 0 ? 1 : 4;
  const bool shuf = !a.idx && a.sample == SAMPLE_SHUFFLE;
  const bool smooth = a.smooth_on != 1.f || a.smooth_off != 0.f;  // hard labels: the instantiations without the two loads
  // (mixing stages two images in two AUG_LDS_BYTES regions: the same condition)
  const bool lds = D % 8 == 0 && D * esz <= AUG_LDS_BYTES && a.C <= AUG_LDS_MAX_C &&
                   ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)a.dst & 15) == 0;
  if (lds) {
    long blocks = a.B < 1 ? 1 : a.B;
    if (blocks > 2048) blocks = 2048;
    const dim3 g((unsigned)blocks);
#define AUG_LDS_LAUNCH(U8, BF)                                                                          \
  do {                                                                                                  \
    if (shuf) launch_lds<U8, BF, true>(a, smooth, g, s);                                                \
    else launch_lds<U8, BF, false>(a, smooth, g, s);                                                    \
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
  if (shuf) launch_elem<true>(a, smooth, dim3((unsigned)blocks), s);
  else launch_elem<false>(a, smooth, dim3((unsigned)blocks), s);
}

}  // namespace dtfe
