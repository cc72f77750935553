// Global gradient norm of an optimizer's var list and the clip_by_global_norm scale, on the device
// (so a captured step can depend on how large this step's gradient was).
//
// Bandwidth-bound: one read of the gradient.  A workgroup takes chunks (<= 8192 elements) of the
// plan; a thread issues its (up to 8) 16-byte loads of a chunk - 8-byte for a bf16 gradient -
// before the first add.  The result is bitwise reproducible and independent of the grid: chunk c's
// sum has a fixed order (per-thread serial, wave butterfly, the four waves through LDS) and lands
// in partials[c]; the last workgroup to arrive adds partials[0..n) in index order, in double.
// No floating-point atomics, nothing waits or spins.
#include "gradnorm.h"

namespace dtfe {

template <bool G16>
__device__ __forceinline__ f32x4_t grad_load4(const GradNormArgs& a, long i) {
  if constexpr (!G16) {
    return *reinterpret_cast<const f32x4_t*>(a.g + i);
  } else {
    const u32x2_t w = *reinterpret_cast<const u32x2_t*>(a.g16 + i);
    return f32x4_t{__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16),
                   __uint_as_float(w[1] & 0xffff0000u)};
  }
}

template <bool G16>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradNormArgs a) {
  __shared__ float part[4];
  __shared__ __attribute__((aligned(16))) float stage[256];
  __shared__ int lastf;
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < a.nchunk; c += gridDim.x) {
    const GradChunk ch = a.plan[c];
    // vector body only from a 16-B (bf16: 8-B) aligned base: both are 4 elements
    const long n4 = (ch.off & 3) == 0 ? (ch.count & ~3L) : 0;
    f32x4_t v[GRAD_CHUNK_MAX / 1024];
#pragma unroll
    for (int u = 0; u < GRAD_CHUNK_MAX / 1024; ++u) {
      const long j = tid * 4 + u * 1024;
      v[u] = j < n4 ? grad_load4<G16>(a, ch.off + j) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < GRAD_CHUNK_MAX / 1024; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = v[u][e] * a.gscale;
        acc += x * x;
      }
    }
    for (long j = n4 + tid; j < ch.count; j += 256) {  // misaligned base / tail: per element
      const float x = (G16 ? bf2f(a.g16[ch.off + j]) : a.g[ch.off + j]) * a.gscale;
      acc += x * x;
    }
    acc = wave_sum(acc);
    __syncthreads();  // the previous chunk's part[] has been read
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    // one lane, one slot per chunk: written through to memory (agent scope) for the last workgroup
    if (tid == 0)
      __hip_atomic_store(a.partials + c, (part[0] + part[1]) + (part[2] + part[3]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid == 0) {
    // this workgroup's partial stores have completed before it takes its ticket; the last arriver
    // then sees every partial (the hand-off of mse_sigmoid_kernel / the split-K GEMMs)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t prev = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == gridDim.x - 1;
    if (last) {
      __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch / replay
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    lastf = last;
  }
  __syncthreads();
  if (!lastf) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  // fold in index order: 256 partials at a time through LDS, added serially in double by one lane
  double sum = 0.0;
  for (int base = 0; base < a.nchunk; base += 256) {
    const int i = base + tid;
    stage[tid] = i < a.nchunk ? __hip_atomic_load(a.partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    __syncthreads();
    if (tid == 0) {
      const int n = a.nchunk - base < 256 ? a.nchunk - base : 256;
      int k = 0;
      for (; k + 4 <= n; k += 4) {
        const f32x4_t q = *reinterpret_cast<const f32x4_t*>(stage + k);
        sum += (double)q[0];
        sum += (double)q[1];
        sum += (double)q[2];
        sum += (double)q[3];
      }
      for (; k < n; ++k) sum += (double)stage[k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float norm = (float)sqrt(sum);
    a.out[0] = norm;
    a.out[1] = (a.clip_norm > 0.f && norm > a.clip_norm) ? a.clip_norm / norm : 1.f;
  }
}

void launch_grad_sumsq(const GradNormArgs& a, hipStream_t s) {
  int blocks = a.nchunk < GRAD_NORM_MAX_BLOCKS ? a.nchunk : GRAD_NORM_MAX_BLOCKS;
  if (a.max_blocks > 0 && blocks > a.max_blocks) blocks = a.max_blocks;
  if (blocks < 1) blocks = 1;
  if (a.g) hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(256) void scale_ranges_kernel(float* t, const float* scale, const GradChunk* plan,
                                                           int nchunk) {
  const float s = *scale;
  for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const GradChunk ch = plan[c];
    const long n4 = (ch.off & 3) == 0 ? (ch.count & ~3L) : 0;
    for (long j = threadIdx.x * 4; j < n4; j += 1024) {
      f32x4_t* q = reinterpret_cast<f32x4_t*>(t + ch.off + j);
      *q = *q * s;
    }
    for (long j = n4 + threadIdx.x; j < ch.count; j += 256) t[ch.off + j] *= s;
  }
}

void launch_scale_ranges(float* t, const float* scale, const GradChunk* plan, int nchunk, hipStream_t s) {
  if (nchunk < 1) return;
  const int blocks = nchunk < GRAD_NORM_MAX_BLOCKS ? nchunk : GRAD_NORM_MAX_BLOCKS;
  hipLaunchKernelGGL(scale_ranges_kernel, dim3(blocks), dim3(256), 0, s, t, scale, plan, nchunk);
}

}  // namespace dtfe
