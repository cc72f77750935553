// Per-variable norms and LARS trust ratios of an optimizer's adaptive variables, one launch per step.
//
// Bandwidth-bound: one read of the masters and one of the gradient.  A workgroup takes chunks
// (<= 8192 elements, all of one variable) of the plan; a thread issues its 16-byte loads of both
// streams - 8-byte for a bf16 gradient - before the first add.  Every output bit is independent of
// the grid: chunk c's two sums have a fixed order (per-thread serial, wave butterfly, the four waves
// through LDS) and land in partials[c]; the last workgroup to arrive adds each variable's partials
// in chunk order, in double, and turns the two sums into the variable's trust ratio.  The hand-off
// is grad_sumsq_kernel's (gradnorm.hip): write-through partials, a relaxed ticket, one acquire.
// No floating-point atomics, nothing waits or spins.
#include "lars.h"

namespace dtfe {

template <bool G16>
__device__ __forceinline__ f32x4_t lars_grad4(const LarsArgs& a, long i) {
  if constexpr (!G16) {
    return *reinterpret_cast<const f32x4_t*>(a.g + i);
  } else {
    const u32x2_t w = *reinterpret_cast<const u32x2_t*>(a.g16 + i);
    return f32x4_t{__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16),
                   __uint_as_float(w[1] & 0xffff0000u)};
  }
}

template <bool G16>
__global__ __launch_bounds__(256) void layer_trust_kernel(LarsArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[2][4];
  __shared__ __attribute__((aligned(16))) float stage[4][2][64];  // the fold: a strip of 64 partial pairs per wave
  __shared__ int lastf;
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < a.nchunk; c += gridDim.x) {
    const LarsChunk ch = a.plan[c];
    // vector body only from a 16-B (bf16: 8-B) aligned base: both are 4 elements
    const long n4 = (ch.off & 3) == 0 ? (ch.count & ~3L) : 0;
    constexpr int U = LARS_CHUNK_MAX / 1024;
    f32x4_t pv[U], gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = tid * 4 + u * 1024;
      pv[u] = j < n4 ? *reinterpret_cast<const f32x4_t*>(a.p + ch.off + j) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      gv[u] = j < n4 ? lars_grad4<G16>(a, ch.off + j) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    float sw = 0.f, sg = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = gv[u][e] * a.gscale;
        sw += pv[u][e] * pv[u][e];
        sg += x * x;
      }
    }
    for (long j = n4 + tid; j < ch.count; j += 256) {  // misaligned base / tail: per element
      const float w = a.p[ch.off + j];
      const float x = (G16 ? bf2f(a.g16[ch.off + j]) : a.g[ch.off + j]) * a.gscale;
      sw += w * w;
      sg += x * x;
    }
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    __syncthreads();  // the previous chunk's part[] has been read
    if ((tid & 63) == 0) {
      part[0][tid >> 6] = sw;
      part[1][tid >> 6] = sg;
    }
    __syncthreads();
    // one lane each, one slot pair per chunk: written through to memory (agent scope) for the last workgroup
    if (tid < 2)
      __hip_atomic_store(a.partials + 2 * (long)c + tid, (part[tid][0] + part[tid][1]) + (part[tid][2] + part[tid][3]),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // every wave's partial stores have completed before the workgroup takes its ticket (only wave 0 stores);
  // the last arriver then sees every partial
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
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
  // fold: a wave per adaptive variable.  64 chunks' partials arrive with one load per lane and stream and go
  // through the wave's own LDS strip; lane 0 then adds them in chunk order - the order is the plan's alone -
  // four per 16-byte LDS read, the two sums as independent chains.  A wave's LDS operations complete in
  // order, so its lanes need no barrier between the strip's stores and lane 0's reads.
  const int lane = tid & 63, wave = tid >> 6;
  for (int s = wave; s < a.nadapt; s += 4) {
    const LarsSeg r = a.segs[s];
    double dw = 0.0, dg = 0.0;
    for (int base = 0; base < r.n; base += 64) {
      const int i = base + lane;
      float w = 0.f, g = 0.f;  // past the variable's last chunk: +0, which changes no sum
      if (i < r.n) {
        w = __hip_atomic_load(a.partials + 2 * (long)(r.first + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g = __hip_atomic_load(a.partials + 2 * (long)(r.first + i) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      stage[wave][0][lane] = w;
      stage[wave][1][lane] = g;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (lane == 0) {
        const int n = r.n - base < 64 ? r.n - base : 64;
        for (int k = 0; k < n; k += 4) {  // whole quads: the strip's tail holds the zeros stored above
          const f32x4_t qw = *reinterpret_cast<const f32x4_t*>(&stage[wave][0][k]);
          const f32x4_t qg = *reinterpret_cast<const f32x4_t*>(&stage[wave][1][k]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            dw += (double)qw[e];
            dg += (double)qg[e];
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // the strip has been read before the next 64 overwrite it
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0) {
      const float fw = (float)dw, fg = (float)dg;
      a.sums[2 * r.seg] = fw;
      a.sums[2 * r.seg + 1] = fg;
      a.trust[r.seg] = lars_trust_eval(fw, fg, a.eeta, a.wd[r.seg], a.eps, a.clip_scale);
    }
  }
}

void launch_layer_trust(const LarsArgs& a, hipStream_t s) {
  int blocks = a.nchunk < LARS_MAX_BLOCKS ? a.nchunk : LARS_MAX_BLOCKS;
  if (a.max_blocks > 0 && blocks > a.max_blocks) blocks = a.max_blocks;
  if (blocks < 1) blocks = 1;
  if (a.g) hipLaunchKernelGGL(layer_trust_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(layer_trust_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace dtfe
