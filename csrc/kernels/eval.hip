// Evaluation metrics of one chunk of logits, accumulated on the device: top-1 / top-k hits, the
// cross-entropy sum, the row count and the bad-label count of a pass over n examples, B rows per
// launch.  All progress (the chunk cursor included) is device state, so the launch is the same
// whether it is issued eagerly or replayed from a graph, and the host reads once per pass.
//
// One wave per row, lanes strided over the classes (NC = 10 ... 1000+): a max pass, then one pass
// that sums exp(z - max) and counts the classes ranked before the label.  A row's loss and flag
// bits go to the workspace; the last workgroup to arrive folds rows [0, valid) in row order - the
// loss in double - into the state, advances the cursor and writes the next chunk's row indices.
// Every word is bitwise reproducible: no floating-point atomics, nothing waits or spins.
#include "eval.h"

namespace dtfe {

namespace {
constexpr uint32_t EV_COUNT = 1u, EV_HIT1 = 2u, EV_HITK = 4u, EV_BAD = 8u;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
}  // namespace

__global__ __launch_bounds__(256) void eval_metrics_kernel(EvalMetricsArgs a) {
  __shared__ __attribute__((aligned(16))) float stage[256];  // the fold's staging: 256 row losses
  __shared__ int cnt[4];                                      // ... and its counters: rows, top-1, top-k, bad
  __shared__ int lastf;
  const int tid = threadIdx.x, lane = tid & 63;
  const int B = a.B, NC = a.NC;
  if (tid < 4) cnt[tid] = 0;  // (the barrier ahead of the ticket orders this before the fold's adds)
  // the cursor is written by the last workgroup only, after every workgroup has taken its ticket -
  // and a workgroup takes it after these loads were used: all of them see the same chunk
  const long cursor = __hip_atomic_load(&a.state->cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const long n = __hip_atomic_load(&a.state->n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const long left = n - cursor * B;
  const int valid = left < 0 ? 0 : (left > B ? B : (int)left);
  if (valid == 0) return;  // past the end (uniform over the grid): nothing moves, the ticket included
  const int row = blockIdx.x * 4 + (tid >> 6);
  if (row < valid) {
    const float* z = a.logits + (long)row * NC;
    const int t = a.labels[row];
    const bool bad = t < 0 || t >= NC;
    const float zt = bad ? 0.f : z[t];
    float mx = -INFINITY;
    for (int j = lane; j < NC; j += 64) mx = fmaxf(mx, z[j]);
    mx = wave_max(mx);
    float se = 0.f;
    int before = 0;  // classes ranked before the label: larger, or equal with a smaller index
    for (int j = lane; j < NC; j += 64) {
      const float v = z[j];
      se += expf(v - mx);
      before += (v > zt || (v == zt && j < t)) ? 1 : 0;
    }
    se = wave_sum(se);
    before = wave_sum_i(before);
    const float loss = (mx + logf(se)) - zt;
    const bool ranked = !bad && zt == zt;  // a NaN target compares false everywhere: a miss, not rank 0
    const uint32_t flags = EV_COUNT | (ranked && before == 0 ? EV_HIT1 : 0u) | (ranked && before < a.k ? EV_HITK : 0u) |
                           (bad ? EV_BAD : 0u);
    if (lane == 0) {
      // written through to memory (agent scope) for the last workgroup
      __hip_atomic_store(a.ws + row, __float_as_uint(bad ? 0.f : loss), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.ws + B + row, flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // every storing wave's row words have completed before the workgroup takes its ticket; the last
  // arriver then sees every row (the hand-off of grad_sumsq_kernel)
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
  // fold rows [0, valid), 256 at a time: the counters by ballot (integer sums: any order gives the same
  // words), the losses through LDS, added in row order in double by one lane (a bad-label row left 0)
  double sum = tid == 0 ? a.state->loss_sum : 0.0;
  for (int base = 0; base < valid; base += 256) {
    const int b = base + tid;
    uint32_t f = 0u;
    float l = 0.f;
    if (b < valid) {
      l = __uint_as_float(__hip_atomic_load(a.ws + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      f = __hip_atomic_load(a.ws + B + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    stage[tid] = l;
    const int c0 = __popcll(__ballot(f & EV_COUNT)), c1 = __popcll(__ballot(f & EV_HIT1)),
              c2 = __popcll(__ballot(f & EV_HITK)), c3 = __popcll(__ballot(f & EV_BAD));
    if (lane == 0) {
      atomicAdd(&cnt[0], c0);
      atomicAdd(&cnt[1], c1);
      atomicAdd(&cnt[2], c2);
      atomicAdd(&cnt[3], c3);
    }
    __syncthreads();
    if (tid == 0) {
      const int m = valid - base < 256 ? valid - base : 256;
      int i = 0;
      for (; i + 4 <= m; i += 4) {
        const f32x4_t q = *reinterpret_cast<const f32x4_t*>(stage + i);
        sum += (double)q[0];
        sum += (double)q[1];
        sum += (double)q[2];
        sum += (double)q[3];
      }
      for (; i < m; ++i) sum += (double)stage[i];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.state->count += cnt[0];
    a.state->hits1 += cnt[1];
    a.state->hitsk += cnt[2];
    a.state->bad_labels += cnt[3];
    a.state->loss_sum = sum;
    a.state->cursor = cursor + 1;
  }
  if (a.idx) {
    const long next = (cursor + 1) * B;
    for (int b = tid; b < B; b += 256) {
      const long r = next + b;
      a.idx[b] = (int32_t)(r < n - 1 ? r : n - 1);
    }
  }
}

void launch_eval_metrics(const EvalMetricsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(eval_metrics_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
}

}  // namespace dtfe
