// Fused multi-tensor apply_gradients: one launch updates
// every parameter of a model in the flat fp32 master buffer with TF1-exact
// math, refreshes the bf16 working copies the MFMA kernels read (natural and,
// where a backward GEMM wants it, transposed through an LDS tile), and - in
// its last workgroup - advances global_step and Adam's beta powers, the
// scalars TF keeps as separate variables (AssignAdd / _finish in TF1).
//
// TF1 reference semantics (tensorflow/python/training/*.py @ 1.11):
//   SGD       : v -= lr*g
//   Momentum  : a = m*a + g ; v -= lr*a
//   Adam      : lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m = b1 m + (1-b1) g;
//               v2 = b2 v2 + (1-b2) g^2; v -= lr_t * m / (sqrt(v2) + eps)
//   RMSProp   : ms = rho ms + (1-rho) g^2 ; mom = mu mom + lr g / sqrt(ms + eps); v -= mom
//               (ms slot initialised to ONES by the host)
//   Nesterov  : a = m*a + g ; v -= g*lr + (a*m)*lr            (ApplyMomentum, use_nesterov)
// Optional, all inside the same launch: lr from a schedule evaluated at global_step
// (OptArgs::sched), a coupled L2 term per segment, g = g*scale + wd*v (OptSeg::wd), and an exponential
// moving average of the updated values, shadow -= (shadow - v) * (1 - decay) (OptArgs::ema); ema_swap_kernel
// exchanges the two buffers to evaluate with the average.
//
// Memory-bound: the flat path moves 4 elements per thread per iteration with
// 16-byte loads/stores of every stream (p, g, slots) and 8-byte bf16 stores.
#include "optim.h"

namespace dtfe {

// the rates of one launch: lr is the host's a.lr or the schedule's value at *global_step; lr_t is what
// Adam multiplies with (lr with the bias correction folded in), lr itself for the other kinds
struct OptRate {
  float lr, lr_t;
  float omd;  // the EMA instantiations: 1 - decay of this launch (unused, and no register, in the others)
};

template <int KIND, bool NAG>
__device__ __forceinline__ float upd(const OptArgs& a, OptRate rt, float v, float g, float& s1, float& s2) {
  // no multiply-add contraction: the rounding of every update must not depend on how a kernel
  // instantiation's instruction selection happened to fuse it (a grouped launch of several
  // optimizers and separate launches must agree bitwise)
#pragma clang fp contract(off)
  if constexpr (KIND == OPT_SGD) {
    return v - rt.lr * g;
  } else if constexpr (KIND == OPT_MOMENTUM) {
    if constexpr (NAG) {
      if (a.nesterov) {  // TF1 ApplyMomentum, use_nesterov: a = a m + g ; v -= g lr + a m lr
        s1 = s1 * a.momentum + g;
        return v - (g * rt.lr + s1 * a.momentum * rt.lr);
      }
    }
    s1 = s1 * a.momentum + g;
    return v - rt.lr * s1;
  } else if constexpr (KIND == OPT_ADAM) {
    return tf1_adam(v, g, s1, s2, rt.lr_t, a.beta1, a.beta2, a.eps);
  } else {
    s1 = s1 * a.rho + (1.f - a.rho) * g * g;
    s2 = s2 * a.momentum + rt.lr * g / sqrtf(s1 + a.eps);
    return v - s2;
  }
}

// the gradient an update sees: g * gs (gs: the host's scale times a clip's), plus - in the weight-decay
// instantiation, for a segment with wd != 0 - the coupled L2 term wd * p, added after the clip scale
// as torch.optim.SGD(weight_decay=) adds it after clip_grad_norm_.  A select, not "+ 0 * p": a segment
// without decay keeps its -0 and does not meet a non-finite parameter.
template <bool WD>
__device__ __forceinline__ float scaled_grad(float g, float gs, float wd, float p) {
#pragma clang fp contract(off)
  const float x = g * gs;
  if constexpr (WD) return wd != 0.f ? x + wd * p : x;
  return x;
}

template <int KIND, bool NAG>
__device__ __forceinline__ float update_one(const OptArgs& a, OptRate rt, long i, float p, float g) {
  float s1 = 0.f, s2 = 0.f;
  if (KIND != OPT_SGD) s1 = a.s1[i];
  if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) s2 = a.s2[i];
  const float v = upd<KIND, NAG>(a, rt, p, g, s1, s2);
  a.p[i] = v;
  if (KIND != OPT_SGD) a.s1[i] = s1;
  if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) a.s2[i] = s2;
  return v;
}

template <bool G16>
__device__ __forceinline__ float load_grad(const OptArgs& a, long i) {
  return G16 ? bf2f(a.g16[i]) : a.g[i];
}

// the updated values' extra destinations: bf16 copies (w16, the ps reply's w16b) and the fp32 copy pb
__device__ __forceinline__ void store_copies(const f32x4_t& p, bf16* w16, bf16* w16b, float* pb) {
  if (w16 || w16b) {
    const u32x2_t q = {pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3])};
    if (w16) *reinterpret_cast<u32x2_t*>(w16) = q;
    if (w16b) *reinterpret_cast<u32x2_t*>(w16b) = q;
  }
  if (pb) *reinterpret_cast<f32x4_t*>(pb) = p;
}

template <int KIND, bool G16, bool WD, bool NAG, bool EMA>
__device__ __forceinline__ void update_vec4(const OptArgs& a, OptRate rt, float gs, float wd, long i, bf16* w16, bf16* w16b,
                                            float* pb) {
  f32x4_t g;
  if constexpr (!G16) {
    g = *reinterpret_cast<const f32x4_t*>(a.g + i);
  } else {
    const u32x2_t w = *reinterpret_cast<const u32x2_t*>(a.g16 + i);
    g = f32x4_t{__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16),
                __uint_as_float(w[1] & 0xffff0000u)};
  }
  f32x4_t p = *reinterpret_cast<const f32x4_t*>(a.p + i);
  f32x4_t s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  if (KIND != OPT_SGD) s1 = *reinterpret_cast<const f32x4_t*>(a.s1 + i);
  if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) s2 = *reinterpret_cast<const f32x4_t*>(a.s2 + i);
  f32x4_t e = {0.f, 0.f, 0.f, 0.f};
  if constexpr (EMA) e = *reinterpret_cast<const f32x4_t*>(a.ema + i);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float x1 = s1[j], x2 = s2[j];
    p[j] = upd<KIND, NAG>(a, rt, p[j], scaled_grad<WD>(g[j], gs, wd, p[j]), x1, x2);
    s1[j] = x1;
    s2[j] = x2;
    if constexpr (EMA) e[j] = ema_update(e[j], p[j], rt.omd);
  }
  *reinterpret_cast<f32x4_t*>(a.p + i) = p;
  if (KIND != OPT_SGD) *reinterpret_cast<f32x4_t*>(a.s1 + i) = s1;
  if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) *reinterpret_cast<f32x4_t*>(a.s2 + i) = s2;
  if constexpr (EMA) *reinterpret_cast<f32x4_t*>(a.ema + i) = e;
  store_copies(p, w16, w16b, pb);
}

// U vec4 updates at i, i+1024, ... (one workgroup-wide stride apart): every load is issued
// before the first update, so each thread keeps U x (3-4) 16-B loads in flight (one more with EMA)
template <int KIND, int U, bool G16, bool WD, bool NAG, bool EMA>
__device__ __forceinline__ void update_vec4x(const OptArgs& a, OptRate rt, float gs, float wd, long i, bf16* w16, bf16* w16b,
                                             float* pb) {
  f32x4_t g[U], p[U], s1[U], s2[U], e[EMA ? U : 1];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long k = i + u * 1024;
    if constexpr (!G16) {
      g[u] = *reinterpret_cast<const f32x4_t*>(a.g + k);
    } else {
      const u32x2_t w = *reinterpret_cast<const u32x2_t*>(a.g16 + k);
      g[u] = f32x4_t{__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16),
                     __uint_as_float(w[1] & 0xffff0000u)};
    }
    p[u] = *reinterpret_cast<const f32x4_t*>(a.p + k);
    s1[u] = s2[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (KIND != OPT_SGD) s1[u] = *reinterpret_cast<const f32x4_t*>(a.s1 + k);
    if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) s2[u] = *reinterpret_cast<const f32x4_t*>(a.s2 + k);
    if constexpr (EMA) e[u] = *reinterpret_cast<const f32x4_t*>(a.ema + k);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long k = i + u * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x1 = s1[u][j], x2 = s2[u][j];
      p[u][j] = upd<KIND, NAG>(a, rt, p[u][j], scaled_grad<WD>(g[u][j], gs, wd, p[u][j]), x1, x2);
      s1[u][j] = x1;
      s2[u][j] = x2;
      if constexpr (EMA) e[u][j] = ema_update(e[u][j], p[u][j], rt.omd);
    }
    *reinterpret_cast<f32x4_t*>(a.p + k) = p[u];
    if (KIND != OPT_SGD) *reinterpret_cast<f32x4_t*>(a.s1 + k) = s1[u];
    if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) *reinterpret_cast<f32x4_t*>(a.s2 + k) = s2[u];
    if constexpr (EMA) *reinterpret_cast<f32x4_t*>(a.ema + k) = e[u];
    store_copies(p[u], w16 ? w16 + u * 1024 : nullptr, w16b ? w16b + u * 1024 : nullptr, pb ? pb + u * 1024 : nullptr);
  }
}

// How many vec4 updates a thread of the flat path keeps in flight.  Without EMA: 4, as ever.  The EMA
// instantiations hold one more 16-byte array per update in flight (Adam / RMSProp: five - g, p, two slots,
// shadow - 20 VGPRs each).  The compiler's register report (-Rpass-analysis=kernel-resource-usage) at 4 in
// flight, without -> with EMA: Adam 140 -> 166 and RMSProp 135 -> 158 VGPRs, both still 3 waves per SIMD
// (the step to 2 is past 170) and no scratch; momentum 112 -> 133 (4 -> 3 waves), SGD 96 -> 114 (5 -> 4).
// Compiled with 2 in flight, SGD and momentum report the same counts (114 and 134): the instantiation's
// registers are set by the transposed-tile path, whose 16 elements per thread now carry a shadow each, not
// by this body - a smaller unroll buys no wave back and only takes loads out of flight.  So: 4 for every
// kind, chosen from the register counts, not from a timing of each choice; bench/ema_apply_bench.py times
// the result against the stock second pass (profiles/ema_apply.txt).
template <int KIND, bool EMA>
__device__ constexpr int ema_unroll() {
  return 4;
}

// the rate of one segment's items under OptArgs::seg_lr
__device__ __forceinline__ float seg_rate(float lr, float factor) {
#pragma clang fp contract(off)
  return lr * factor;
}

// One optimizer's share of a launch: workgroups bid = 0..nblk-1 of the grid (the whole grid for a
// plain launch, a contiguous range of it for a grouped one).
// lr: the launch's learning rate (launch_rate); omd: 1 - the launch's EMA decay (launch_ema_decay).
// SLR: the instantiation with a per-segment factor of the rate (OptArgs::seg_lr): an item's rate is
// lr * seg_lr[its segment], one multiply
template <int KIND, bool G16, bool WD, bool NAG, bool EMA, bool SLR>
__device__ __forceinline__ void apply_items(const OptArgs& a, float lr, float omd, int bid, int nblk,
                                            bf16 (&tile)[64][66]) {
  OptRate rt{lr, lr, omd};
  if (KIND == OPT_ADAM) rt.lr_t = tf1_adam_lr(lr, a.beta_pow);
  // the gradient scale of this launch: the host's, times the device scalar of a global-norm clip
  // (grad_sumsq_kernel's out[1], written by the launch before this one on the stream)
  const float gs = a.clip_scale ? a.gscale * *a.clip_scale : a.gscale;
  bool waited = false;
  for (int wi = bid; wi < a.nwork; wi += nblk) {
    const OptWork w = a.work[wi];
    const OptSeg sg = a.segs[w.seg];
    if constexpr (SLR) rt.lr = rt.lr_t = seg_rate(lr, a.seg_lr[w.seg]);
    if (a.wait_done && !waited && w.seg < 32 && ((a.wait_segs >> w.seg) & 1u)) {
      // the producer (another stream, no graph edge) signals through *wait_done; poll with a bounded
      // wall-clock wait (a producer that never ran: proceed rather than hang the device)
      if (threadIdx.x == 0) {
        const int target = __hip_atomic_load(a.wait_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load(a.wait_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target &&
               wall_clock64() - t0 < 200000000ull)  // 2 s at 100 MHz
          __builtin_amdgcn_s_sleep(2);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      waited = true;
    }
    if (w.kind == 0) {
      const long base = sg.off + w.start;
      const long n4 = ((base & 3) == 0) ? (w.count / 4) * 4 : 0;  // segments are 64-aligned; chunks 8192
      long j = threadIdx.x * 4;
      auto at16 = [&](bf16* q, long jj) { return q ? q + w.start + jj : nullptr; };
      auto at32 = [&](float* q, long jj) { return q ? q + w.start + jj : nullptr; };
      constexpr int U = ema_unroll<KIND, EMA>();  // independent vec4 updates in flight per thread: 4 without EMA
      for (; j + (U - 1) * 1024 < n4; j += U * 1024)
        update_vec4x<KIND, U, G16, WD, NAG, EMA>(a, rt, gs, sg.wd, base + j, at16(sg.w16, j), at16(sg.w16b, j),
                                                 at32(sg.pb, j));
      for (; j < n4; j += 256 * 4)
        update_vec4<KIND, G16, WD, NAG, EMA>(a, rt, gs, sg.wd, base + j, at16(sg.w16, j), at16(sg.w16b, j), at32(sg.pb, j));
      for (long j = n4 + threadIdx.x; j < w.count; j += 256) {
        const long li = w.start + j, i = sg.off + li;
        const float p = a.p[i];
        const float v = update_one<KIND, NAG>(a, rt, i, p, scaled_grad<WD>(load_grad<G16>(a, i), gs, sg.wd, p));
        if constexpr (EMA) a.ema[i] = ema_update(a.ema[i], v, rt.omd);
        if (sg.w16) sg.w16[li] = f2bf(v);
        if (sg.w16b) sg.w16b[li] = f2bf(v);
        if (sg.pb) sg.pb[li] = v;
      }
    } else {
      // 64x64 tile of tap t: rows r0.., cols c0.. of the [R][C] slice; transposed copy via LDS
      // the 16 elements of a thread are loaded together before any update (the update's stores may
      // alias later loads, so a per-element loop ran 16 dependent HBM round trips per workgroup)
      const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
      const int c = w.c0 + tx;
      float gv[16], pv[16], s1v[16], s2v[16], ev[EMA ? 16 : 1];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int r = w.r0 + ty + 4 * u;
        // out-of-tile lanes load the segment's first element (never stored): no branches here
        const bool ok = r < sg.R && c < sg.C;
        const long i = sg.off + (ok ? ((long)r * sg.T + w.t) * sg.C + c : 0);
        pv[u] = a.p[i];
        gv[u] = scaled_grad<WD>(load_grad<G16>(a, i), gs, sg.wd, pv[u]);
        s1v[u] = KIND != OPT_SGD ? a.s1[i] : 0.f;
        s2v[u] = (KIND == OPT_ADAM || KIND == OPT_RMSPROP) ? a.s2[i] : 0.f;
        if constexpr (EMA) ev[u] = a.ema[i];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int rr = ty + 4 * u, r = w.r0 + rr;
        if (r < sg.R && c < sg.C) {
          const long li = ((long)r * sg.T + w.t) * sg.C + c, i = sg.off + li;
          float x1 = s1v[u], x2 = s2v[u];
          const float v = upd<KIND, NAG>(a, rt, pv[u], gv[u], x1, x2);
          a.p[i] = v;
          if (KIND != OPT_SGD) a.s1[i] = x1;
          if (KIND == OPT_ADAM || KIND == OPT_RMSPROP) a.s2[i] = x2;
          if constexpr (EMA) a.ema[i] = ema_update(ev[u], v, rt.omd);
          const bf16 b = f2bf(v);
          if (sg.w16) sg.w16[li] = b;
          if (sg.w16b) sg.w16b[li] = b;
          if (sg.pb) sg.pb[li] = v;
          tile[rr][tx] = b;
        }
      }
      __syncthreads();
      for (int cc = ty; cc < 64; cc += 4) {
        const int c = w.c0 + cc, r = w.r0 + tx;
        if (r < sg.R && c < sg.C) {
          const long ti = ((long)c * sg.T + w.t) * sg.R + r;
          if (sg.wt16) sg.wt16[ti] = tile[tx][cc];
          if (sg.wt16b) sg.wt16b[ti] = tile[tx][cc];
        }
      }
      __syncthreads();
    }
  }
}

// The learning rate of a launch, read by every workgroup before its first item: the host's a.lr, or the
// schedule's value at the global step the launch starts from.  The last workgroup advances the step
// only after every workgroup has finished its items, so all of a launch's workgroups read the same
// step here.  The whole struct is loaded before the step is waited for - one round trip to memory for
// both, not a chain of loads that depend on the step.
// Out of line: cold code that stays out of the update loops' register allocation (inlined it cost the
// plain SGD kernel 4 VGPRs, a wave of occupancy).  A call passes pointers in vector registers, so the
// schedule's address is made scalar again (readfirstlane of its halves): the struct arrives by scalar loads.
__device__ __noinline__ float scheduled_rate(const LrSchedule* sched, int32_t* global_step) {
  const uint64_t addr = reinterpret_cast<uint64_t>(sched);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)addr);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(addr >> 32));
  const LrSchedule s = *reinterpret_cast<const LrSchedule*>(((uint64_t)hi << 32) | lo);
  const int step = __hip_atomic_load(global_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return lr_schedule_eval(s, __builtin_amdgcn_readfirstlane(step));
}
__device__ __forceinline__ float launch_rate(const OptArgs& a) {
  if (!a.sched) return a.lr;
  // wave-uniform, and told so (readfirstlane): the rate stays in a scalar register like the host's a.lr
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(scheduled_rate(a.sched, a.global_step))));
}

// The EMA decay of a launch, read by every workgroup where the rate is: before its first item, so every
// workgroup of the launch sees the step the launch starts from.  With num_updates the decay is a function
// of the step AFTER this launch's advance (TF runs the EMA op after minimize has incremented the step).
// Out of line for scheduled_rate's reason: the division's dozen instructions are cold code.
__device__ __noinline__ float stepped_ema_decay(float decay, int32_t* global_step, int gs_inc) {
  const int step = __hip_atomic_load(global_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ema_decay_eval(decay, 1, __builtin_amdgcn_readfirstlane(step) + gs_inc);
}
__device__ __forceinline__ float launch_ema_decay(const OptArgs& a) {
  if (!a.ema_num_updates) return a.ema_decay;
  return __uint_as_float(
      __builtin_amdgcn_readfirstlane(__float_as_uint(stepped_ema_decay(a.ema_decay, a.global_step, a.gs_inc))));
}

// the ps reply words (ps_link.h PsWord: REP_GS 9, REP_VER 10, REP_STALE 11, REP_SEQ 8 last) into
// the worker's slot of the host-mapped shared page: system-scope relaxed stores (they go to the
// page, no cache holds them), the sequence number only after the others have completed - no
// release fence: an L2 write-back here would wait for every dirty line the apply just wrote
__device__ __forceinline__ void publish_reply(const OptArgs& a) {
  uint64_t* slot = a.rep_slot;
  const uint64_t gsv = a.rep_gs ? (uint64_t)(int64_t)__hip_atomic_load(const_cast<int32_t*>(a.rep_gs), __ATOMIC_RELAXED,
                                                                         __HIP_MEMORY_SCOPE_AGENT)
                                : (uint64_t)(int64_t)-1;
  __hip_atomic_store(slot + 9, gsv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(slot + 10, a.rep_ver, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(slot + 11, (uint64_t)a.rep_stale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(slot + 8, a.rep_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// WD: the weight-decay instantiation, launched only when some segment decays (OptArgs::decay); NAG: the
// one with the Nesterov branch (OptArgs::nesterov).  A launch with neither runs the kernel, and the
// arithmetic, it ran before there was either.  EMA: the one that also updates the shadow buffer
// (OptArgs::ema), launched only when there is one - the same rule; SLR: the one with a per-segment rate
// (OptArgs::seg_lr), likewise
template <int KIND, bool WD, bool NAG, bool EMA, bool SLR>
__device__ __forceinline__ void apply_body(const OptArgs& a, int bid, int nblk, bf16 (&tile)[64][66]) {
#pragma clang fp contract(off)
  const float lr = launch_rate(a);
  const float d = EMA ? launch_ema_decay(a) : 0.f;
  if (a.g) apply_items<KIND, false, WD, NAG, EMA, SLR>(a, lr, 1.f - d, bid, nblk, tile);
  else apply_items<KIND, true, WD, NAG, EMA, SLR>(a, lr, 1.f - d, bid, nblk, tile);
  // last workgroup: advance the non-slot scalars.  Every thread read them at its start and
  // used the value; after the barrier one lane takes a ticket (relaxed agent atomics - nothing
  // is handed between workgroups, so no fences) and the last arriver updates them.
  // A folded ps reply is handed over: every wave's stores (the reply buffer copies, uncached
  // memory) have completed before its workgroup takes the ticket, so the last arriver's reply
  // words follow every value the worker will read.
  if (a.rep_slot) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(a.done_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the rate this launch used, for logging: stored before the step it was computed from advances
    if (prev == (uint32_t)nblk - 1 && a.lr_out) *a.lr_out = lr;
    if (EMA && prev == (uint32_t)nblk - 1 && a.ema_out) *a.ema_out = d;
    if (prev == (uint32_t)nblk - 1 && !a.skip_advance) {
      if (KIND == OPT_ADAM) {
        a.beta_pow[0] *= a.beta1;
        a.beta_pow[1] *= a.beta2;
      }
      if (a.global_step && a.gs_inc) atomicAdd(a.global_step, a.gs_inc);
    }
    if (prev == (uint32_t)nblk - 1 && a.wait_seen)
      __hip_atomic_fetch_add(a.wait_seen, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == (uint32_t)nblk - 1 && a.rep_slot) publish_reply(a);
    if (prev == (uint32_t)nblk - 1) __hip_atomic_store(a.done_counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int KIND, bool WD, bool NAG, bool EMA, bool SLR = false>
__global__ __launch_bounds__(256) void apply_gradients_kernel(OptArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 tile[64][66];
  apply_body<KIND, WD, NAG, EMA, SLR>(a, blockIdx.x, gridDim.x, tile);
}

// Several optimizers of one kind in ONE launch (the GAN's two Adams over disjoint var lists):
// workgroup ranges [first[i], first[i + 1]) run optimizer i; each keeps its own done counter,
// beta powers and global-step increment, exactly as separate launches would.
// Not for optimizers with a schedule that share a global step: one optimizer's last workgroup may
// advance the step before another's workgroups have read it (launch_apply_gradients_group refuses).
// Nor, for the same reason, for optimizers with an EMA: the group kernels have no EMA instantiation -
// and none with a per-segment rate.
template <int KIND, bool WD, bool NAG>
__global__ __launch_bounds__(256) void apply_gradients_group_kernel(OptGroup g) {
  __shared__ __attribute__((aligned(16))) bf16 tile[64][66];
  int i = 0;
  while (i + 1 < g.n && (int)blockIdx.x >= g.first[i + 1]) ++i;
  apply_body<KIND, WD, NAG, false, false>(g.o[i], blockIdx.x - g.first[i], g.first[i + 1] - g.first[i], tile);
}

__device__ __forceinline__ void advance_one(const OptArgs& a) {
  if (a.kind == OPT_ADAM && a.beta_pow) {
    a.beta_pow[0] *= a.beta1;
    a.beta_pow[1] *= a.beta2;
  }
  if (a.global_step && a.gs_inc) atomicAdd(a.global_step, a.gs_inc);
}

__global__ void opt_advance_kernel(OptArgs a) {
  if (threadIdx.x != 0) return;
  advance_one(a);
}

struct OptAdvanceSet {
  OptArgs o[OPT_GROUP_MAX];
  int n;
};
__global__ void opt_advance_reply_kernel(OptAdvanceSet g) {
  if (threadIdx.x != 0) return;
  for (int i = 0; i < g.n; ++i) advance_one(g.o[i]);
  if (g.o[g.n - 1].rep_slot) publish_reply(g.o[g.n - 1]);
}

__global__ void epoch_signal_kernel(int* ctr) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
void launch_epoch_signal(int* ctr, hipStream_t s) { hipLaunchKernelGGL(epoch_signal_kernel, dim3(1), dim3(64), 0, s, ctr); }

static int apply_blocks(const OptArgs& a) {
  int blocks = a.nwork < 2048 ? a.nwork : 2048;
  return blocks < 1 ? 1 : blocks;
}

static void check_sched(const OptArgs& a) {
  if (a.sched && !a.global_step) throw std::runtime_error("apply_gradients: a learning-rate schedule needs a global_step");
  if (a.nesterov && a.kind != OPT_MOMENTUM)
    throw std::runtime_error("apply_gradients: nesterov is for the momentum optimizer");
  if (a.seg_lr && a.kind != OPT_MOMENTUM)
    throw std::runtime_error("apply_gradients: a per-segment rate (seg_lr) is for the momentum optimizer");
}

// the instantiation of a launch: WD when some segment decays, NAG (momentum only) when some optimizer
// of the launch uses Nesterov momentum; neither: the kernel as it was before either existed
template <bool WD, bool NAG>
static void launch_group(const OptGroup& g, dim3 grid, hipStream_t s) {
  const dim3 blk(256);
  switch (g.o[0].kind) {
    case OPT_SGD: hipLaunchKernelGGL((apply_gradients_group_kernel<OPT_SGD, WD, false>), grid, blk, 0, s, g); break;
    case OPT_MOMENTUM: hipLaunchKernelGGL((apply_gradients_group_kernel<OPT_MOMENTUM, WD, NAG>), grid, blk, 0, s, g); break;
    case OPT_ADAM: hipLaunchKernelGGL((apply_gradients_group_kernel<OPT_ADAM, WD, false>), grid, blk, 0, s, g); break;
    default: hipLaunchKernelGGL((apply_gradients_group_kernel<OPT_RMSPROP, WD, false>), grid, blk, 0, s, g); break;
  }
}

template <bool WD, bool NAG, bool EMA>
static void launch_one(const OptArgs& a, int blocks, hipStream_t s) {
  const dim3 grid(blocks), blk(256);
  switch (a.kind) {
    case OPT_SGD: hipLaunchKernelGGL((apply_gradients_kernel<OPT_SGD, WD, false, EMA>), grid, blk, 0, s, a); break;
    case OPT_MOMENTUM:
      if (a.seg_lr) hipLaunchKernelGGL((apply_gradients_kernel<OPT_MOMENTUM, WD, NAG, EMA, true>), grid, blk, 0, s, a);
      else hipLaunchKernelGGL((apply_gradients_kernel<OPT_MOMENTUM, WD, NAG, EMA>), grid, blk, 0, s, a);
      break;
    case OPT_ADAM: hipLaunchKernelGGL((apply_gradients_kernel<OPT_ADAM, WD, false, EMA>), grid, blk, 0, s, a); break;
    default: hipLaunchKernelGGL((apply_gradients_kernel<OPT_RMSPROP, WD, false, EMA>), grid, blk, 0, s, a); break;
  }
}
template <bool EMA>
static void launch_one_recipe(const OptArgs& a, int blocks, hipStream_t s) {
  if (a.decay) a.nesterov ? launch_one<true, true, EMA>(a, blocks, s) : launch_one<true, false, EMA>(a, blocks, s);
  else a.nesterov ? launch_one<false, true, EMA>(a, blocks, s) : launch_one<false, false, EMA>(a, blocks, s);
}

// an EMA's decay follows the optimizer's own step and every element's one update: no partial applies, no
// second destinations of a ps reply
static void check_ema(const OptArgs& a) {
  if (!a.ema) return;
  if (!(a.ema_decay >= 0.f && a.ema_decay < 1.f)) throw std::runtime_error("apply_gradients: ema_decay lies in [0, 1)");
  if (a.ema_num_updates && !a.global_step)
    throw std::runtime_error("apply_gradients: ema_num_updates needs a global_step");
  if (a.skip_advance) throw std::runtime_error("apply_gradients: an EMA cannot be combined with skip_advance");
  if (a.rep_slot) throw std::runtime_error("apply_gradients: an EMA cannot be combined with a ps reply");
}

void launch_apply_gradients_group(const OptArgs* o, int n, hipStream_t s) {
  if (n < 1 || n > OPT_GROUP_MAX) throw std::runtime_error("apply_gradients_group: 1..4 optimizers");
  // the group kernels have no EMA instantiation and none with a per-segment rate
  if (n == 1 && (o[0].ema || o[0].seg_lr)) return launch_apply_gradients(o[0], s);
  OptGroup g{};
  g.n = n;
  g.first[0] = 0;
  bool decay = false, nag = false;
  for (int i = 0; i < n; ++i) {
    if (o[i].kind != o[0].kind) throw std::runtime_error("apply_gradients_group: one optimizer kind per launch");
    check_sched(o[i]);
    if (o[i].sched && n > 1)
      throw std::runtime_error("apply_gradients_group: an optimizer with a schedule takes a launch of its own");
    if (o[i].ema && n > 1)
      throw std::runtime_error("apply_gradients_group: an optimizer with an EMA takes a launch of its own");
    if (o[i].seg_lr && n > 1)
      throw std::runtime_error("apply_gradients_group: an optimizer with a per-segment rate takes a launch of its own");
    decay = decay || o[i].decay;
    nag = nag || o[i].nesterov;
    g.o[i] = o[i];
    g.first[i + 1] = g.first[i] + apply_blocks(o[i]);
  }
  const dim3 grid(g.first[n]);
  if (decay) nag ? launch_group<true, true>(g, grid, s) : launch_group<true, false>(g, grid, s);
  else nag ? launch_group<false, true>(g, grid, s) : launch_group<false, false>(g, grid, s);
}

void launch_opt_advance(const OptArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(opt_advance_kernel, dim3(1), dim3(64), 0, s, a);
}

void launch_opt_advance_reply(const OptArgs* a, int n, hipStream_t s) {
  if (n < 1 || n > OPT_GROUP_MAX) throw std::runtime_error("opt_advance_reply: 1..4 optimizers");
  OptAdvanceSet g{};
  for (int i = 0; i < n; ++i) g.o[i] = a[i];
  g.n = n;
  hipLaunchKernelGGL(opt_advance_reply_kernel, dim3(1), dim3(64), 0, s, g);
}

void launch_apply_gradients(const OptArgs& a, hipStream_t s) {
  check_sched(a);
  check_ema(a);
  const int blocks = apply_blocks(a);
  if (a.ema) launch_one_recipe<true>(a, blocks, s);
  else launch_one_recipe<false>(a, blocks, s);
}

// Exchanges the masters of a var list with their EMA shadows and rewrites the bf16 working copies from
// the new masters, over the optimizer's own plan: flat ranges with 16-byte loads and stores, transposed
// variables through the LDS tile as the apply lays them out (copy = f2bf(master), the apply's invariant).
// Every element belongs to one work item and nothing is handed between workgroups: no counters, no step.
__global__ __launch_bounds__(256) void ema_swap_kernel(OptArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 tile[64][66];
  for (int wi = blockIdx.x; wi < a.nwork; wi += gridDim.x) {
    const OptWork w = a.work[wi];
    const OptSeg sg = a.segs[w.seg];
    if (w.kind == 0) {
      const long base = sg.off + w.start;
      const long n4 = ((base & 3) == 0) ? (w.count / 4) * 4 : 0;
      for (long j = threadIdx.x * 4; j < n4; j += 256 * 4) {
        const f32x4_t p = *reinterpret_cast<const f32x4_t*>(a.p + base + j);
        const f32x4_t e = *reinterpret_cast<const f32x4_t*>(a.ema + base + j);
        *reinterpret_cast<f32x4_t*>(a.p + base + j) = e;
        *reinterpret_cast<f32x4_t*>(a.ema + base + j) = p;
        store_copies(e, sg.w16 ? sg.w16 + w.start + j : nullptr, nullptr, nullptr);
      }
      for (long j = n4 + threadIdx.x; j < w.count; j += 256) {
        const long li = w.start + j, i = sg.off + li;
        const float p = a.p[i], e = a.ema[i];
        a.p[i] = e;
        a.ema[i] = p;
        if (sg.w16) sg.w16[li] = f2bf(e);
      }
    } else {
      const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
      const int c = w.c0 + tx;
      float pv[16], ev[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int r = w.r0 + ty + 4 * u;
        // out-of-tile lanes load the segment's first element (never stored), as in the apply
        const bool ok = r < sg.R && c < sg.C;
        const long i = sg.off + (ok ? ((long)r * sg.T + w.t) * sg.C + c : 0);
        pv[u] = a.p[i];
        ev[u] = a.ema[i];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int rr = ty + 4 * u, r = w.r0 + rr;
        if (r < sg.R && c < sg.C) {
          const long li = ((long)r * sg.T + w.t) * sg.C + c, i = sg.off + li;
          a.p[i] = ev[u];
          a.ema[i] = pv[u];
          const bf16 b = f2bf(ev[u]);
          if (sg.w16) sg.w16[li] = b;
          tile[rr][tx] = b;
        }
      }
      __syncthreads();
      for (int cc = ty; cc < 64; cc += 4) {
        const int c = w.c0 + cc, r = w.r0 + tx;
        if (r < sg.R && c < sg.C && sg.wt16) sg.wt16[((long)c * sg.T + w.t) * sg.R + r] = tile[tx][cc];
      }
      __syncthreads();
    }
  }
}

void launch_ema_swap(const OptArgs& a, hipStream_t s) {
  if (!a.ema) throw std::runtime_error("ema_swap: the optimizer has no EMA");
  if (a.nwork < 1) return;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(apply_blocks(a)), dim3(256), 0, s, a);
}

}  // namespace dtfe
