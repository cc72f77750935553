// Bidirectional GRU layer (TF1 tf.nn.bidirectional_dynamic_rnn(GRUCell(128), GRUCell(128), x)): both directions of
// the layer in ONE persistent launch, forward and BPTT.
//
// gru_seq.hip's kernels give a workgroup 16 batch rows for the whole sequence and never let it talk to another
// workgroup, so at B = 128 a recurrence launch occupies 8 CUs.  The two directions of a bidirectional layer are
// independent recurrences over the same input: here the grid is (B / 16, 2), blockIdx.y = d is the direction, and the
// second direction runs on CUs the first leaves idle.  d selects the weights, the step order and the row each h goes to:
//
//   d = 0  forward in time:   steps t = 0..T-1,  h_{-1} in the h columns of xh[0][0],   h_t   -> h columns of xh[0][t+1]
//   d = 1  backward in time:  steps t = T-1..0,  h_T    in the h columns of xh[1][T-1], h_t   -> h columns of xh[1][t-1]
//
// so row t of every buffer of direction d belongs to time t and xh[d][t] = [x_t | the state step t starts from].  The
// caller stages x_t once, in xh[0]; the d = 1 workgroups read it there and write it into the x columns of xh[1][t]
// and xrh[1][t] (the weight gradients read whole rows).  Direction 1 only reads x columns of xh[0], direction 0 only
// writes h columns of it, and neither writes an initial-state column: the launch needs no order between the two.
// The final states go to feat [B][2H]: d = 0's (after time T-1) in columns 0..H-1, d = 1's (after time 0) in H..2H-1.
//
// Ownership as gru_seq.hip: a workgroup of 1024 threads (16 waves) per (16 rows, direction) for all T steps, no flags,
// no spin loops, every weight the recurrence multiplies by loaded ONCE as v_mfma_f32_16x16x4_f32 B fragments.
//
// forward, per step (3 barriers) - the phases of gru_seq_fwd_kernel with the tiles split by how they are read:
//   x_t has its own tile Xs (pitch 29, scalar reads down the rows), h and r * h live in Hs / RH with 16-byte rows, and
//   the recurrent rows of both kernels are loaded so that lane group g supplies k = 16 q + 4 g + e of MFMA step (q, e):
//   one 16-byte LDS read feeds 4 MFMAs, 7 + 8 LDS reads for the gate GEMM (k = 156) instead of 39 and 4 instead of 16
//   for each half of the candidate's recurrent part.  59 weight VGPRs per lane (7 + 32 gate, 4 + 16 candidate).
//   A   gates over [x_t | h] (wave w: gate columns 16 w .. + 16; waves 0-7 r, 8-15 u) and, before the barrier, this
//       wave's share of x_t . Wc_x;  r * h -> RH, xrh;  u -> Us
//   B   candidate: wave w takes column tile w % 8 and k half w / 8 of the recurrent rows, partial -> P[half]
//   C   one thread per (row, unit) pair, 2 pairs per thread: c = tanh(P0 + P1 + bc), h' = u h + (1 - u) c -> cand, Hs,
//       the h columns of the next step's xh row (or feat)
//   x of the next step is prefetched under the current one.
//
// backward, per step in the reverse of the direction's forward order (4 barriers), dh carried on chip - the phases
// a-d of gru_seq.hip's BPTT.  Each direction starts from its half of d loss / d feat: dhT [B][2H] columns
// d H .. d H + H - 1, or dl . wo[d H : (d + 1) H]^T formed here from the head's dlogits.
//
// The kernel and bias gradients are four wgrad_tallk launches over (xh[d], dgg[d]) and (xrh[d], dgc[d]).
#include "gru_seq.h"

#include "common.h"

namespace dtfe {

namespace {

constexpr int LR = 16;      // batch rows per workgroup (one MFMA row tile)
constexpr int GH = 128;     // hidden units
constexpr int GI = 28;      // inputs per step
constexpr int KT = GI + GH; // rows of both kernels, pitch of xh / xrh
constexpr int XK = GI / 4;  // x k-steps of the gate GEMM
constexpr int XS = 4;       // x k-steps of the candidate per wave half (half 0: steps 0-3, half 1: steps 3-6, 3 zeroed)
constexpr int NQ = LR * GH / 1024;  // (row, unit) pairs per thread
constexpr int XP = GI + 1;  // Xs pitch (scalar reads down the rows: odd)
constexpr int RP = GH + 1;  // Us pitch
constexpr int DP = GH + 4;  // 16-byte rows for vector reads
constexpr int DGP = 2 * GH + 4;

__global__ __launch_bounds__(1024) void gru_bidir_fwd_kernel(GruBidirArgs a) {
  __shared__ float Xs[LR * XP];                               // x_t
  __shared__ __attribute__((aligned(16))) float Hs[LR * DP];  // the state step t starts from
  __shared__ __attribute__((aligned(16))) float RH[LR * DP];  // r * h
  __shared__ float Us[LR * RP];                               // u
  __shared__ float P[2][LR * GH];                             // candidate partials of the two k halves
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, d = blockIdx.y, B = a.B, T = a.T;
  const int mrow = lane & 15, g = lane >> 4;
  const int tile = w & 7, half = w >> 3;
  const long TB = (long)T * B;
  // this direction's slices; x is always read from direction 0's xh
  float* const xh_d = a.xh + d * TB * KT;
  float* const xrh_d = a.xrh + d * TB * KT;
  float* const g_d = a.g + d * TB * (2 * GH);
  float* const cand_d = a.cand + d * TB * GH;
  const float* const Wg = a.Wg[d];
  const float* const Wc = a.Wc[d];
  // weights: loaded once, register-resident for all T steps
  float wgx[XK], wcx[XS];
  f32x4_t wgh[8], wch[4];
  {
    const float* p = Wg + 16 * w + mrow;
#pragma unroll
    for (int kk = 0; kk < XK; ++kk) wgx[kk] = p[(long)(4 * kk + g) * (2 * GH)];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) wgh[k][e] = p[(long)(GI + 16 * k + 4 * g + e) * (2 * GH)];
    const float* q = Wc + 16 * tile + mrow;
#pragma unroll
    for (int j = 0; j < XS; ++j) {
      const int kk = 3 * half + j;  // half 1 starts at step 3, which half 0 owns: zero there
      wcx[j] = (half == 1 && j == 0) ? 0.f : q[(long)(4 * kk + g) * GH];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) wch[k][e] = q[(long)(GI + 64 * half + 16 * k + 4 * g + e) * GH];
  }
  const float bgate = a.bg[d][16 * w + mrow];
  const int t0 = d ? T - 1 : 0, dt = d ? -1 : 1;
  // h: NQ (row, unit) pairs per thread, in registers and in Hs
  float hreg[NQ], bcand[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
    hreg[q] = xh_d[((long)t0 * B + r0 + r) * KT + GI + u];  // the initial state
    Hs[r * DP + u] = hreg[q];
    bcand[q] = a.bc[d][u];
  }
  // x_t: one element per thread (LR * GI = 448), a step ahead
  const bool xl = tid < LR * GI;
  const int xr = xl ? tid / GI : 0, xk = xl ? tid - xr * GI : 0;
  // every address of a step is a workgroup-uniform base (row_t) plus one of these small per-thread offsets
  const unsigned ox = xr * KT + xk;                            // this thread's x element
  const unsigned og = 4 * g * (2 * GH) + 16 * w + mrow;        // accumulator rows 4 g + e, gate column 16 w + mrow
  const unsigned orh = 4 * g * KT + GI + 16 * w + mrow;        // the same element's r * h in xrh (waves 0-7)
  float xnext = xl ? (a.xh + ((long)t0 * B + r0) * KT)[ox] : 0.f;
  for (int s = 0; s < T; ++s) {
    const int t = t0 + dt * s;
    const long row_t = (long)t * B + r0, row_n = row_t + (long)dt * B;  // this step's rows, the next step's
    const bool more = s + 1 < T;
    float* const xrh_t = xrh_d + row_t * KT;
    if (xl) {
      Xs[xr * XP + xk] = xnext;
      xrh_t[ox] = xnext;
      if (d) (xh_d + row_t * KT)[ox] = xnext;
    }
    __syncthreads();
    if (more && xl) xnext = (a.xh + row_n * KT)[ox];
    // ---- phase A: gates, and the x part of the candidate
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, accc = {0.f, 0.f, 0.f, 0.f};
    {
      const float* xrow = Xs + mrow * XP + g;
#pragma unroll
      for (int kk = 0; kk < XK; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xrow[4 * kk], wgx[kk], acc, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < XS; ++j)
        accc = __builtin_amdgcn_mfma_f32_16x16x4f32(xrow[4 * (3 * half + j)], wcx[j], accc, 0, 0, 0);
      const float* hrow = Hs + mrow * DP + 4 * g;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(hrow + 16 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wgh[k][e], acc, 0, 0, 0);
      }
      const int col = 16 * w + mrow;  // 0..127 r, 128..255 u
      float* const g_t = g_d + row_t * (2 * GH);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const float v = sigmoidf_(acc[e] + bgate);
        g_t[og + e * (2 * GH)] = v;
        if (w < 8) {
          const float rh = v * Hs[r * DP + col];
          RH[r * DP + col] = rh;
          xrh_t[orh + e * KT] = rh;
        } else {
          Us[r * RP + col - GH] = v;
        }
      }
    }
    __syncthreads();
    // ---- phase B: the recurrent part of the candidate, this wave's k half
    {
      const float* rrow = RH + mrow * DP + 64 * half + 4 * g;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(rrow + 16 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) accc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wch[k][e], accc, 0, 0, 0);
      }
      float* pp = P[half] + 16 * tile + mrow;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[(4 * g + e) * GH] = accc[e];
    }
    __syncthreads();
    // ---- phase C: candidate activation and the state update
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const float c = tanhf(P[0][p] + P[1][p] + bcand[q]);
      const float uu = Us[r * RP + u];
      const float h = uu * hreg[q] + (1.f - uu) * c;
      hreg[q] = h;
      (cand_d + row_t * GH)[(unsigned)p] = c;
      Hs[r * DP + u] = h;
      if (more) (xh_d + row_n * KT)[(unsigned)(r * KT + GI + u)] = h;
      else (a.feat + (long)r0 * (2 * GH) + d * GH)[(unsigned)(r * (2 * GH) + u)] = h;
    }
    // (the next step's barrier orders these Hs writes before its reads; its Xs write touches a tile last read in
    // phase A, and its phase A writes of RH / Us come after this step's reads)
  }
}

// this direction's half of d loss / d feat at (row, unit)
__device__ __forceinline__ float dfeat_of(const GruBidirArgs& a, int d, int row, int u) {
  if (!a.dl) return a.dhT[(long)row * (2 * GH) + d * GH + u];
  const float* wrow = a.wo + (long)(d * GH + u) * a.nc;
  float s = 0.f;
  for (int c = 0; c < a.nc; ++c) s = __builtin_fmaf(a.dl[(long)row * a.nc + c], wrow[c], s);
  return s;
}

__global__ __launch_bounds__(1024) void gru_bidir_bwd_kernel(GruBidirArgs a) {
  __shared__ __attribute__((aligned(16))) float DG[LR * DGP];  // [dr~ | du~]
  __shared__ __attribute__((aligned(16))) float DC[LR * DP];   // dc~
  __shared__ float P[2][LR * GH];  // GEMM partials of the two k halves: drh (b -> c), then the carried dh (d -> a)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, d = blockIdx.y, B = a.B, T = a.T;
  const int mrow = lane & 15, g = lane >> 4;
  const int tile = w & 7, half = w >> 3;
  const long TB = (long)T * B;
  const float* const xh_d = a.xh + d * TB * KT;
  const float* const g_d = a.g + d * TB * (2 * GH);
  const float* const cand_d = a.cand + d * TB * GH;
  float* const dgg_d = a.dgg + d * TB * (2 * GH);
  float* const dgc_d = a.dgc + d * TB * GH;
  // transposed recurrent weights of this wave's 16 units and k half: lane group g supplies k = 16 q + 4 g + e of
  // MFMA step (q, e), so one 16-byte load / LDS read feeds 4 steps
  f32x4_t kc[4], ku[4], kr[4];
  {
    const int unit = 16 * tile + mrow;
    const float* pc = a.Wc[d] + (long)(GI + unit) * GH + 64 * half + 4 * g;
    const float* pg = a.Wg[d] + (long)(GI + unit) * (2 * GH) + 64 * half + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      kc[q] = *reinterpret_cast<const f32x4_t*>(pc + 16 * q);
      kr[q] = *reinterpret_cast<const f32x4_t*>(pg + 16 * q);
      ku[q] = *reinterpret_cast<const f32x4_t*>(pg + GH + 16 * q);
    }
  }
  float carry[NQ], sr[NQ], su[NQ], sc[NQ], sh[NQ];  // the current step's saved r, u, c and the state it started from
  auto fetch = [&](int t) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const long row = (long)t * B + r0 + r;
      sr[q] = g_d[row * (2 * GH) + u];
      su[q] = g_d[row * (2 * GH) + GH + u];
      sc[q] = cand_d[row * GH + u];
      sh[q] = xh_d[row * KT + GI + u];
    }
  };
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = tid + 1024 * q;
    P[0][p] = dfeat_of(a, d, r0 + p / GH, p % GH);
    P[1][p] = 0.f;
    carry[q] = 0.f;
  }
  // the reverse of the direction's forward order: d = 0 from T-1 down, d = 1 from 0 up
  const int t0 = d ? 0 : T - 1, dt = d ? 1 : -1;
  fetch(t0);
  __syncthreads();
  for (int s = 0; s < T; ++s) {
    const int t = t0 + dt * s;
    const long row_t = (long)t * B + r0;
    const bool more = s + 1 < T;
    // ---- a: the two gradients that need only dh
    float vr[NQ], vh[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const float rr = sr[q], uu = su[q], c = sc[q], h = sh[q];
      const float dh = carry[q] + P[0][p] + P[1][p];
      const float dc = dh * (1.f - uu) * (1.f - c * c);
      const float du = dh * (h - c) * uu * (1.f - uu);
      DC[r * DP + u] = dc;
      DG[r * DGP + GH + u] = du;
      dgc_d[(row_t + r) * GH + u] = dc;
      dgg_d[(row_t + r) * (2 * GH) + GH + u] = du;
      carry[q] = dh * uu;
      vr[q] = rr;
      vh[q] = h;
    }
    if (more) fetch(t + dt);
    __syncthreads();
    // ---- b: GEMM 1 (drh partial of this k half) and the du~ half of GEMM 2
    f32x4_t acc2 = {0.f, 0.f, 0.f, 0.f};
    {
      f32x4_t acc1 = {0.f, 0.f, 0.f, 0.f};
      const float* crow = DC + mrow * DP + 64 * half + 4 * g;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(crow + 16 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], kc[q][e], acc1, 0, 0, 0);
      }
      float* pp = P[half] + 16 * tile + mrow;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[(4 * g + e) * GH] = acc1[e];
      if (more) {
        const float* urow = DG + mrow * DGP + GH + 64 * half + 4 * g;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4_t av = *reinterpret_cast<const f32x4_t*>(urow + 16 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], ku[q][e], acc2, 0, 0, 0);
        }
      }
    }
    __syncthreads();
    // ---- c: the reset gate's gradient
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const float drh = P[0][p] + P[1][p];
      const float dr = drh * vh[q] * vr[q] * (1.f - vr[q]);
      DG[r * DGP + u] = dr;
      dgg_d[(row_t + r) * (2 * GH) + u] = dr;
      carry[q] += drh * vr[q];
    }
    if (!more) break;
    __syncthreads();
    // ---- d: the dependent half of GEMM 2
    {
      const float* rrow = DG + mrow * DGP + 64 * half + 4 * g;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(rrow + 16 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], kr[q][e], acc2, 0, 0, 0);
      }
      float* pp = P[half] + 16 * tile + mrow;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[(4 * g + e) * GH] = acc2[e];
    }
    __syncthreads();
  }
}

bool covered(const GruBidirArgs& a) { return a.H == GH && a.I == GI && a.T >= 1 && a.B >= LR && a.B % LR == 0; }

}  // namespace

bool launch_gru_bidir_fwd(const GruBidirArgs& a, hipStream_t s) {
  if (!covered(a)) return false;
  hipLaunchKernelGGL(gru_bidir_fwd_kernel, dim3(a.B / LR, 2), dim3(1024), 0, s, a);
  return true;
}

bool launch_gru_bidir_bwd(const GruBidirArgs& a, hipStream_t s) {
  if (!covered(a)) return false;
  hipLaunchKernelGGL(gru_bidir_bwd_kernel, dim3(a.B / LR, 2), dim3(1024), 0, s, a);
  return true;
}

}  // namespace dtfe
