// Persistent whole-sequence GRU kernels (TF1 tf.nn.rnn_cell.GRUCell, default arguments).
//
//   [r | u] = sigmoid([x_t | h] . Wg + bg)      c = tanh([x_t | r * h] . Wc + bc)      h' = u * h + (1 - u) * c
//
// Unlike the LSTM step (one GEMM), a GRU step is TWO DEPENDENT GEMMs with an elementwise product between
// them - and so is its backward step, in the other order - so these kernels have a data flow of their own.
// What they share with lstm_seq.hip's single-workgroup kernels is the ownership: ONE launch runs the whole
// recurrence, a workgroup of 1024 threads (16 waves) owns 16 batch rows for all T steps and never waits on
// another workgroup (no flags, no spin loops, no co-residency requirement), and every weight the recurrence
// multiplies by is loaded ONCE into VGPRs as v_mfma_f32_16x16x4_f32 B fragments (exact fp32).
//
// forward, per step t (3 barriers):
//   A   As = [x_t | h_{t-1}] (16 x 156, LDS).  Wave w owns gate columns 16 w .. + 16 of Wg (156 x 256: 39
//       k-steps = 39 VGPRs): waves 0-7 produce r, waves 8-15 produce u.  Next to the gate GEMM, BEFORE the
//       barrier, every wave also accumulates its share of x_t . Wc_x (k = 28), the only part of the candidate
//       that does not depend on r: the dependent chain of a step is then gate GEMM (k = 156) -> sigmoid ->
//       r * h -> candidate GEMM over k = 128 only.  The r waves form r * h from the h columns of As and write it
//       to the RH tile (LDS) and xrh (HBM); the u waves park u in LDS for phase C.
//   B   the candidate has 8 column tiles for 16 waves: wave w takes tile w % 8 and k half w / 8 of the recurrent
//       rows (64 of 128: 16 k-steps; the x rows are split 4 + 3 k-steps the same way), continues the accumulator
//       it started in phase A and leaves its partial in P[half] (LDS).  59 weight VGPRs per lane in all.
//   C   one thread per (row, unit) pair, 2 pairs per thread, h in registers: c = tanh(P0 + P1 + bc),
//       h' = u h + (1 - u) c -> cand, the h columns of As and of xh[t + 1] (or hT).
//   x_{t+1} is prefetched under step t; its thread also copies x_t into xrh (the weight gradient reads it there).
//
// backward, per step t = T-1..0 (4 barriers), dh carried on chip:
//   a   dh = carry + P0 + P1;  dc~ = dh (1 - u)(1 - c^2),  du~ = dh (h - c) u (1 - u)  -> LDS + dgc / dgg
//   b   GEMM 1: drh = dc~ . Wc_h^T (k = 128 split over the two wave halves, partials in P).  du~ . Wg_h[:, u]^T,
//       the half of GEMM 2 that does not depend on GEMM 1, is accumulated here too and stays in registers.
//   c   drh = P0 + P1;  dr~ = drh h r (1 - r) -> LDS + dgg;  carry = dh u + drh r
//   d   GEMM 2, dependent part: += dr~ . Wg_h[:, r]^T -> P.  48 weight VGPRs per lane (16 + 16 + 16).
//   Step t - 1's saved r, u, c, h are loaded while step t computes.
//
// The kernel and bias gradients are two wgrad_tallk launches over (xh, dgg) and (xrh, dgc).
//
// Stacked layers (a GRU cell whose input is the h sequence of the cell below) add two kernels on the same ownership:
// gru_proj_fwd_kernel, a forward whose x part was projected beforehand by throughput GEMMs (described at the kernel),
// and gru_stack_bwd_kernel, the backward above with the input width as an argument and dh += dhs[t] in phase a.  Both
// forward kernels can also write every h_t straight into the x columns of the next layer's xh (GruSeqArgs::h2).
#include "gru_seq.h"

#include "common.h"

namespace dtfe {

namespace {

constexpr int LR = 16;      // batch rows per workgroup (one MFMA row tile)
constexpr int GH = 128;     // hidden units
constexpr int GI = 28;      // inputs per step
constexpr int KT = GI + GH; // rows of both kernels
constexpr int KT4 = KT / 4; // gate k-steps
constexpr int XS = 4;       // x k-steps of the candidate per wave half (half 0: steps 0-3, half 1: steps 3-6, 3 zeroed)
constexpr int HS = GH / 8;  // recurrent k-steps per wave half
constexpr int NQ = LR * GH / 1024;  // (row, unit) pairs per thread
constexpr int AP = KT + 1;  // As pitch
constexpr int RP = GH + 1;  // RH / U pitch (scalar reads down the rows: odd)
constexpr int DP = GH + 4;  // backward tiles: 16-byte rows for vector reads
constexpr int DGP = 2 * GH + 4;

__device__ __forceinline__ float dh_t_of(const GruSeqArgs& a, int row, int u) {
  if (!a.dl) return a.dhT[(long)row * GH + u];
  float s = 0.f;
  for (int c = 0; c < a.nc; ++c) s = __builtin_fmaf(a.dl[(long)row * a.nc + c], a.wo[(long)u * a.nc + c], s);
  return s;
}

__global__ __launch_bounds__(1024) void gru_seq_fwd_kernel(GruSeqArgs a) {
  __shared__ float As[LR * AP];     // [x_t | h_{t-1}]
  __shared__ float RH[LR * RP];     // r * h_{t-1}
  __shared__ float Us[LR * RP];     // u
  __shared__ float P[2][LR * GH];   // candidate partials of the two k halves
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, B = a.B;
  const int mrow = lane & 15, g = lane >> 4;
  const int tile = w & 7, half = w >> 3;
  // weights: loaded once, register-resident for all T steps
  float wg[KT4], wcx[XS], wch[HS];
  {
    const float* p = a.Wg + 16 * w + mrow;
#pragma unroll
    for (int kk = 0; kk < KT4; ++kk) wg[kk] = p[(long)(4 * kk + g) * (2 * GH)];
    const float* q = a.Wc + 16 * tile + mrow;
#pragma unroll
    for (int j = 0; j < XS; ++j) {
      const int kk = 3 * half + j;  // half 1 starts at step 3, which half 0 owns: zero there
      wcx[j] = (half == 1 && j == 0) ? 0.f : q[(long)(4 * kk + g) * GH];
    }
#pragma unroll
    for (int kk = 0; kk < HS; ++kk) wch[kk] = q[(long)(GI + 64 * half + 4 * kk + g) * GH];
  }
  const float bgate = a.bg[16 * w + mrow];
  // h: NQ (row, unit) pairs per thread, in registers and in the A tile
  float hreg[NQ], bcand[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
    hreg[q] = a.xh[(long)(r0 + r) * KT + GI + u];   // h_{-1}
    As[r * AP + GI + u] = hreg[q];
    bcand[q] = a.bc[u];
  }
  // x_t: one element per thread (LR * GI = 448), a step ahead
  const bool xl = tid < LR * GI;
  const int xr = xl ? tid / GI : 0, xk = xl ? tid - xr * GI : 0;
  float xnext = xl ? a.xh[(long)(r0 + xr) * KT + xk] : 0.f;
  for (int t = 0; t < a.T; ++t) {
    const long row_t = (long)t * B + r0;
    if (xl) {
      As[xr * AP + xk] = xnext;
      a.xrh[(row_t + xr) * KT + xk] = xnext;
    }
    __syncthreads();
    if (t + 1 < a.T && xl) xnext = a.xh[(row_t + B + xr) * KT + xk];
    // ---- phase A: gates, and the x part of the candidate
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, accc = {0.f, 0.f, 0.f, 0.f};
    const float* arow = As + mrow * AP + g;
#pragma unroll
    for (int kk = 0; kk < KT4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * kk], wg[kk], acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < XS; ++j)
      accc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * (3 * half + j)], wcx[j], accc, 0, 0, 0);
    {
      const int col = 16 * w + mrow;  // 0..127 r, 128..255 u
      float* g_t = a.g + row_t * (2 * GH) + col;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const float v = sigmoidf_(acc[e] + bgate);
        g_t[(long)r * (2 * GH)] = v;
        if (w < 8) {
          const float rh = v * As[r * AP + GI + col];
          RH[r * RP + col] = rh;
          a.xrh[(row_t + r) * KT + GI + col] = rh;
        } else {
          Us[r * RP + col - GH] = v;
        }
      }
    }
    __syncthreads();
    // ---- phase B: the recurrent part of the candidate, this wave's k half
    {
      const float* rrow = RH + mrow * RP + 64 * half + g;
#pragma unroll
      for (int kk = 0; kk < HS; ++kk) accc = __builtin_amdgcn_mfma_f32_16x16x4f32(rrow[4 * kk], wch[kk], accc, 0, 0, 0);
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
      a.cand[(row_t + r) * GH + u] = c;
      As[r * AP + GI + u] = h;
      if (t + 1 < a.T) a.xh[(row_t + B + r) * KT + GI + u] = h;
      else a.hT[(long)(r0 + r) * GH + u] = h;
      if (a.h2) a.h2[(row_t + r) * a.h2p + u] = h;
    }
    // (the next step's x write touches only the x columns of As, last read in phase A; its barrier orders the rest)
  }
}

// The forward of a layer whose whole input sequence exists before it starts (a stacked layer): the x part of both
// GEMMs was hoisted into two throughput GEMMs over all T * B rows and arrives as xpg / xpc (biases folded in), so a
// step is gate GEMM (k = 128) -> sigmoid -> r * h -> candidate GEMM (k = 128 over the two wave halves) and phase A
// has no x work.  Same ownership as gru_seq_fwd_kernel; the data flow differs:
//   - only the recurrent rows are register-resident: 32 + 16 = 48 weight VGPRs per lane, whatever I is;
//   - the accumulators of step t START from this wave's xpg[t] / xpc[t] tile (half 1 of the candidate from zero, so the
//     projection counts once), each fetched as soon as step t - 1 has consumed its own, two barriers ahead of its use;
//   - h and r * h are read from LDS as 16-byte vectors: lane group g supplies k = 16 q + 4 g + e of MFMA step (q, e)
//     (the weights are loaded in the same order), 8 + 4 LDS reads per step instead of 32 + 16;
//   - the x columns of xrh[t] are copied from xh[t] by the u waves, which have no r * h work in phase A.
__global__ __launch_bounds__(1024) void gru_proj_fwd_kernel(GruSeqArgs a) {
  __shared__ __attribute__((aligned(16))) float Hs[LR * DP];  // h_{t-1}
  __shared__ __attribute__((aligned(16))) float RH[LR * DP];  // r * h_{t-1}
  __shared__ float Us[LR * RP];                               // u
  __shared__ float P[2][LR * GH];                             // candidate partials of the two k halves
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, B = a.B, I = a.I, kt = I + GH, I4 = I / 4;
  const int mrow = lane & 15, g = lane >> 4;
  const int tile = w & 7, half = w >> 3;
  f32x4_t wg[8], wc[4];
  {
    const float* p = a.Wg + (long)(I + 4 * g) * (2 * GH) + 16 * w + mrow;
    const float* q = a.Wc + (long)(I + 64 * half + 4 * g) * GH + 16 * tile + mrow;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) wg[k][e] = p[(long)(16 * k + e) * (2 * GH)];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) wc[k][e] = q[(long)(16 * k + e) * GH];
  }
  float hreg[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
    hreg[q] = a.xh[(long)(r0 + r) * kt + I + u];  // h_{-1}
    Hs[r * DP + u] = hreg[q];
  }
  // every address of a step is a workgroup-uniform base (row_t) plus one of these small per-thread offsets.
  // This wave's accumulator tiles: rows 4 g + e, gate column 16 w + mrow, candidate column 16 tile + mrow
  const unsigned og = 4 * g * (2 * GH) + 16 * w + mrow, oc = 4 * g * GH + 16 * tile + mrow;
  f32x4_t gnext, cnext = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    gnext[e] = (a.xpg + (long)r0 * (2 * GH))[og + e * (2 * GH)];
    if (half == 0) cnext[e] = (a.xpc + (long)r0 * GH)[oc + e * GH];
  }
  for (int t = 0; t < a.T; ++t) {
    const long row_t = (long)t * B + r0;
    float* const g_t = a.g + row_t * (2 * GH);
    float* const xrh_t = a.xrh + row_t * kt;
    const float* const xh_t = a.xh + row_t * kt;
    f32x4_t acc = gnext;
    __syncthreads();
    // ---- phase A: gates
    {
      const float* hrow = Hs + mrow * DP + 4 * g;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(hrow + 16 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wg[k][e], acc, 0, 0, 0);
      }
      const int col = 16 * w + mrow;  // 0..127 r, 128..255 u
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const float v = sigmoidf_(acc[e]);
        g_t[og + e * (2 * GH)] = v;
        if (w < 8) {
          const float rh = v * Hs[r * DP + col];
          RH[r * DP + col] = rh;
          xrh_t[(unsigned)(r * kt + I + col)] = rh;
        } else {
          Us[r * RP + col - GH] = v;
        }
      }
      if (w >= 8) {  // x_t -> xrh (the candidate's weight gradient reads it there)
        for (int i = tid - 512; i < LR * I4; i += 512) {
          const int r = i / I4;
          const unsigned o = r * kt + 4 * (i - r * I4);
          *reinterpret_cast<f32x4_t*>(xrh_t + o) = *reinterpret_cast<const f32x4_t*>(xh_t + o);
        }
      }
    }
    __syncthreads();
    // ---- phase B: the candidate, this wave's k half (and the next step's gate tile, now that this one's is used)
    f32x4_t accc = cnext;
    if (t + 1 < a.T) {
#pragma unroll
      for (int e = 0; e < 4; ++e) gnext[e] = (a.xpg + (row_t + B) * (2 * GH))[og + e * (2 * GH)];
    }
    {
      const float* rrow = RH + mrow * DP + 64 * half + 4 * g;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(rrow + 16 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) accc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wc[k][e], accc, 0, 0, 0);
      }
      float* pp = P[half] + 16 * tile + mrow;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[(4 * g + e) * GH] = accc[e];
    }
    __syncthreads();
    // ---- phase C: candidate activation and the state update (and the next step's candidate tile)
    if (t + 1 < a.T && half == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) cnext[e] = (a.xpc + (row_t + B) * GH)[oc + e * GH];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const float c = tanhf(P[0][p] + P[1][p]);
      const float uu = Us[r * RP + u];
      const float h = uu * hreg[q] + (1.f - uu) * c;
      hreg[q] = h;
      (a.cand + row_t * GH)[(unsigned)p] = c;
      Hs[r * DP + u] = h;
      if (t + 1 < a.T) (a.xh + (row_t + B) * kt)[(unsigned)(r * kt + I + u)] = h;
      else (a.hT + (long)r0 * GH)[(unsigned)p] = h;
      if (a.h2) (a.h2 + row_t * a.h2p)[(unsigned)(r * a.h2p + u)] = h;
    }
    // (the next step's first barrier orders these Hs writes before its reads, and its phase A writes of RH / Us
    // after this step's reads)
  }
}

// BPTT of one layer.  STACK false: the single layer's kernel (I = 28 a constant, one dh_T).  STACK true: I an
// argument (row offset I, xh pitch I + H) and an optional d loss / d h_t arriving at every step.
template <bool STACK>
__device__ __forceinline__ void gru_bwd_body(const GruSeqArgs& a) {
  __shared__ __attribute__((aligned(16))) float DG[LR * DGP];  // [dr~ | du~]
  __shared__ __attribute__((aligned(16))) float DC[LR * DP];   // dc~
  __shared__ float P[2][LR * GH];  // GEMM partials of the two k halves: drh (b -> c), then dh_{t-1} (d -> a)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, B = a.B, I = STACK ? a.I : GI, kt = I + GH;
  const int mrow = lane & 15, g = lane >> 4;
  const int tile = w & 7, half = w >> 3;
  // transposed recurrent weights of this wave's 16 units and k half: lane group g supplies k = 16 q + 4 g + e of
  // MFMA step (q, e), so one 16-byte load / LDS read feeds 4 steps
  f32x4_t kc[4], ku[4], kr[4];
  {
    const int unit = 16 * tile + mrow;
    const float* pc = a.Wc + (long)(I + unit) * GH + 64 * half + 4 * g;
    const float* pg = a.Wg + (long)(I + unit) * (2 * GH) + 64 * half + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      kc[q] = *reinterpret_cast<const f32x4_t*>(pc + 16 * q);
      kr[q] = *reinterpret_cast<const f32x4_t*>(pg + 16 * q);
      ku[q] = *reinterpret_cast<const f32x4_t*>(pg + GH + 16 * q);
    }
  }
  float carry[NQ], sr[NQ], su[NQ], sc[NQ], sh[NQ];  // step t's saved r, u, c, h_{t-1}
  float sd[NQ];                                      // STACK: step t's incoming dhs
  auto fetch = [&](int t) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const long row = (long)t * B + r0 + r;
      sr[q] = a.g[row * (2 * GH) + u];
      su[q] = a.g[row * (2 * GH) + GH + u];
      sc[q] = a.cand[row * GH + u];
      sh[q] = a.xh[row * kt + I + u];
      if (STACK) sd[q] = a.dhs ? a.dhs[row * GH + u] : 0.f;
    }
  };
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = tid + 1024 * q;
    P[0][p] = (!STACK || a.dl || a.dhT) ? dh_t_of(a, r0 + p / GH, p % GH) : 0.f;  // (a lower layer starts from zeros)
    P[1][p] = 0.f;
    carry[q] = 0.f;
  }
  fetch(a.T - 1);
  __syncthreads();
  for (int t = a.T - 1; t >= 0; --t) {
    const long row_t = (long)t * B + r0;
    // ---- a: the two gradients that need only dh
    float vr[NQ], vh[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = tid + 1024 * q, r = p / GH, u = p - r * GH;
      const float rr = sr[q], uu = su[q], c = sc[q], h = sh[q];
      float dh = carry[q] + P[0][p] + P[1][p];
      if (STACK) dh += sd[q];
      const float dc = dh * (1.f - uu) * (1.f - c * c);
      const float du = dh * (h - c) * uu * (1.f - uu);
      DC[r * DP + u] = dc;
      DG[r * DGP + GH + u] = du;
      a.dgc[(row_t + r) * GH + u] = dc;
      a.dgg[(row_t + r) * (2 * GH) + GH + u] = du;
      carry[q] = dh * uu;
      vr[q] = rr;
      vh[q] = h;
    }
    if (t > 0) fetch(t - 1);
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
      if (t > 0) {
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
      a.dgg[(row_t + r) * (2 * GH) + u] = dr;
      carry[q] += drh * vr[q];
    }
    if (t == 0) break;
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

__global__ __launch_bounds__(1024) void gru_seq_bwd_kernel(GruSeqArgs a) { gru_bwd_body<false>(a); }
__global__ __launch_bounds__(1024) void gru_stack_bwd_kernel(GruSeqArgs a) { gru_bwd_body<true>(a); }

bool covered(const GruSeqArgs& a) { return a.H == GH && a.I == GI && a.T >= 1 && a.B >= LR && a.B % LR == 0; }

bool covered_stack(const GruSeqArgs& a) {
  return a.H == GH && a.I >= 4 && a.I % 4 == 0 && a.T >= 1 && a.B >= LR && a.B % LR == 0;
}

}  // namespace

bool launch_gru_seq_fwd(const GruSeqArgs& a, hipStream_t s) {
  if (!covered(a)) return false;
  hipLaunchKernelGGL(gru_seq_fwd_kernel, dim3(a.B / LR), dim3(1024), 0, s, a);
  return true;
}

bool launch_gru_seq_bwd(const GruSeqArgs& a, hipStream_t s) {
  if (!covered(a)) return false;
  hipLaunchKernelGGL(gru_seq_bwd_kernel, dim3(a.B / LR), dim3(1024), 0, s, a);
  return true;
}

bool launch_gru_proj_fwd(const GruSeqArgs& a, hipStream_t s) {
  if (!covered_stack(a) || !a.xpg || !a.xpc) return false;
  hipLaunchKernelGGL(gru_proj_fwd_kernel, dim3(a.B / LR), dim3(1024), 0, s, a);
  return true;
}

bool launch_gru_stack_bwd(const GruSeqArgs& a, hipStream_t s) {
  if (!covered_stack(a)) return false;
  hipLaunchKernelGGL(gru_stack_bwd_kernel, dim3(a.B / LR), dim3(1024), 0, s, a);
  return true;
}

}  // namespace dtfe
