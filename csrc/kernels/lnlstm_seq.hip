// Persistent whole-sequence layer-normalised LSTM kernels (TF1 tf.contrib.rnn.LayerNormBasicLSTMCell, default
// arguments: forget_bias 1, no recurrent dropout).
//
//   z = [x_t | h] . K  (no bias)       y_k = gamma_k * LN(z_k) + beta_k,  k = i, j, f, o  (LN over the 128 units of a row)
//   c~ = c * sigmoid(y_f + 1) + sigmoid(y_i) * tanh(y_j)      c' = gamma_s * LN(c~) + beta_s      h' = tanh(c') * sigmoid(y_o)
//
// The normalised c' is the carried cell state.  Against lstm_seq.hip's step (GEMM -> activations -> cell update) this
// step has five row reductions, two of them on the dependent chain - the gates' after the GEMM and before any
// activation, the state's after the cell update and before tanh(c) - so it has a data flow of its own.  The ownership
// is the single-workgroup LSTM kernels' and gru_seq.hip's: ONE launch runs the whole recurrence, a workgroup of 1024
// threads (16 waves) owns 16 batch rows for all T steps and never waits on another workgroup (no flags, no spin loops,
// no co-residency requirement), and the weights the recurrence multiplies by are loaded ONCE into VGPRs as
// v_mfma_f32_16x16x4_f32 B fragments (exact fp32).
//
// Row statistics, always centred (two passes; never E[z^2] - mean^2).  The gates' (forward): the raw pre-activations
// sit in LDS, and wave w takes row w - each of its four (row, gate) pairs is two values per lane, a wave sum for the
// mean and a second one for the squares about it, no exchange.  Everything else uses the cell-update mapping
// p = tid + 1024 q: thread tid has unit tid % 128 of rows tid / 128 and tid / 128 + 8, so wave w holds the 64 consecutive
// units 64 (w % 2) .. of row w / 2 (+ 8), and a row statistic is a wave reduction (DPP, the total read back from
// lane 63 as a wave-uniform scalar) plus ONE exchange with the partner wave w ^ 1 through LDS.  For the state's variance each wave takes
// the mean of its 64 values and the sum of squares about it, and the halves are merged as mean = (m0 + m1) / 2,
// M2 = M2_0 + M2_1 + 32 (m1 - m0)^2 (the pairwise update of Chan et al.), both waves in the same order.  The gamma /
// beta vectors live in LDS (10 x 128).
//
// forward, per step t (4 barriers):
//   1  As = [x_t | h_{t-1}] (16 x 156, LDS) complete.  Wave w multiplies it by its 32 gate columns of K (78 VGPRs per
//      lane, all T steps) and leaves the RAW pre-activations in the Z tile (LDS).  x_{t+1} is fetched here.
//   2  wave w: mean and rstd of the four gates of row w -> LDS (and rs).
//   3  cell mapping: zhat -> HBM; affine, activations, c~ (c in registers); wave moments of c~ -> LDS.
//   4  merge: chat -> HBM, c' = gamma_s chat + beta_s, h' -> the h columns of As and of xh[t + 1] (or hT).
//   Saved for the backward: zhat [T][B][4H], chat [T][B][H], the five reciprocal deviations rs [T][B][5]; activations and
//   c' are rebuilt from them.
//
// backward, per step t = T-1..0 (4 barriers), dh (LDS partials) and dc (registers) carried on chip:
//   a  dh = P0 + P1; rebuild sigmoid(y_o), tanh(c'); dc' = dc + dh o (1 - tanh^2), dy_o; dchat = dc' gamma_s and its two
//      row sums (sum dchat, sum dchat chat) -> wave sums -> LDS.
//   1  dc~ = rs_s (dchat - mean(dchat) - chat mean(dchat chat)); rebuild i, j, f; dy_i, dy_j, dy_f; dc = dc~ f;
//      dzhat_k = dy_k gamma_k and the two row sums of each gate -> LDS.
//   2  dz_k = rs_k (dzhat_k - mean(dzhat_k) - zhat_k mean(dzhat_k zhat_k)) -> the DG tile (LDS) and dg (HBM).  Step
//      t - 1's saved values are fetched now, under the GEMM.
//   3  dh_{t-1} = dz . K_h^T: wave w takes unit tile w % 8 and k half w / 8 of the 512 (64 VGPRs of transposed recurrent
//      rows per lane, all T steps), partials into P[half].
//   4  next step.
//   The ten gamma / beta gradients: every thread sums its two (row, unit) pairs over all T steps in registers, the
//   workgroup adds its 16 rows through LDS in a fixed order and stores one [10][128] slab; lnlstm_ln_reduce_kernel
//   adds the slabs in workgroup order.  No atomics: the result is bitwise reproducible for a given B.
//
// The kernel gradient is one wgrad_tallk launch over (xh, dg), M = 156, N = 512, without a bias output.
//
// With csrc/build.py's flags (hipcc -O3 -std=c++17 --offload-arch=gfx950, no per-file flag), no scratch in any kernel:
//   lnlstm_seq_fwd_kernel  124 VGPRs, 48960 bytes LDS      lnlstm_seq_bwd_kernel  128 VGPRs, 56128 bytes LDS
// At 1024 threads a lane has 128 registers and the weights take 78 / 64 of them, so what keeps the rest within bounds is
// part of the design: wave sums on the DPP path (no index registers, results in SGPRs), per-thread indices rebuilt
// every step from an opaque tid (opaque_tid) so that no 64-bit address pair lives across the GEMM, workgroup-uniform
// bases for every HBM address, the reciprocal deviations of the backward through LDS, and scheduling barriers
// (LNLSTM_SERIAL) between the unrolled elementwise iterations and inside the GEMMs' operand loads.
#include "lnlstm_seq.h"

#include "common.h"

namespace dtfe {

namespace {

constexpr int LR = 16;        // batch rows per workgroup (one MFMA row tile)
constexpr int LH = 128;       // hidden units
constexpr int LI = 28;        // inputs per step
constexpr int KT = LI + LH;   // rows of K
constexpr int KT4 = KT / 4;   // gate k-steps
constexpr int G4 = 4 * LH;    // gate columns
constexpr int TPW = 2;        // 16-column MFMA tiles per wave (32 gate columns)
constexpr int NQ = LR * LH / 1024;  // (row, unit) pairs per thread
constexpr int AP = KT + 1;    // As pitch
constexpr int GP = G4 + 4;    // Z / DG tile pitch (16-byte rows)
constexpr int KH = G4 / 2;    // backward: k range per wave half
constexpr int NLN = LNLSTM_NLN, NRS = LNLSTM_NRS;
constexpr float LN_EPS = 1e-12f;

// Between the unrolled (pair, gate) iterations of the elementwise phases: the scheduler must not interleave them.
// Interleaved they need more registers than the weights leave (128 per lane at 1024 threads), and it is the weights
// that get spilled.
#define LNLSTM_SERIAL() __builtin_amdgcn_sched_barrier(0)

// tid, opaque to the optimiser: what is derived from it is computed where it is used, not hoisted out of the time loop
__device__ __forceinline__ int opaque_tid(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

__device__ __forceinline__ float dh_t_of(const LnLstmSeqArgs& a, int row, int u) {
  if (!a.dl) return a.dhT[(long)row * LH + u];
  float s = 0.f;
  for (int c = 0; c < a.nc; ++c) s = __builtin_fmaf(a.dl[(long)row * a.nc + c], a.wo[(long)u * a.nc + c], s);
  return s;
}

// Sum over the 64 lanes on the DPP path, the gfx9 wave reduction: quad swaps, the two row mirrors (every lane of a
// 16-lane row then holds its row's sum), row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3; lane 63 holds the
// total, read back as a wave-uniform scalar.  Against xor shuffles it needs no index registers and leaves the result in
// an SGPR.  Every lane must be active.
#define LNLSTM_DPP_ADD(v, ctrl, rows) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rows, 0xf, false))
__device__ __forceinline__ float wave_sum_dpp(float v) {
  LNLSTM_DPP_ADD(v, 0xB1, 0xf);   // quad_perm [1, 0, 3, 2]
  LNLSTM_DPP_ADD(v, 0x4E, 0xf);   // quad_perm [2, 3, 0, 1]
  LNLSTM_DPP_ADD(v, 0x141, 0xf);  // row_half_mirror
  LNLSTM_DPP_ADD(v, 0x140, 0xf);  // row_mirror
  LNLSTM_DPP_ADD(v, 0x142, 0xa);  // row_bcast15 -> rows 1, 3
  LNLSTM_DPP_ADD(v, 0x143, 0xc);  // row_bcast31 -> rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// mean of this wave's 64 values and their sum of squares about it
__device__ __forceinline__ void wave_moments(float v, float& m, float& m2) {
  m = wave_sum_dpp(v) * (1.f / 64.f);
  const float d = v - m;
  m2 = wave_sum_dpp(d * d);
}

// s = {m, M2} of half 0, {m, M2} of half 1 (64 values each) -> mean and reciprocal deviation of the 128
__device__ __forceinline__ void row_stats(const float* s, float& mean, float& rstd) {
  const float dm = s[2] - s[0];
  mean = 0.5f * (s[0] + s[2]);
  rstd = rsqrtf((s[1] + s[3] + 32.f * dm * dm) * (1.f / LH) + LN_EPS);
}

__global__ __launch_bounds__(1024) void lnlstm_seq_fwd_kernel(LnLstmSeqArgs a) {
  __shared__ float As[LR * AP];      // [x_t | h_{t-1}]
  __shared__ float Zs[LR * GP];      // raw gate pre-activations
  __shared__ float Ln[NLN * LH];     // gamma / beta
  __shared__ float Sg[LR * 4 * 2];   // [row][gate]{mean, rstd}
  __shared__ float Ss[LR * 4];       // [row][half]{m, M2} of c~
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, B = a.B;
  for (int e = tid; e < LR * KT; e += 1024) {
    const int r = e / KT, k = e - r * KT;
    As[r * AP + k] = a.xh[(long)(r0 + r) * KT + k];   // t = 0: x_0 and h_{-1}
  }
  for (int e = tid; e < NLN * LH; e += 1024) Ln[e] = a.ln[e];
  const int c0 = w * (16 * TPW), mrow = lane & 15, g = lane >> 4;
  // this wave's 32 gate columns of K as MFMA B fragments, loaded once and kept in VGPRs for all T steps
  float kreg[KT4][TPW];
  {
    const float* kcol = a.K + c0 + mrow;
#pragma unroll
    for (int kk = 0; kk < KT4; ++kk)
#pragma unroll
      for (int j = 0; j < TPW; ++j) kreg[kk][j] = kcol[(long)(4 * kk + g) * G4 + 16 * j];
  }
  float creg[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) creg[q] = 0.f;
  float xnext = 0.f;
  for (int t = 0; t < a.T; ++t) {
    const long row_t = (long)t * B + r0;
    // The per-thread indices outside the GEMM are rebuilt every step from an opaque copy of tid (opaque_tid): as loop
    // invariants the compiler keeps them, widened to 64-bit address pairs, in registers across the GEMM.
    // x_{t+1}: one element per thread (LR * LI = 448), fetched a step ahead
    const int tx = opaque_tid(tid);
    const bool xl = tx < LR * LI;
    const int xr = xl ? tx / LI : 0, xk = xl ? tx - xr * LI : 0;
    if (t > 0 && xl) As[xr * AP + xk] = xnext;
    __syncthreads();
    // (every HBM address of a step is a workgroup-uniform base plus a small 32-bit per-thread offset: no 64-bit
    // per-thread pointers live across the GEMM)
    if (t + 1 < a.T && xl) xnext = (a.xh + (row_t + B) * KT)[(unsigned)(xr * KT + xk)];
    // ---- 1: the gate GEMM, raw pre-activations into Zs
    {
      f32x4_t acc[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KT4; ++kk) {
        const float av = As[mrow * AP + 4 * kk + g];
#pragma unroll
        for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, kreg[kk][j], acc[j], 0, 0, 0);
        if (kk % 8 == 7) LNLSTM_SERIAL();  // at most 8 A values in flight beside the 78 of K
      }
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) Zs[(4 * g + e) * GP + c0 + 16 * j + mrow] = acc[j][e];
    }
    __syncthreads();
    // ---- 2: wave w takes row w: mean and reciprocal deviation of its four gates (two values per lane, no exchange)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* zr = Zs + w * GP + k * LH + lane;
      const float v0 = zr[0], v1 = zr[64];
      const float mean = wave_sum_dpp(v0 + v1) * (1.f / LH);
      const float d0 = v0 - mean, d1 = v1 - mean;
      const float rstd = rsqrtf(wave_sum_dpp(d0 * d0 + d1 * d1) * (1.f / LH) + LN_EPS);
      if (lane == 0) {
        Sg[(w * 4 + k) * 2] = mean;
        Sg[(w * 4 + k) * 2 + 1] = rstd;
        (a.rs + row_t * NRS)[(unsigned)(w * NRS + k)] = rstd;
      }
      LNLSTM_SERIAL();
    }
    __syncthreads();
    // ---- 3: normalise, affine, activations, c~ and its moments
    // cell mapping: unit cu of rows cr and cr + 8; this wave holds half ch of those rows
    const int tc = opaque_tid(tid), cr = tc >> 7, cu = tc & (LH - 1), ch = (tc >> 6) & 1;
    float ct[NQ], so[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int r = cr + 8 * q;
      float y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float zh = (Zs[r * GP + k * LH + cu] - Sg[(r * 4 + k) * 2]) * Sg[(r * 4 + k) * 2 + 1];
        (a.zhat + row_t * G4)[(unsigned)(r * G4 + k * LH + cu)] = zh;
        y[k] = Ln[2 * k * LH + cu] * zh + Ln[(2 * k + 1) * LH + cu];
        LNLSTM_SERIAL();
      }
      const float si = sigmoidf_(y[0]);
      LNLSTM_SERIAL();
      const float tj = tanhf(y[1]);
      LNLSTM_SERIAL();
      const float sf = sigmoidf_(y[2] + a.forget_bias);
      LNLSTM_SERIAL();
      so[q] = sigmoidf_(y[3]);
      ct[q] = creg[q] * sf + si * tj;
      float m, m2;
      wave_moments(ct[q], m, m2);
      if (lane == 0) {
        float* s = Ss + (r * 2 + ch) * 2;
        s[0] = m;
        s[1] = m2;
      }
      LNLSTM_SERIAL();
    }
    __syncthreads();
    // ---- 4: the normalised state and h
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int r = cr + 8 * q;
      float mean, rstd;
      row_stats(Ss + r * 4, mean, rstd);
      const float chv = (ct[q] - mean) * rstd;
      (a.chat + row_t * LH)[(unsigned)(r * LH + cu)] = chv;
      if (cu == 0) (a.rs + row_t * NRS)[(unsigned)(r * NRS + 4)] = rstd;
      const float c = Ln[8 * LH + cu] * chv + Ln[9 * LH + cu];
      creg[q] = c;
      const float h = tanhf(c) * so[q];
      As[r * AP + LI + cu] = h;
      if (t + 1 < a.T) (a.xh + (row_t + B) * KT)[(unsigned)(r * KT + LI + cu)] = h;
      else (a.hT + (long)r0 * LH)[(unsigned)(r * LH + cu)] = h;
      LNLSTM_SERIAL();
    }
    // (the next step's x write touches only the x columns of As, last read before barrier 2; its barrier orders the
    // h columns; Zs, Sg and Ss are rewritten only two or more barriers after their last read)
  }
}

__global__ __launch_bounds__(1024) void lnlstm_seq_bwd_kernel(LnLstmSeqArgs a) {
  __shared__ __attribute__((aligned(16))) float DG[LR * GP];  // dz of step t; after the last step the slab reduction
  __shared__ float P[2][LR * LH];    // dh partials of the two k halves
  __shared__ float Ln[NLN * LH];     // gamma / beta
  __shared__ float X1[LR * 2 * 2];   // [row][half]{sum dchat, sum dchat chat}
  __shared__ float X2[LR * 2 * 8];   // [row][half][gate]{sum dzhat, sum dzhat zhat}
  __shared__ float RS[LR * NRS];     // step t's reciprocal deviations
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r0 = blockIdx.x * LR, B = a.B;
  const int mrow = lane & 15, g = lane >> 4;
  const int tile = w & 7, half = w >> 3;
  for (int e = tid; e < NLN * LH; e += 1024) Ln[e] = a.ln[e];
  // this wave's K_h^T fragments (16 hidden units x its k half) in VGPRs for all T steps: lane group g supplies
  // k = 16 q + 4 g + e of MFMA step (q, e), so one 16-byte load / LDS read feeds 4 steps
  f32x4_t kb[KH / 16];
  {
    const float* krow = a.K + (long)(LI + tile * 16 + mrow) * G4 + half * KH + 4 * g;
#pragma unroll
    for (int q = 0; q < KH / 16; ++q) kb[q] = *reinterpret_cast<const f32x4_t*>(krow + 16 * q);
  }
  float dcn[NQ], acc[NLN];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int p = tid + 1024 * q;
    P[0][p] = dh_t_of(a, r0 + p / LH, p % LH);  // dh_T
    P[1][p] = 0.f;
    dcn[q] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < NLN; ++v) acc[v] = 0.f;
  // step t's saved values: zhat of the four gates, chat of steps t and t - 1; the 16 x 5 reciprocal deviations go
  // through one register of the first 80 threads into LDS
  float zh[NQ][4], chv[NQ], chp[NQ], rsn = 0.f;
  auto fetch = [&](int t) {
    const int tf = opaque_tid(tid), cr = tf >> 7, cu = tf & (LH - 1);  // (indices rebuilt per step, as in the forward)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const long row = (long)t * B + r0;  // (uniform bases, 32-bit per-thread offsets)
      const int r = cr + 8 * q;
#pragma unroll
      for (int k = 0; k < 4; ++k) zh[q][k] = (a.zhat + row * G4)[(unsigned)(r * G4 + k * LH + cu)];
      chv[q] = (a.chat + row * LH)[(unsigned)(r * LH + cu)];
      chp[q] = t > 0 ? (a.chat + (row - B) * LH)[(unsigned)(r * LH + cu)] : 0.f;
    }
    if (tf < LR * NRS) rsn = (a.rs + ((long)t * B + r0) * NRS)[(unsigned)tf];
  };
  fetch(a.T - 1);
  __syncthreads();
  for (int t = a.T - 1; t >= 0; --t) {
    const long row_t = (long)t * B + r0;
    const int ts = opaque_tid(tid), cr = ts >> 7, cu = ts & (LH - 1), ch = (ts >> 6) & 1;
    const float gs = Ln[8 * LH + cu], bs = Ln[9 * LH + cu];
    float dch[NQ];
    if (ts < LR * NRS) RS[ts] = rsn;
    // ---- a: through h' = tanh(c') o and c' = gamma_s chat + beta_s
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int r = cr + 8 * q, p = ts + 1024 * q;
      const float dh = P[0][p] + P[1][p];
      const float so = sigmoidf_(Ln[6 * LH + cu] * zh[q][3] + Ln[7 * LH + cu]);
      LNLSTM_SERIAL();
      const float tc = tanhf(gs * chv[q] + bs);
      LNLSTM_SERIAL();
      const float dc = dcn[q] + dh * so * (1.f - tc * tc);
      const float dyo = dh * tc * so * (1.f - so);
      acc[6] += dyo * zh[q][3];
      acc[7] += dyo;
      acc[8] += dc * chv[q];
      acc[9] += dc;
      DG[r * GP + 3 * LH + cu] = dyo * Ln[6 * LH + cu];  // dzhat_o, parked in this thread's own DG slot
      dch[q] = dc * gs;
      const float s1 = wave_sum_dpp(dch[q]), s2 = wave_sum_dpp(dch[q] * chv[q]);
      if (lane == 0) {
        float* s = X1 + (r * 2 + ch) * 2;
        s[0] = s1;
        s[1] = s2;
      }
      LNLSTM_SERIAL();
    }
    __syncthreads();
    // ---- 1: the state's LN backward, the cell backward, the gates' row sums
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int r = cr + 8 * q;
      const float* x = X1 + r * 4;
      const float m1 = (x[0] + x[2]) * (1.f / LH), m2 = (x[1] + x[3]) * (1.f / LH);
      const float dct = RS[r * NRS + 4] * (dch[q] - m1 - chv[q] * m2);
      const float si = sigmoidf_(Ln[0 * LH + cu] * zh[q][0] + Ln[1 * LH + cu]);
      LNLSTM_SERIAL();
      const float tj = tanhf(Ln[2 * LH + cu] * zh[q][1] + Ln[3 * LH + cu]);
      LNLSTM_SERIAL();
      const float sf = sigmoidf_(Ln[4 * LH + cu] * zh[q][2] + Ln[5 * LH + cu] + a.forget_bias);
      LNLSTM_SERIAL();
      const float cp = t > 0 ? gs * chp[q] + bs : 0.f;  // c'_{t-1}; c_{-1} = 0
      const float dy[3] = {dct * tj * si * (1.f - si), dct * si * (1.f - tj * tj), dct * cp * sf * (1.f - sf)};
      dcn[q] = dct * sf;
      float* dr = DG + r * GP + cu;  // dzhat_k: this thread's own slots, overwritten by dz_k in phase 2
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        acc[2 * k] += dy[k] * zh[q][k];
        acc[2 * k + 1] += dy[k];
        dr[k * LH] = dy[k] * Ln[2 * k * LH + cu];
      }
      float* s = X2 + (r * 2 + ch) * 8;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dzh = k < 3 ? dy[k] * Ln[2 * k * LH + cu] : dr[3 * LH];
        const float s1 = wave_sum_dpp(dzh), s2 = wave_sum_dpp(dzh * zh[q][k]);
        if (lane == 0) {
          s[2 * k] = s1;
          s[2 * k + 1] = s2;
        }
        LNLSTM_SERIAL();
      }
    }
    __syncthreads();
    // ---- 2: the gates' LN backward -> dz
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int r = cr + 8 * q;
      const float* x = X2 + r * 16;
      float* dr = DG + r * GP + cu;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float m1 = (x[2 * k] + x[8 + 2 * k]) * (1.f / LH), m2 = (x[2 * k + 1] + x[8 + 2 * k + 1]) * (1.f / LH);
        const float dz = RS[r * NRS + k] * (dr[k * LH] - m1 - zh[q][k] * m2);
        dr[k * LH] = dz;
        (a.dg + row_t * G4)[(unsigned)(r * G4 + k * LH + cu)] = dz;
        LNLSTM_SERIAL();
      }
    }
    if (t == 0) break;
    fetch(t - 1);  // lands under the GEMM
    __syncthreads();
    // ---- 3: dh_{t-1}[r][u] = sum_c DG[r][c] * K[I + u][c], this wave's unit tile and k half
    {
      const float* drow = DG + mrow * GP + half * KH + 4 * g;
      f32x4_t dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < KH / 16; ++q) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(drow + 16 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) dacc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], kb[q][e], dacc, 0, 0, 0);
        if (q % 2 == 1) LNLSTM_SERIAL();  // at most 2 A vectors (8 registers) in flight beside the 64 of K_h^T
      }
      float* pp = P[half] + tile * 16 + mrow;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[(4 * g + e) * LH] = dacc[e];
    }
    __syncthreads();
  }
  // the workgroup's slab of gamma / beta gradients: thread group cr = tid / 128 holds rows cr and cr + 8 of unit cu;
  // the 8 groups are added in order, five vectors at a time through the DG tile (8 x 5 x 128 floats)
  const int cr = tid >> 7, cu = tid & (LH - 1);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NLN / 2; ++v) DG[(cr * (NLN / 2) + v) * LH + cu] = acc[pass * (NLN / 2) + v];
    __syncthreads();
    if (tid < NLN / 2 * LH) {
      float s = DG[tid];
#pragma unroll
      for (int gq = 1; gq < 8; ++gq) s += DG[gq * (NLN / 2) * LH + tid];
      a.ws[((long)blockIdx.x * NLN + pass * (NLN / 2)) * LH + tid] = s;
    }
  }
}

// dln[e] = the slabs' element e added in workgroup order
__global__ __launch_bounds__(256) void lnlstm_ln_reduce_kernel(const float* ws, float* dln, int groups) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= NLN * LH) return;
  float s = ws[e];
  for (int gq = 1; gq < groups; ++gq) s += ws[(long)gq * NLN * LH + e];
  dln[e] = s;
}

bool covered(const LnLstmSeqArgs& a) { return a.H == LH && a.I == LI && a.T >= 1 && a.B >= LR && a.B % LR == 0; }

}  // namespace

bool launch_lnlstm_seq_fwd(const LnLstmSeqArgs& a, hipStream_t s) {
  if (!covered(a)) return false;
  hipLaunchKernelGGL(lnlstm_seq_fwd_kernel, dim3(a.B / LR), dim3(1024), 0, s, a);
  return true;
}

bool launch_lnlstm_seq_bwd(const LnLstmSeqArgs& a, hipStream_t s) {
  if (!covered(a)) return false;
  hipLaunchKernelGGL(lnlstm_seq_bwd_kernel, dim3(a.B / LR), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(lnlstm_ln_reduce_kernel, dim3((NLN * LH + 255) / 256), dim3(256), 0, s, a.ws, a.dln, a.B / LR);
  return true;
}

}  // namespace dtfe
