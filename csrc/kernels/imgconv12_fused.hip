// MNIST conv1 + conv2 forward in ONE persistent launch (B >= 256, bf16):
//
//   uint8 row (sampled) -> x, label -> conv1 5x5x1->32 +bias, ReLU, 2x2 max-pool (p1, a1)
//                                   -> conv2 5x5x32->64 +bias, ReLU, 2x2 max-pool (p2, a2)
//
// The pair of launches this replaces (conv1c_fwd_kernel, imgconv1_copies.hip; the conv2 forward
// instance of imgconv_fixed_kernel, imgconv_persist.hip) were both bound by fixed cost, not by MFMA
// work: conv1's prologue, its scattered 2-byte / 1-byte p1 / a1 stores and its drain, then conv2's
// prologue (zeroing, 104 KB of weights per workgroup), its global re-read of the p1 written one
// launch earlier, and the launch boundary between them.  Here one workgroup per CU keeps conv2's
// weights in LDS and, per image, runs conv1 straight into conv2's zero-padded LDS image.
//
// Waves: 13 conv2 waves (one 16-row tile each) and 3 producer waves, 4 per SIMD.  While the 13 run
// conv2's k loop of image i, the producers store p1 / a1 of image i and build conv1's input of image
// i + 1.  A producer owns whole rows of P and of the shifted copies: it writes its rows of P and
// reads them back itself (LDS operations of one wave execute in order), so the staging needs no
// barrier of its own.  All 16 waves run conv1's tiles and the p2 / a2 stores.
//
//   once:      zero the image, clear the step's accumulators; then
//                conv2 waves: stage conv2's weights
//                producers:   zero P; first image's row -> P, x, label; its copies; the second
//                             row's load is issued                                     barrier
//   per image: conv1's 49 tiles over 16 waves; epilogue -> conv2's LDS image (values in the
//              pixel's 32 channels, argmax bytes in the pixel's 32 pad bytes)          barrier 1
//                conv2 waves: the k loop; pooled epilogue staged in LDS padding
//                producers:   p1 / a1 leave as 16-B chunks of the LDS image; next image's row -> P,
//                             x and label to global; its 8 shifted copies; the load of the row
//                             after it is issued                                       barrier 2
//              p2 / a2 leave as 16-B chunks
//
// The MFMA sequences and accumulation orders are those of the two kernels (conv1: 2 steps per
// tile; conv2: 25 steps x 4 n-tiles per 16-row tile), so every output is bit-identical to the
// pair's.  The conv1 tile body (a wave's 3 or 4 tiles go as one batch) and the conv2 k loop /
// epilogue are copies of those kernels' bodies with the geometry folded to constants (sharing the
// bodies as functions would re-schedule the tuned originals); the P / shifted-copy layout is that
// of imgconv1_common.h.
//
// LDS (bytes): conv2 weights 64 x 816 x 2 = 104,448; conv2 image 18 x 20 x 48 x 2 = 34,560;
// shifted copies 20,608 (live from their build under image i's k loop to conv1 of image i + 1:
// nothing aliases them); P 3,072 (its zero border persists across images).  162,688 of 163,840.
// The p2 / a2 staging (9,408 = 588 chunks of 16 B) has no region of its own: it lies in padding of
// the other three that nothing reads and that only the prologue writes (stage_off below), so the
// epilogue needs no barrier in front of it and nothing has to be zeroed again.
#include "imgconv.h"
#include "imgconv1_common.h"

namespace dtfe {

namespace {

using namespace c1;

constexpr int CW = 13, SW = 3;         // conv2 waves, producer waves
constexpr int WAVES = CW + SW, THREADS = 64 * WAVES;
// conv2 (the geometry of imgconv_fixed_kernel<32, 5, 5, 20, 48, 816, 4, 1, 13, 1, false, ACT_RELU>)
constexpr int CS = 32, KH = 5, KW = 5, LWP = 20, PS = 48, N2 = 64, NT = N2 / 16;
constexpr int K2 = KH * KW * CS, NK = K2 / 32, KP = K2 + 16;
constexpr int PH = HI / 2;             // conv1's pooled output = conv2's source and output extent (14)
constexpr int LH = PH + KH - 1;        // padded LDS image rows (18)
constexpr int QH = PH / 2, Q2 = QH * QH;  // conv2's pooled output (7 x 7)
constexpr int P1N = PH * PH * NCH;     // elements of one image's p1 / a1
constexpr int P2N = Q2 * N2;           // elements of one image's p2 / a2
constexpr int W_EL = N2 * KP, IMG_EL = LH * LWP * PS;
constexpr int STAGE_B = P2N * 3, COPIES_B = 8 * CSZ * 2;
constexpr int P_B = PRW * PWD * 2;
constexpr int LDS_B = W_EL * 2 + IMG_EL * 2 + COPIES_B + P_B;
static_assert(W_EL * 2 == 104448 && IMG_EL * 2 == 34560 && STAGE_B == 9408 && COPIES_B == 20608 && P_B == 3072,
              "LDS regions");
static_assert(LDS_B == 162688 && LDS_B <= 160 * 1024, "LDS budget");
static_assert(K2 % 32 == 0 && PS >= CS + NCH / 2, "a pixel's pad bytes hold its 32 argmax bytes");
static_assert((PH * PH + 15) / 16 == CW, "one conv2 row tile per wave");
static_assert(3 * WAVES < 49 && 49 <= 3 * WAVES + 1, "conv1: 3 tiles per wave and tile 48 for wave 0");

// p2 / a2 staging: 16-B chunk c (p2: P2N / 8 chunks, then a2: P2N / 16) -> byte offset in LDS.  The staging
// lies in padding that nothing else reads or, after the prologue, writes:
//   chunks   0..255  the 16-B pad behind each of the 8 x 32 copy rows (conv1 reads 32 of a row's 40 elements)
//          256..383  the 32-B pad behind each of the 64 weight rows (elements K2 .. KP - 1)
//          384..587  columns 18, 19 of the image's rows 0 .. 16 (conv2 reads columns 0 .. 17): 12 chunks a row
constexpr int PIXB = PS * 2;                                       // bytes of an LDS pixel
constexpr int ST_C = 8 * PRW, ST_W = 2 * N2, ST_I = STAGE_B / 16 - ST_C - ST_W;
constexpr int ST_IROW = (LWP - (PH + KW - 1)) * PIXB / 16;         // chunks of a row's unread columns
static_assert(CWD - 32 == 8 && CSZ == PRW * CWD + 8 && KP - K2 == 16 && PIXB % 16 == 0, "pad chunks");
static_assert(ST_I > 0 && ST_I <= LH * ST_IROW, "the padding holds the staging");
__device__ __forceinline__ int stage_off(int c) {
  if (c < ST_C) return W_EL * 2 + IMG_EL * 2 + c * (CWD * 2) + (c / PRW) * 16 + 64;
  if (c < ST_C + ST_W) return ((c - ST_C) >> 1) * (KP * 2) + K2 * 2 + ((c - ST_C) & 1) * 16;
  const int i = c - ST_C - ST_W, row = i / ST_IROW;
  return W_EL * 2 + (row * LWP + PH + KW - 1) * PIXB + (i - row * ST_IROW) * 16;
}

struct Conv12Args {
  ImgConvArgs c1;     // conv1 with the fused sampling (y = p1, argmax = a1)
  const bf16* w2;     // [64][25][32]
  const float* b2;
  bf16* p2;           // [B][7][7][64]
  uint8_t* a2;
};

// compile-time loop (as in imgconv_persist.hip)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// conv2 output row m in 2x2-window (pool) order -> window index; -1 for the last tile's padding rows.
// Row quad `quad` of 16-row tile t is window t*4 + {0,2,3,1}[quad] (imgconv_persist.hip: row_pixel).
__device__ __forceinline__ int row_window(int m) {
  const int t = m >> 4, quad = (m >> 2) & 3;
  const int w = t * 4 + (quad == 0 ? 0 : quad == 1 ? 2 : quad == 2 ? 3 : 1);
  return w < Q2 ? w : -1;
}

// the value, hidden from the optimizer: addresses derived from it are formed where they are used,
// not hoisted out of the image loop into registers that would stay live through conv2's k loop
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

__global__ __launch_bounds__(THREADS) void conv12_fwd_kernel(Conv12Args A) {
  constexpr int NP = (((PRW + SW - 1) / SW) * 7 + 63) / 64;  // passes over a producer wave's 8-byte image chunks
  static_assert(((PRW + SW - 1) / SW) * 4 <= 64, "a lane per (row, 16-B column chunk) of the wave's copy rows");
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  bf16* wl = lds;
  bf16* img = wl + W_EL;
  bf16* C = img + IMG_EL;                                    // conv1's shifted copies
  bf16* P = C + COPIES_B / 2;
  uint8_t* stg = reinterpret_cast<uint8_t*>(lds);            // conv2's staged p2 / a2: stage_off()
  const ImgConvArgs& a = A.c1;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4;

  for (int i = tid; i < IMG_EL / 8; i += THREADS) reinterpret_cast<u32x4_t*>(img)[i] = u32x4_t{0u, 0u, 0u, 0u};

  // the step's accumulators and the sampling counter, exactly as conv1c_fwd_kernel
  const int64_t gstep = *a.g_counter;
  for (int z = 0; z < a.nz; ++z)
    for (long i = (long)blockIdx.x * THREADS + tid; i < a.zlen[z]; i += (long)gridDim.x * THREADS) a.zptr[z][i] = 0u;

  // producer wave sw owns rows [r0, r1) of P and of the copies, that is the image's 8-byte chunks
  // (4 pixels of one row, 7 per row) [c0, c0 + nc)
  const int sw = wid - CW;
  const bool producer = sw >= 0;
  const int r0 = sw * PRW / SW, r1 = (sw + 1) * PRW / SW;
  const int c0 = 7 * (r0 > 2 ? r0 - 2 : 0), nc = 7 * (r1 - 2 < HI ? r1 - 2 : HI) - c0;
  // sampled row of image bb: only the loads are issued here (the label by the first producer wave's
  // lane 0); the conversion and the x / label stores wait until the row is staged
  uint32_t px[NP];
  int32_t lab = 0;
#pragma unroll
  for (int u = 0; u < NP; ++u) px[u] = 0u;
  auto fetch = [&](long bb) {
    const long r = (long)(hash_u32(a.g_seed, (uint64_t)gstep * a.B + bb) % (uint32_t)a.g_rows);
    const int ln = opaque(lane);
#pragma unroll
    for (int u = 0; u < NP; ++u)
      if (ln + 64 * u < nc) px[u] = *reinterpret_cast<const uint32_t*>(a.g_src + r * (HI * HI) + (c0 + ln + 64 * u) * 4);
    if (sw == 0 && lane == 0) lab = a.g_labels_src[r];
  };
  // the fetched row of image bb: bf16 into the wave's rows of P, x and the label to global (conv1's
  // weight gradient reads x); then the wave's rows of the 8 shifted copies (build_copies' windows)
  auto stage = [&](long bb) {
    const int ln = opaque(lane);
#pragma unroll
    for (int u = 0; u < NP; ++u)
      if (ln + 64 * u < nc) {
        const int id = c0 + ln + 64 * u, r = id / 7, c = (id - r * 7) * 4;
        const u32x2_t v = px4_to_bf16(px[u]);
        *reinterpret_cast<u32x2_t*>(const_cast<bf16*>(a.src) + bb * (HI * HI) + id * 4) = v;
        *reinterpret_cast<u32x2_t*>(P + (r + 2) * PWD + c + 4) = v;
      }
    if (sw == 0 && lane == 0 && a.g_labels_dst) a.g_labels_dst[bb] = lab;
    // the reads below are of rows this wave wrote: in order behind the writes, no barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int r = r0 + (ln >> 2), c8 = (ln & 3) * 8;
    if (r < r1) {
      const u32x4_t* src = reinterpret_cast<const u32x4_t*>(P + r * PWD + c8);
      uint32_t d[12];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const u32x4_t v = src[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[4 * j + e] = v[e];
      }
      static_for<0, 8>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int e0 = s + 2;
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (e0 & 1) ? shr16(d[(e0 >> 1) + j], d[(e0 >> 1) + j + 1]) : d[(e0 >> 1) + j];
        *reinterpret_cast<u32x4_t*>(C + s * CSZ + r * CWD + c8) = o;
      });
    }
  };
  long b = blockIdx.x;
  if (producer) {
    // the producers stage the first image beside the weight staging: each zeroes its own rows of P
    // (the border stays zero from here on) and is the only wave that touches them
    if (b < a.B) fetch(b);
    for (int k = lane; k < (r1 - r0) * (PWD / 8); k += 64)
      reinterpret_cast<u32x4_t*>(P + r0 * PWD)[k] = u32x4_t{0u, 0u, 0u, 0u};
    if (b < a.B) {
      stage(b);
      if (b + gridDim.x < a.B) fetch(b + gridDim.x);
    }
  } else {  // conv2's weights -> LDS rows of KP elements (zero past K2), 8 loads in flight per thread
    constexpr int kc_row = KP / 8, total = N2 * kc_row;
    static_assert(total <= 8 * 64 * CW, "one pass");
    u32x4_t v[8];
    int off[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = tid + u * 64 * CW;
      const int n = i / kc_row, k = (i - n * kc_row) * 8;
      off[u] = i < total ? n * KP + k : -1;
      v[u] = u32x4_t{0u, 0u, 0u, 0u};
      if (i < total && k < K2) v[u] = *reinterpret_cast<const u32x4_t*>(A.w2 + (long)n * K2 + k);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (off[u] >= 0) *reinterpret_cast<u32x4_t*>(wl + off[u]) = v[u];
  }

  // conv1: weights as B fragments, bias
  bf16x8_t bw[2][2];
  float bias1[2];
  load_conv1_weights(a.w, a.bias, lane, g, bw, bias1);

  // conv2: per-lane constants (the same for every image)
  const bf16* wlane = wl + (lane & 15) * KP + 8 * g;
  float bias2[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) bias2[n] = A.b2 ? A.b2[n * 16 + (lane & 15)] : 0.f;
  // A-fragment base: the lane's output pixel (row wid*16 + lane%16 of the image in pool order);
  // padding rows of the last tile multiply pixel 0 and are dropped by the epilogue
  const bf16* abase;
  {
    const int m = wid * 16 + (lane & 15), w = row_window(m), q = m & 3;
    const int oy = 2 * (w / QH) + (q >> 1), ox = 2 * (w % QH) + (q & 1);
    abase = img + (w >= 0 ? (oy * LWP + ox) * PS : 0) + 8 * g;
  }
  const int ppix = row_window(wid * 16 + g * 4);  // the pooled pixel of this lane's accumulator quad (-1: none)

  __syncthreads();  // zero borders, weights and the first image's copies
  for (; b < a.B; b += gridDim.x) {
    const bool more = b + gridDim.x < a.B;
    // staging of the next image; the row after it is fetched behind it
    auto stage_next = [&]() {
      if (more) {
        stage(b + gridDim.x);
        if (b + 2 * (long)gridDim.x < a.B) fetch(b + 2 * (long)gridDim.x);
      }
    };
    // p1 (784 chunks: pixel i / 4, channels 8 (i % 4) ..) and a1 (392 chunks: pixel k / 2, bytes
    // 16 (k % 2) ..) leave as the 16-B chunks of the LDS image's interior: the
    // producer waves' work, beside the k loop
    auto store_p1a1 = [&]() {
      const long ob = b * (long)P1N;
      for (int i = opaque(tid) - 64 * CW; i < P1N / 8 + P1N / 16; i += 64 * SW) {
        const bool isv = i < P1N / 8;
        const int k = isv ? i : i - P1N / 8;
        const int pix = isv ? k >> 2 : k >> 1, py = pix / PH, pxx = pix - py * PH;
        const bf16* pp = img + ((py + 2) * LWP + pxx + 2) * PS;
        if (isv) {
          *reinterpret_cast<u32x4_t*>(a.y + ob + k * 8) = *reinterpret_cast<const u32x4_t*>(pp + (k & 3) * 8);
        } else {
          *reinterpret_cast<u32x4_t*>(a.argmax + ob + k * 16) =
              *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const uint8_t*>(pp + CS) + (k & 1) * 16);
        }
      }
    };

    // ---- 1. conv1: 49 tiles of 16 output pixels in 2x2-window order (conv1c_fwd_kernel's tile body);
    // the pooled value goes to conv2's LDS image at interior pixel (py + 2, px + 2), its argmax
    // byte into that pixel's pad bytes
    // The wave's tiles (wid, wid + 16, ..: 3, and a 4th for wave 0) go as one batch - all fragment
    // reads, then the MFMAs, then the epilogues - so that their LDS and MFMA latencies overlap;
    // each tile's two accumulation steps are as before.  Waves without a 4th tile compute tile 48
    // again and drop it.
    {
      constexpr int TPW = (49 + WAVES - 1) / WAVES;
      bf16x8_t fa0[TPW], fa1[TPW];
      f32x4_t acc[TPW][2];
      static_for<0, TPW>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const int t = j < TPW - 1 ? wid + j * WAVES : 48;
        const int m = t * 16 + (lane & 15), q = m & 3, w = m >> 2;
        const int oy = 2 * (w / 14) + (q >> 1), ox = 2 * (w % 14) + (q & 1);
        const int s = ox & 7;
        const bf16* ab = C + s * CSZ + (ox - s) + oy * CWD;
        fa0[j] = __builtin_bit_cast(bf16x8_t, ld16l(ab + g * CWD));
        fa1[j] = __builtin_bit_cast(bf16x8_t, ld16l(ab + 4 * CWD));
      });
      static_for<0, TPW>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0[j], bw[nt][0], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1[j], bw[nt][1], acc[j][nt], 0, 0, 0);
        }
      });
      static_for<0, TPW>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < TPW - 1 || wid == 0) {
          // lane holds rows (lane>>4)*4 + j = one 2x2 window, column lane & 15 of each n-tile
          const int t = j < TPW - 1 ? wid + j * WAVES : 48;
          const int wq = t * 4 + g, py = wq / 14, pxx = wq - py * 14;
          bf16* pp = img + ((py + 2) * LWP + pxx + 2) * PS;
          uint8_t* pa = reinterpret_cast<uint8_t*>(pp + CS);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const f32x4_t v = acc[j][nt];
            int am = 0;
            float mx = v[0];
#pragma unroll
            for (int e = 1; e < 4; ++e) if (v[e] > mx) { mx = v[e]; am = e; }
            const int ch = nt * 16 + (lane & 15);
            pp[ch] = f2bf(apply_act(mx + bias1[nt], ACT_RELU));
            pa[ch] = (uint8_t)am;
          }
        }
      });
    }
    __syncthreads();  // 1 (also: the copies are dead, and the previous p2 / a2 staging has been read)

    // ---- 2. conv2 (imgconv_fixed_kernel's forward body, RT = 1): the k loop is fully unrolled, fragments
    // are fetched PF steps ahead in a ring of PF + 1 register sets, reads pinned between the MFMAs
    f32x4_t acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (wid < CW) {
      constexpr int PF = 2;
      u32x4_t fa[PF + 1], fb[PF + 1][NT];
      auto fetch_frag = [&](auto sc) {
        constexpr int st = decltype(sc)::value;
        constexpr int k0 = 32 * st, tap = k0 / CS, cs = k0 - tap * CS;
        constexpr int toff = ((tap / KW) * LWP + (tap % KW)) * PS + cs;
        constexpr int buf = st % (PF + 1);
        fa[buf] = *reinterpret_cast<const u32x4_t*>(abase + toff);
#pragma unroll
        for (int n = 0; n < NT; ++n) fb[buf][n] = *reinterpret_cast<const u32x4_t*>(wlane + n * 16 * KP + k0);
      };
      static_for<0, PF>([&](auto sc) { fetch_frag(sc); });
      static_for<0, NK>([&](auto sc) {
        constexpr int st = decltype(sc)::value;
        if constexpr (st + PF < NK) fetch_frag(std::integral_constant<int, st + PF>{});
        constexpr int buf = st % (PF + 1);
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[buf]),
                                                           __builtin_bit_cast(bf16x8_t, fb[buf][n]), acc[n], 0, 0, 0);
        constexpr int nm = NT, nr = (st + PF < NK) ? 1 + NT : 0;
        static_for<0, nm>([&](auto ic) {
          constexpr int i = decltype(ic)::value, r0 = i * nr / nm, r1 = (i + 1) * nr / nm;
          if constexpr (r1 > r0) __builtin_amdgcn_sched_group_barrier(0x100, r1 - r0, 0);
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        });
      });
    } else {  // producer waves
      store_p1a1();
      stage_next();
    }
    // pooled epilogue (+bias, ReLU, 2x2 max, argmax) staged in the output's own layout
    if (ppix >= 0) {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = n * 16 + (lane & 15), e = ppix * N2 + col;
        const f32x4_t v = acc[n];
        int am = 0;
        float mx = v[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) if (v[j] > mx) { mx = v[j]; am = j; }
        *reinterpret_cast<bf16*>(stg + stage_off(e >> 3) + (e & 7) * 2) = f2bf(apply_act(mx + bias2[n], ACT_RELU));
        stg[stage_off(P2N / 8 + (e >> 4)) + (e & 15)] = (uint8_t)am;
      }
    }
    __syncthreads();  // 2 (also: every wave is done with the LDS image before the next conv1 rewrites it)
    {
      constexpr int ny = P2N / 8, na = P2N / 16;
      const long pb = b * (long)P2N;
      for (int i = tid; i < ny + na; i += THREADS) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(stg + stage_off(i));
        if (i < ny) {
          *reinterpret_cast<u32x4_t*>(A.p2 + pb + i * 8) = v;
        } else {
          *reinterpret_cast<u32x4_t*>(A.a2 + pb + (i - ny) * 16) = v;
        }
      }
    }
  }
  if (a.g_done && tid == 0) {  // the last workgroup advances the sampling step (as conv1c_fwd_kernel)
    const uint32_t prev = __hip_atomic_fetch_add(a.g_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_fetch_add((unsigned long long*)a.g_counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.g_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

bool launch_conv12_fused_fwd(const ImgConvArgs& a, const bf16* w2, const float* b2, bf16* p2, uint8_t* a2,
                             hipStream_t s) {
  if (a.B < 256 || a.SH != HI || a.SW != HI || a.CS != 1 || a.OH != HI || a.OW != HI || a.N != NCH || a.KH != 5 ||
      a.KW != 5 || a.stride != 1 || a.pad != 2)
    return false;
  if (!a.src || !a.pool || a.flip_taps || a.dil > 1 || a.relu_mask || a.act != ACT_RELU) return false;
  if (!a.g_src || !a.g_counter || !a.g_labels_src || !a.y || !a.argmax || !w2 || !p2 || !a2) return false;
  Conv12Args A{a, w2, b2, p2, a2};
  A.c1.diag = 0;
  const int grid = a.B < 256 ? a.B : 256;  // one workgroup per CU, persistent over the batch
  (void)hipFuncSetAttribute((const void*)conv12_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_B);
  hipLaunchKernelGGL(conv12_fwd_kernel, dim3(grid), dim3(THREADS), LDS_B, s, A);
  return true;
}

}  // namespace dtfe
