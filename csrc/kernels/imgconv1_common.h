#pragma once
// MNIST conv1's padded plane P and its column-shifted copies (see imgconv1_copies.hip): the layout
// constants and the staging helpers shared by the conv1 kernels and the fused conv1 + conv2 forward
// (imgconv12_fused.hip, whose producer waves build the same P and copies row by row).
#include "common.h"

#include <type_traits>

namespace dtfe {
namespace c1 {

constexpr int TH = 256;                  // 4 waves
constexpr int HI = 28;                   // image / output size
constexpr int PWD = 48, PRW = 32;        // P: 32 rows x 48 columns (rows 16-B aligned)
constexpr int CWD = 40;                  // copy row pitch (elements): 5 x 16-B slots
constexpr int CSZ = PRW * CWD + 8;       // copy stride (+1 slot skew per copy)
constexpr int NCH = 32;                  // output channels
constexpr int XCH = HI * HI / 4;         // 8-byte chunks of an image (196)

__device__ __forceinline__ u32x4_t ld16l(const bf16* p) { return *reinterpret_cast<const u32x4_t*>(p); }

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [B, E)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for_c1(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for_c1<B + 1, E>(f);
  }
}

// image b -> P interior (8-byte chunks: 4 pixels of one row; rows are 56 B)
__device__ __forceinline__ void load_img(const bf16* x, long b, u32x2_t& v) {
  if (threadIdx.x < XCH) v = *reinterpret_cast<const u32x2_t*>(x + b * (HI * HI) + threadIdx.x * 4);
}
__device__ __forceinline__ void write_img(bf16* P, const u32x2_t& v) {
  if (threadIdx.x < XCH) {
    const int r = threadIdx.x / 7, c = (threadIdx.x - r * 7) * 4;
    *reinterpret_cast<u32x2_t*>(P + (r + 2) * PWD + c + 4) = v;
  }
}

// four pixels of a sampled uint8 row -> bf16 in [0, 1] (the weight gradient's x and P hold these bits)
__device__ __forceinline__ u32x2_t px4_to_bf16(uint32_t px) {
  const float k = 1.f / 255.f;
  return u32x2_t{pack_bf16x2((float)(px & 0xffu) * k, (float)((px >> 8) & 0xffu) * k),
                 pack_bf16x2((float)((px >> 16) & 0xffu) * k, (float)(px >> 24) * k)};
}

// copies s < S (rows 0..31, 32 columns each = 4 chunks of 8).  Thread (r, c8, half) reads the three
// aligned 16-B chunks P[r][c8 .. c8+23] once and forms its copies' 8-element windows (first element
// s + 2) with dword funnel shifts (v_alignbyte) - an earlier form gathered every element with its own
// ds_read_u16 (8 LDS reads + 8 VALU per chunk, bank conflicts: rocprof PMC r6pmc2)
__device__ __forceinline__ uint32_t shr16(uint32_t lo, uint32_t hi) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> 16);
}
template <int S>
__device__ __forceinline__ void build_copies(const bf16* P, bf16* C) {
  constexpr int HALF = (S + 1) / 2;  // copies per thread: threads 0..127 take s < HALF, 128..255 the rest
  const int t = threadIdx.x & 127, r = t >> 2, c8 = (t & 3) * 8;
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(P + r * PWD + c8);
  uint32_t d[12];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const u32x4_t v = src[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) d[4 * j + e] = v[e];
  }
  auto emit = [&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int e0 = s + 2;
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (e0 & 1) ? shr16(d[(e0 >> 1) + j], d[(e0 >> 1) + j + 1]) : d[(e0 >> 1) + j];
    *reinterpret_cast<u32x4_t*>(C + s * CSZ + r * CWD + c8) = o;
  };
  if (threadIdx.x < 128) {
    static_for_c1<0, HALF>(emit);
  } else {
    static_for_c1<HALF, S>(emit);
  }
}

// conv1's weights as this lane's MFMA B fragments (k = kh*8 + kw, kw >= 5 zero): step 0 rows
// kh = g (kw 0..7), step 1 row kh = 4 (g == 0 only); and the lane's two bias values
// (g = lane >> 4).  A copy of conv1c_fwd_kernel's prologue block, which stays inline there: routed
// through this function that kernel's generated code changed (the rest of this header leaves it
// instruction for instruction as it was)
__device__ __forceinline__ void load_conv1_weights(const bf16* w, const float* bias, int lane, int g,
                                                   bf16x8_t (&bw)[2][2], float (&biasv)[2]) {
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = nt * 16 + (lane & 15);
    biasv[nt] = bias ? bias[n] : 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int kh = st == 0 ? g : 4;
      const bool rowok = st == 0 || g == 0;
      s16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (short)((rowok && j < 5) ? w[n * 25 + kh * 5 + j] : 0);
      bw[nt][st] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
}

}  // namespace c1
}  // namespace dtfe
