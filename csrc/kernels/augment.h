#pragma once
#include "elementwise.h"

namespace dtfe {

// ---- image input transforms fused into the batch gather: random crop of the zero-padded image,
// random horizontal flip, per-channel standardisation.  A superset of GatherArgs for image rows:
// src [n_rows][H][W][C] (dtype 0 = uint8 scaled by 1/255, 1 = f32) -> dst [B][H][W][C] (1 = f32,
// 2 = bf16); idx / on-device sampling, labels, one-hot rows, zero ranges and the (seed, counter, done)
// ticket mean what they mean there, and the row stream is the same: equal (seed, counter) pick equal rows.
//
// Per sample b at counter value s: h = hash_u32(seed ^ AUG_SALT, s * B + b), span = 2 * pad + 1,
//   dx = h % span, dy = (h / span) % span, flipped = flip && ((h / span^2) & 1)
//   out[b][y][x][c] = in(y + dy - pad, (flipped ? W - 1 - x : x) + dx - pad, c)
// i.e. a crop window of the padded image, then a mirror of the window.  in() outside the image is 0;
// inside it is (v - mean[c]) * inv_std[c] in fp32 (two roundings, no fused multiply-add), rounded to
// nearest even for a bf16 destination.  The border is 0 AFTER standardisation: it shows the mean
// colour, not black.  mean == nullptr: v unchanged.  ops.augment_draws is the host mirror.
constexpr uint64_t AUG_SALT = 0xC1FA5A17D00D5EEDull;
constexpr int AUG_MAX_PAD = 15;

struct AugmentArgs {
  const void* src; int src_dtype; long n_rows;
  void* dst; int dst_dtype; int B;
  int H, W, C, pad, flip;
  const float* mean; const float* inv_std;  // [C] each, or both null
  const int32_t* idx;
  const int32_t* labels_src; int32_t* labels_dst;
  uint64_t seed; int64_t* counter; uint32_t* done;
  uint32_t* zptr[4]; long zlen[4]; int nz;
  float* onehot; int ncls;
  int sample;  // SampleMode (elementwise.h) of the rows when idx is null; the crop / flip draws are the same in both
};
void launch_augment_rows(const AugmentArgs& a, hipStream_t s);

}  // namespace dtfe
