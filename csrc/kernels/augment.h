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

// ---- label-side regularisation in the same launch: label smoothing, mixup, CutMix (B >= 2 to mix).
// With A_b the transformed fp32 pixel of slot b above, i = s * B + b (uint64, wrapping):
//   partner   shift = 1 + hash_u32(seed ^ MIX_ROT_SALT, s) % (B - 1),  p(b) = (b + shift) % B: a rotation
//             without a fixed point.  The partner image is what slot p gathers, under slot p's own crop /
//             flip draw: nothing new is drawn for it.
//   lambda    k = hash_u32(seed ^ MIX_LAM_SALT, i) >> 8,  lam = k * 2^-24 (hash_uniform; 1 - lam is exact)
//   mixup     out = fl(fl(lam * A_b) + fl((1 - lam) * A_p)): three roundings, no fused multiply-add
//   cutmix    r24 = floor(sqrt((2^24 - k) * 2^24)) as an exact integer, rw = (W * r24) >> 24, rh = (H * r24) >> 24,
//             hb = hash_u32(seed ^ MIX_BOX_SALT, i), cx = hb % W, cy = (hb / W) % H,
//             x0 = max(cx - rw / 2, 0), x1 = min(cx + rw / 2, W), y0, y1 alike with cy, rh, H (integer /);
//             out = A_p inside [y0, y1) x [x0, x1) of the OUTPUT, else A_b: no arithmetic on pixels;
//             lam' = fl(float(H * W - (x1 - x0) * (y1 - y0)) * inv_hw), inv_hw = fl(1 / fl(H * W)) from the host
//   labels    t_x[c] = smooth_on if c == label(x) else smooth_off (1 and 0 without smoothing; with
//             --label_smoothing E the host passes off = fl(E / ncls), on = fl(fl(1 - E) + off));
//             no mixing: onehot[b][c] = t_b[c];  mixing: fl(fl(w * t_b[c]) + fl((1 - w) * t_p[c])), w = lam or lam'
// labels_dst stays slot b's own label.  ops.mix_draws is the host mirror.
constexpr uint64_t MIX_LAM_SALT = 0x4D1C5EEDB1E2D0A7ull;
constexpr uint64_t MIX_BOX_SALT = 0xB0C5CE27E4A1F00Dull;
constexpr uint64_t MIX_ROT_SALT = 0x9A27E4F00D5EED13ull;
enum MixMode : int { MIX_NONE = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2 };

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
  int mix;  // MixMode; != MIX_NONE needs onehot and B >= 2
  float smooth_on = 1.f, smooth_off = 0.f;  // the two values of an unmixed label row (1, 0: hard labels)
  float inv_hw;  // cutmix: fl(1 / fl(H * W))
};
void launch_augment_rows(const AugmentArgs& a, hipStream_t s);

}  // namespace dtfe
