#pragma once
#include "common.h"

namespace dtfe {

// One chunk of a gradient-norm plan: elements [off, off + count) of the flat gradient buffer,
// count <= GRAD_CHUNK_MAX.  The plan (a device array of these) covers exactly the elements of an
// optimizer's var list - never the padding between variables, never a variable outside the list.
struct GradChunk {
  long off;
  long count;
};
constexpr int GRAD_CHUNK_MAX = 8192;
constexpr int GRAD_NORM_MAX_BLOCKS = 2048;

// tf.clip_by_global_norm's two scalars of one var list:
//   out[0] = norm  = sqrt(sum over the plan of (gscale * g[i])^2)
//   out[1] = scale = clip_norm / max(norm, clip_norm)   (1 when norm <= clip_norm)
struct GradNormArgs {
  const float* g; const bf16* g16; float gscale;   // exactly one of g / g16
  float clip_norm;
  const GradChunk* plan; int nchunk;
  float* partials;     // [nchunk]: chunk c's sum of squares lands in partials[c], whatever the grid
  uint32_t* ticket;    // zero-initialised; reset by the last workgroup
  float* out;          // [2]
  int max_blocks;      // 0: up to GRAD_NORM_MAX_BLOCKS workgroups (a test forces 1)
};
void launch_grad_sumsq(const GradNormArgs& a, hipStream_t s);

// t[i] *= *scale over the plan's chunks (a ps worker scales its gradient before the push)
void launch_scale_ranges(float* t, const float* scale, const GradChunk* plan, int nchunk, hipStream_t s);

}  // namespace dtfe
