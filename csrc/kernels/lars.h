#pragma once
#include "common.h"

namespace dtfe {

// Layer-wise adaptive rate scaling (tf.contrib.opt.LARSOptimizer): one norm of the fp32 master and one of the
// gradient per adaptive variable of an optimizer, and from the two the variable's trust ratio - the factor
// the fused apply multiplies into its learning rate (OptArgs::seg_lr).

// One chunk of the plan: elements [off, off + count) of the flat buffers, all of segment seg (an index into
// the optimizer's var list), count <= LARS_CHUNK_MAX.  A segment's chunks are consecutive in the plan, in
// element order.  The plan covers exactly the adaptive variables' elements - never the padding between
// variables, never a variable outside the var list, never a variable of the skip list.
struct LarsChunk {
  long seg;
  long off;
  long count;
};
constexpr int LARS_CHUNK_MAX = 8192;
constexpr int LARS_MAX_BLOCKS = 2048;

// The chunks [first, first + n) of the plan are adaptive segment seg
struct LarsSeg {
  int seg, first, n;
};

// The scalar arithmetic of one variable, fp32 with no contraction, one IEEE sqrt per norm and one IEEE
// division: a numpy-float32 host mirror (ops.lars_trust_ref) gives the same bits from the same two sums.
// clip: the scale of a global-norm clip, which scales the gradient before the optimizer sees it (null: none)
__host__ __device__ __forceinline__ float lars_trust_eval(float sum_w, float sum_g, float eeta, float wd, float eps,
                                                          const float* clip) {
#pragma clang fp contract(off)
  const float wn = sqrtf(sum_w);
  float gn = sqrtf(sum_g);
  if (clip) gn = gn * *clip;
  return (wn > 0.f && gn > 0.f) ? eeta * wn / (gn + wd * wn + eps) : 1.f;
}

struct LarsArgs {
  const float* p;                                  // fp32 masters
  const float* g; const bf16* g16; float gscale;   // exactly one of g / g16
  const LarsChunk* plan; int nchunk;
  const LarsSeg* segs; int nadapt;                 // the adaptive segments, with their chunk ranges
  const float* wd;          // [nseg]: OptSeg::wd of every segment of the var list
  float eeta, eps;
  const float* clip_scale;  // nullable device scalar (launch_grad_sumsq's out[1])
  float* partials;          // [nchunk][2]: chunk c's (sum p^2, sum (gscale g)^2), whatever the grid
  uint32_t* ticket;         // zero-initialised; reset by the last workgroup
  float* sums;              // [nseg][2]: written for the adaptive segments only
  float* trust;             // [nseg]: written for the adaptive segments only - the others hold the 1.0f
                            // they were given at setup
  int max_blocks;           // 0: up to LARS_MAX_BLOCKS workgroups (a test forces 1)
};
void launch_layer_trust(const LarsArgs& a, hipStream_t s);

}  // namespace dtfe
