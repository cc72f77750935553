#pragma once
#include "common.h"

#include <stdexcept>

namespace dtfe {

enum OptKind : int { OPT_SGD = 0, OPT_MOMENTUM = 1, OPT_ADAM = 2, OPT_RMSPROP = 3 };

// A parameter segment of the flat fp32 master buffer.  The segment is viewed
// as [R][T][C]; wt16 (optional) receives the bf16 copy laid out as [C][T][R]
// (dense: W[out][in] -> Wt[in][out]; conv: W[cout][kh*kw][cin] -> Wt[cin][kh*kw][cout]).
struct OptSeg {
  long off;
  int R, T, C;
  float wd;    // coupled L2 weight decay of this segment (0: none); sits in the former padding after C
  bf16* w16;   // natural-layout bf16 working copy (nullable)
  bf16* wt16;  // transposed bf16 working copy (nullable)
  // second destinations of the updated values (nullable): a ps writes the requesting worker's
  // reply buffer from the apply itself - bf16 natural / transposed copies, or the fp32 value of
  // a variable without bf16 copies - instead of snapshotting its working copies afterwards
  bf16* w16b;
  bf16* wt16b;
  float* pb;
};

static_assert(sizeof(OptSeg) == 64, "OptSeg: wd fills the padding, the plan blobs keep their layout");

// Work item: kind 0 = flat range [start, start+count) of segment seg;
// kind 1 = 64x64 tile (r0, c0) of tap t of segment seg (transpose path).
struct OptWork {
  int kind, seg, t, r0, c0;
  long start, count;
};

// An optimizer plan is one device blob: nseg OptSeg, then the OptWork items at the next 256-B boundary
inline size_t opt_blob_work_offset(size_t nseg) { return (nseg * sizeof(OptSeg) + 255) / 256 * 256; }

// A learning-rate schedule evaluated on the device from *global_step (OptArgs::sched).  Integer compares
// and fp32 +, -, * only, no contraction: a numpy-float32 host mirror (ops.lr_schedule_value) gives the
// same bits.  The reciprocals are rounded to float32 on the host.
constexpr int LR_MAX_BOUNDS = 8;
enum LrKind : int { LR_CONSTANT = 0, LR_PIECEWISE = 1, LR_LINEAR = 2 };
struct LrSchedule {
  int kind;
  int nb;                          // piecewise: boundaries in use
  int bounds[LR_MAX_BOUNDS];       // strictly increasing
  float values[LR_MAX_BOUNDS + 1];
  float lr, end;                   // constant: lr; linear: from lr to end over decay_steps steps
  int decay_steps; float inv_decay;
  int warmup; float inv_warmup;    // warmup > 0: the rate times (step + 1) / warmup while step < warmup
};
static_assert(sizeof(LrSchedule) == 25 * 4, "LrSchedule: 25 four-byte fields, no padding");

// tf.train.piecewise_constant (values[i] for b[i-1] < step <= b[i]) / tf.train.polynomial_decay with
// power 1 and no cycling, each under an optional linear warm-up
// Branch-free over the boundaries (they increase, so the last one passed decides): nothing here is
// loaded depending on step, the struct and the step can be in flight together.
__host__ __device__ __forceinline__ float lr_schedule_eval(const LrSchedule& s, int step) {
#pragma clang fp contract(off)
  float v = s.lr;
  if (s.kind == LR_PIECEWISE) {
    v = s.values[0];
#pragma unroll
    for (int i = 0; i < LR_MAX_BOUNDS; ++i)
      if (i < s.nb && step > s.bounds[i]) v = s.values[i + 1];
  } else if (s.kind == LR_LINEAR) {
    const float t = (float)(step < s.decay_steps ? step : s.decay_steps);
    v = (s.lr - s.end) * (1.f - t * s.inv_decay) + s.end;
  }
  if (step < s.warmup) v = v * ((float)(step + 1) * s.inv_warmup);
  return v;
}

struct OptArgs {
  int kind;
  float* p;
  const float* g; const bf16* g16; float gscale;   // exactly one of g / g16
  float* s1; float* s2;                            // slots (adam: m, v; rmsprop: ms, mom; momentum: accum)
  float lr, beta1, beta2, eps, momentum, rho;
  float* beta_pow;          // adam: [beta1_power, beta2_power] (TF1 non-slot variables)
  int32_t* global_step; int gs_inc;
  uint32_t* done_counter;   // zero-initialised; reset by the last workgroup
  const OptSeg* segs; const OptWork* work; int nwork;
  int skip_advance;         // 1: leave the beta powers / global step alone (a partial apply: the
                            // ps applies a push bucket by bucket, then launch_opt_advance once)
  // ps reply folded into the launch (rep_slot != nullptr): after every workgroup's stores have
  // completed, the last one publishes (global step, version, stale, seq) into the worker's slot
  // of the shared page (ps_link.h), exactly as ps_reply_kernel would after this launch
  uint64_t* rep_slot;
  const int32_t* rep_gs;
  uint64_t rep_seq, rep_ver;
  int rep_stale;
  // optional device-side dependency (a gradient produced on another stream with no graph edge to this
  // launch): the work items of segments in wait_segs wait until *wait_done exceeds *wait_seen (set by
  // epoch_signal_kernel after the producer); the last workgroup then advances *wait_seen
  const int* wait_done; int* wait_seen; uint32_t wait_segs;
  // optional device scalar multiplied into gscale (nullable): the scale of a global-norm clip
  // (gradnorm.h, launch_grad_sumsq's out[1]).  Null: the arithmetic is exactly gscale's
  const float* clip_scale;
  // optional learning-rate schedule (nullable): every workgroup evaluates it at *global_step when it
  // starts and uses the result in place of lr.  Null: lr, and the arithmetic is exactly as without it
  const LrSchedule* sched;
  float* lr_out;            // nullable: the last workgroup stores the rate this launch used
  int nesterov;             // OPT_MOMENTUM: TF1 ApplyMomentum's use_nesterov form
  int decay;                // 1: some segment has wd != 0 (the kernels' weight-decay instantiation)
  // optional exponential moving average of the var list (tf.train.ExponentialMovingAverage), nullable: a
  // full-size flat buffer with p's offsets.  Every element the launch stores to p also updates its shadow,
  // shadow -= (shadow - p) * (1 - d), with d = ema_decay or, with ema_num_updates,
  // min(ema_decay, (1 + n) / (10 + n)) at n = *global_step + gs_inc (the step after this launch's advance).
  // Null: the kernels' instantiation without it, and the arithmetic is exactly as before there was one
  float* ema;
  float ema_decay;
  int ema_num_updates;
  float* ema_out;           // nullable: the last workgroup stores the decay this launch used
  // optional per-segment factor of the rate (nullable), indexed by a work item's seg: the item's rate is
  // lr_used * seg_lr[seg], one fp32 multiply (lr_used: the schedule's value, else lr) - the trust ratios of
  // the launch before this one on the stream (lars.h).  OPT_MOMENTUM only.  lr_out reports lr_used.
  // Null: the kernels' instantiation without it, and the arithmetic is exactly as before there was one
  const float* seg_lr;
};

// the decay of a launch and one element's update (TF1 assign_moving_average), fp32 with no contraction:
// a numpy-float32 host mirror (ops.ema_decay_value / ops.ema_update_ref) gives the same bits - the one
// division is IEEE-rounded (hipcc's default for fp32 division)
__host__ __device__ __forceinline__ float ema_decay_eval(float decay, int num_updates, int n) {
#pragma clang fp contract(off)
  if (!num_updates) return decay;
  const float r = (float)(1 + n) / (float)(10 + n);
  return r < decay ? r : decay;
}
__host__ __device__ __forceinline__ float ema_update(float shadow, float v, float omd) {
#pragma clang fp contract(off)
  return shadow - (shadow - v) * omd;
}
// points a.segs / a.work into a plan blob of nseg segments
inline void opt_blob_plan(const void* blob, size_t nseg, OptArgs& a) {
  a.segs = reinterpret_cast<const OptSeg*>(blob);
  a.work = reinterpret_cast<const OptWork*>(static_cast<const char*>(blob) + opt_blob_work_offset(nseg));
}
// *ctr += 1 (agent-scope release) - launched on the producer's stream right after the producer
void launch_epoch_signal(int* ctr, hipStream_t s);

void launch_apply_gradients(const OptArgs& a, hipStream_t s);
// exchanges p and ema over the optimizer's plan (a.segs / a.work) and rewrites the bf16 copies from the new
// p, as the apply lays them out; slots, step and counters are not touched.  Two swaps restore every buffer
void launch_ema_swap(const OptArgs& a, hipStream_t s);
// the non-slot scalars of one optimizer step: beta powers (Adam) and global_step += gs_inc
void launch_opt_advance(const OptArgs& a, hipStream_t s);
// the step scalars of n (<= OPT_GROUP_MAX) optimizers and then, if a[n-1].rep_slot is set, its
// reply words - one launch (a ps request whose gradient was all applied bucket by bucket)
void launch_opt_advance_reply(const OptArgs* a, int n, hipStream_t s);

// TF1 Adam step of one element: m = b1 m + (1-b1) g; v2 = b2 v2 + (1-b2) g^2; p -= lr_t m / (sqrt(v2) + eps).
// No multiply-add contraction: the rounding must not depend on a kernel's instruction selection.
__device__ __forceinline__ float tf1_adam(float p, float g, float& m, float& v2, float lr_t, float beta1, float beta2,
                                          float eps) {
#pragma clang fp contract(off)
  m = m * beta1 + (1.f - beta1) * g;
  v2 = v2 * beta2 + (1.f - beta2) * g * g;
  return p - lr_t * m / (sqrtf(v2) + eps);
}
__device__ __forceinline__ float tf1_adam_lr(float lr, const float* beta_pow) {
#pragma clang fp contract(off)
  return lr * sqrtf(1.f - beta_pow[1]) / (1.f - beta_pow[0]);
}

// up to OPT_GROUP_MAX optimizers of one kind in a single launch (contiguous workgroup ranges)
constexpr int OPT_GROUP_MAX = 4;
struct OptGroup {
  OptArgs o[OPT_GROUP_MAX];
  int first[OPT_GROUP_MAX + 1];
  int n;
};
void launch_apply_gradients_group(const OptArgs* o, int n, hipStream_t s);

}  // namespace dtfe
