#pragma once
#include "common.h"

namespace dtfe {

// The running totals of one evaluation pass over n examples in chunks of B rows: one contiguous
// block of 64-bit words on the device, so the host reads the whole result in a single copy.
struct EvalState {
  long cursor;      // chunks folded so far: the next launch scores rows [cursor * B, cursor * B + B)
  long n;           // examples in the pass (set by the host before the first chunk, >= 1)
  long count;       // rows folded (bad-label rows included)
  long hits1;       // rows whose label ranks first
  long hitsk;       // rows whose label ranks among the first k
  long bad_labels;  // rows whose label lies outside [0, NC): counted, no loss, no hit
  double loss_sum;  // sum of the rows' cross-entropy, added in row order in double
};
constexpr int EVAL_STATE_WORDS = 7;

// One chunk of an evaluation (eval.hip).  valid = clamp(n - cursor * B, 0, B) rows are in play; the
// rows behind them may hold anything.  valid == 0: the launch changes nothing.
struct EvalMetricsArgs {
  const float* logits;    // [B][NC]
  const int32_t* labels;  // [B]
  int B, NC, k;           // 1 <= k <= NC
  EvalState* state;
  int32_t* idx;           // optional [B]: receives the next chunk's rows, min(cursor' * B + b, n - 1)
  uint32_t* ws;           // [2 * B]: row b's loss bits in ws[b], its flag bits in ws[B + b]
  uint32_t* ticket;       // zero-initialised; reset by the last workgroup
};
void launch_eval_metrics(const EvalMetricsArgs& a, hipStream_t s);

}  // namespace dtfe
