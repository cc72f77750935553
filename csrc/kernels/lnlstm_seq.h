// Persistent whole-sequence layer-normalised LSTM forward / BPTT (TF1 tf.contrib.rnn.LayerNormBasicLSTMCell),
// lnlstm_seq.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfe {

constexpr int LNLSTM_NLN = 10;  // layer-norm vectors: gamma, beta of input, transform, forget_gate, output, state
constexpr int LNLSTM_NRS = 5;   // reciprocal standard deviations per (step, row): the four gates, then the state

struct LnLstmSeqArgs {
  int T, B, I, H;
  // [T][B][I+H]: x_t columns and the h_{-1} columns of step 0 given; the forward writes the h_{t-1} columns of
  // steps 1..T-1 (the kernel gradient's A operand)
  float* xh;
  const float* K;    // [I+H][4H] (rows x then h; columns gates i, j, f, o); no bias
  const float* ln;   // [10][H]: row 2k gamma, row 2k + 1 beta of k = i, j, f, o, state
  float forget_bias;
  float* zhat;       // [T][B][4H] normalised gate pre-activations, before gamma / beta (forward out, backward in)
  float* chat;       // [T][B][H] normalised cell state, before gamma / beta (forward out, backward in)
  float* rs;         // [T][B][5] reciprocal standard deviations of i, j, f, o, state (forward out, backward in)
  float* hT;         // [B][H] last hidden state
  const float* dhT;  // [B][H] d loss / d h_T (backward in), unless dl is given:
  // dh_T formed in the kernel as dl . W_out^T - dl [B][nc] (the classifier head's dlogits), W_out [H][nc]
  const float* dl; const float* wo; int nc;
  float* dg;         // [T][B][4H] gradient of the raw gate pre-activations z (backward out)
  float* dln;        // [10][H] gradient of ln (backward out)
  float* ws;         // [B/16][10][H] one slab of gamma / beta gradients per workgroup, summed into dln in workgroup order
};

// false, with nothing launched or written, outside H = 128, I = 28, T >= 1, B >= 16, B % 16 == 0.
// The backward reads the recurrent rows of K with 16-byte loads.
bool launch_lnlstm_seq_fwd(const LnLstmSeqArgs& a, hipStream_t s);
bool launch_lnlstm_seq_bwd(const LnLstmSeqArgs& a, hipStream_t s);

}  // namespace dtfe
