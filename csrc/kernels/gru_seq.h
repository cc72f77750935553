// Persistent whole-sequence GRU forward / BPTT (TF1 tf.nn.rnn_cell.GRUCell), gru_seq.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfe {

struct GruSeqArgs {
  int T, B, I, H;
  // [T][B][I+H]: x_t columns and the h_{-1} columns of step 0 given; the forward writes the h_{t-1} columns
  // of steps 1..T-1 (backward in: h_{t-1})
  float* xh;
  float* xrh;        // [T][B][I+H] forward out: x_t columns copied, then r_t * h_{t-1} (the candidate GEMM's rows)
  const float* Wg;   // [I+H][2H] gates kernel (rows x then h; columns r then u)
  const float* bg;   // [2H]
  const float* Wc;   // [I+H][H] candidate kernel (rows x then r * h)
  const float* bc;   // [H]
  float* g;          // [T][B][2H] activated r, u (forward out, backward in)
  float* cand;       // [T][B][H] tanh candidate (forward out, backward in)
  float* hT;         // [B][H] last hidden state
  const float* dhT;  // [B][H] d loss / d h_T (backward in), unless dl is given:
  // dh_T formed in the kernel as dl . W_out^T - dl [B][nc] (the classifier head's dlogits), W_out [H][nc]
  const float* dl; const float* wo; int nc;
  float* dgg;        // [T][B][2H] gate pre-activation grads (backward out)
  float* dgc;        // [T][B][H] candidate pre-activation grads (backward out)
  // optional second destination of every h_t (both forward kernels): h2[(t B + b) h2p + u], the x columns of the
  // xh buffer of a layer stacked on this one (h2p = its I' + H)
  float* h2; int h2p;
  // the projected-input forward: x_t . Wg[:I] + bg [T][B][2H] and x_t . Wc[:I] + bc [T][B][H] (bg / bc unused)
  const float* xpg; const float* xpc;
  // the stacked backward: optional d loss / d h_t arriving at every step [T][B][H] (the layer above's dx_t)
  const float* dhs;
};

// false, with nothing launched or written, for a shape outside H = 128, I = 28, B % 16 == 0
bool launch_gru_seq_fwd(const GruSeqArgs& a, hipStream_t s);
bool launch_gru_seq_bwd(const GruSeqArgs& a, hipStream_t s);

// The kernels of a stacked layer: any I % 4 == 0 (I is only the row offset of the recurrent rows and part of the xh
// pitch), H = 128, B % 16 == 0; false with nothing launched otherwise.
//   forward over projected inputs: the x part of both GEMMs arrives as xpg / xpc, the recurrence multiplies only
//   by the recurrent rows; xh, xrh 16-byte aligned (the x columns are copied xh -> xrh in 16-byte pieces).
//   backward: dh_t = carry + dhs[t]; the recurrence starts from dhT or dl . wo^T when given, else from zeros.
bool launch_gru_proj_fwd(const GruSeqArgs& a, hipStream_t s);
bool launch_gru_stack_bwd(const GruSeqArgs& a, hipStream_t s);

// A bidirectional layer, both directions in one launch (gru_bidir.hip).  Every buffer has a leading direction axis:
// d = 0 runs forward in time, d = 1 backward in time, and row t of direction d belongs to time t.
struct GruBidirArgs {
  int T, B, I, H;
  // [2][T][B][I+H].  xh[0]: as GruSeqArgs::xh.  xh[1]: only the initial state given, in the h columns of step T-1; the
  // forward reads x_t from xh[0], writes it into the x columns of xh[1][t] and its h into the h columns of step t-1,
  // so xh[1][t] = [x_t | h_bw(t+1)].  Neither direction writes its initial-state columns.
  float* xh;
  float* xrh;           // [2][T][B][I+H] forward out: [x_t | r_t * (the state step t starts from)]
  const float* Wg[2];   // per direction [I+H][2H]
  const float* bg[2];   // [2H]
  const float* Wc[2];   // [I+H][H]
  const float* bc[2];   // [H]
  float* g;             // [2][T][B][2H]
  float* cand;          // [2][T][B][H]
  float* feat;          // [B][2H] forward out: d = 0's state after time T-1 | d = 1's state after time 0
  // backward in: d loss / d feat [B][2H], unless dl [B][nc] and wo [2H][nc] are given (direction d starts from
  // dl . wo[d H : (d + 1) H]^T, formed in the kernel)
  const float* dhT;
  const float* dl; const float* wo; int nc;
  float* dgg;           // [2][T][B][2H] backward out
  float* dgc;           // [2][T][B][H] backward out
};

// grid (B / 16, 2); false, with nothing launched or written, outside H = 128, I = 28, T >= 1, B >= 16, B % 16 == 0.
// The backward reads the recurrent rows of Wg / Wc with 16-byte loads.
bool launch_gru_bidir_fwd(const GruBidirArgs& a, hipStream_t s);
bool launch_gru_bidir_bwd(const GruBidirArgs& a, hipStream_t s);

}  // namespace dtfe
