// torch.ops.dtfe_rnn.* bindings: the persistent GRU sequence kernels (csrc/kernels/gru_seq.hip), single and stacked,
// the bidirectional layer's paired-direction kernels (csrc/kernels/gru_bidir.hip), and the layer-normalised LSTM
// sequence kernels (csrc/kernels/lnlstm_seq.hip).
//
// As in torch_ops.cpp, every tensor goes through one TensorArgs (tensor_args.h): device, dtype and the exact
// extent the kernel reads or writes are checked before a pointer leaves it, so a refused call has written nothing.
#include <ATen/ATen.h>
#include <torch/library.h>

#include <cstdint>

#include "../kernels/gru_seq.h"
#include "../kernels/lnlstm_seq.h"
#include "tensor_args.h"

using at::Tensor;
using c10::optional;
using dtfe::at_least;
using dtfe::exactly;
using dtfe::has;
using dtfe::TensorArgs;

namespace {

// the two kernels (Wg [I+H][2H], bg [2H], Wc [I+H][H], bc [H]) of a cell with the sizes already in `a`
void gru_weights(const TensorArgs& t, dtfe::GruSeqArgs& a, const Tensor& Wg, const Tensor& Wc) {
  const int64_t KT = a.I + a.H;
  a.Wg = t.in<float>(Wg, "Wg", exactly(KT * 2 * a.H));
  a.Wc = t.in<float>(Wc, "Wc", exactly(KT * a.H));
}

// optional second destination of every h_t: h2 [T][B][pitch >= H], h_t in the first H columns of row (t, b)
void gru_h2(const TensorArgs& t, dtfe::GruSeqArgs& a, const optional<Tensor>& h2, const char* op) {
  if (!has(h2)) return;
  TORCH_CHECK(h2->dim() == 3 && h2->size(0) == a.T && h2->size(1) == a.B && h2->size(2) >= a.H, op,
              ": h2 [T][B][pitch >= H]");
  a.h2p = (int)h2->size(2);
  a.h2 = t.out<float>(*h2, "h2", exactly((int64_t)a.T * a.B * a.h2p));
}

// whole-sequence GRU forward: false (nothing written) when the shape is outside the kernel's (H = 128, I = 28,
// B % 16 == 0)
bool gru_seq_fwd(const Tensor& xh, const Tensor& xrh, const Tensor& Wg, const Tensor& bg, const Tensor& Wc,
                 const Tensor& bc, const Tensor& g, const Tensor& cand, const Tensor& hT, const optional<Tensor>& h2) {
  const TensorArgs t("gru_seq_fwd", xh, "xh");
  TORCH_CHECK(xh.dim() == 3 && hT.dim() == 2 && xh.size(2) > hT.size(1) && xh.size(0) >= 1 && hT.size(0) == xh.size(1),
              "gru_seq_fwd: xh [T][B][I+H] f32, hT [B][H]");
  dtfe::GruSeqArgs a{};
  a.T = (int)xh.size(0); a.B = (int)xh.size(1); a.H = (int)hT.size(1); a.I = (int)xh.size(2) - a.H;
  const int64_t TB = (int64_t)a.T * a.B;
  a.xh = t.out<float>(xh, "xh", exactly(TB * (a.I + a.H)));
  a.xrh = t.out<float>(xrh, "xrh", exactly(TB * (a.I + a.H)));
  gru_weights(t, a, Wg, Wc);
  a.bg = t.in<float>(bg, "bg", exactly(2 * a.H)); a.bc = t.in<float>(bc, "bc", exactly(a.H));
  a.g = t.out<float>(g, "g", exactly(TB * 2 * a.H)); a.cand = t.out<float>(cand, "cand", exactly(TB * a.H));
  a.hT = t.out<float>(hT, "hT", exactly((int64_t)a.B * a.H));
  gru_h2(t, a, h2, "gru_seq_fwd");
  return dtfe::launch_gru_seq_fwd(a, t.stream());
}

// the forward of a stacked layer over projected inputs xpg [T][B][2H] = x . Wg[:I] + bg, xpc [T][B][H] = x . Wc[:I] + bc:
// false (nothing written) outside H = 128, I % 4 == 0, B % 16 == 0
bool gru_proj_fwd(const Tensor& xh, const Tensor& xrh, const Tensor& xpg, const Tensor& xpc, const Tensor& Wg,
                  const Tensor& Wc, const Tensor& g, const Tensor& cand, const Tensor& hT, const optional<Tensor>& h2) {
  const TensorArgs t("gru_proj_fwd", xh, "xh");
  TORCH_CHECK(xh.dim() == 3 && hT.dim() == 2 && xh.size(2) > hT.size(1) && xh.size(0) >= 1 && hT.size(0) == xh.size(1),
              "gru_proj_fwd: xh [T][B][I+H] f32, hT [B][H]");
  dtfe::GruSeqArgs a{};
  a.T = (int)xh.size(0); a.B = (int)xh.size(1); a.H = (int)hT.size(1); a.I = (int)xh.size(2) - a.H;
  const int64_t TB = (int64_t)a.T * a.B;
  a.xh = t.out<float>(xh, "xh", exactly(TB * (a.I + a.H)));
  a.xrh = t.out<float>(xrh, "xrh", exactly(TB * (a.I + a.H)));
  // the x columns go from xh to xrh in 16-byte pieces
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.xh) % 16 == 0 && reinterpret_cast<uintptr_t>(a.xrh) % 16 == 0,
              "gru_proj_fwd: xh and xrh must be 16-byte aligned");
  a.xpg = t.in<float>(xpg, "xpg", exactly(TB * 2 * a.H)); a.xpc = t.in<float>(xpc, "xpc", exactly(TB * a.H));
  gru_weights(t, a, Wg, Wc);
  a.g = t.out<float>(g, "g", exactly(TB * 2 * a.H)); a.cand = t.out<float>(cand, "cand", exactly(TB * a.H));
  a.hT = t.out<float>(hT, "hT", exactly((int64_t)a.B * a.H));
  gru_h2(t, a, h2, "gru_proj_fwd");
  return dtfe::launch_gru_proj_fwd(a, t.stream());
}

// whole-sequence GRU BPTT; dh_T is dhT, or dl . W_out^T when dl / wo (the fused head's dlogits) are given
bool gru_seq_bwd(const Tensor& xh, const Tensor& Wg, const Tensor& Wc, const Tensor& g, const Tensor& cand,
                 const Tensor& dhT, const Tensor& dgg, const Tensor& dgc, const optional<Tensor>& dl,
                 const optional<Tensor>& wo) {
  const TensorArgs t("gru_seq_bwd", cand, "cand");
  TORCH_CHECK(cand.dim() == 3 && cand.size(0) >= 1 && xh.dim() == 3 && xh.size(2) > cand.size(2),
              "gru_seq_bwd: cand [T][B][H], xh [T][B][I+H]");
  dtfe::GruSeqArgs a{};
  a.T = (int)cand.size(0); a.B = (int)cand.size(1); a.H = (int)cand.size(2); a.I = (int)xh.size(2) - a.H;
  const int64_t TB = (int64_t)a.T * a.B;
  a.xh = const_cast<float*>(t.in<float>(xh, "xh", exactly(TB * (a.I + a.H))));
  gru_weights(t, a, Wg, Wc);
  // the kernel reads the recurrent rows with 16-byte loads
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.Wg) % 16 == 0 && reinterpret_cast<uintptr_t>(a.Wc) % 16 == 0,
              "gru_seq_bwd: Wg and Wc must be 16-byte aligned");
  a.g = const_cast<float*>(t.in<float>(g, "g", exactly(TB * 2 * a.H)));
  a.cand = const_cast<float*>(t.in<float>(cand, "cand", exactly(TB * a.H)));
  a.dhT = t.in<float>(dhT, "dhT", exactly((int64_t)a.B * a.H));
  a.dgg = t.out<float>(dgg, "dgg", exactly(TB * 2 * a.H)); a.dgc = t.out<float>(dgc, "dgc", exactly(TB * a.H));
  if (has(dl)) {
    TORCH_CHECK(has(wo) && wo->dim() == 2 && wo->size(0) == a.H && dl->dim() == 2 && dl->size(0) == a.B &&
                    dl->size(1) == wo->size(1), "gru_seq_bwd: dl [B][NC] with W_out [H][NC]");
    a.dl = t.in<float>(dl, "dl", exactly(dl->numel())); a.wo = t.in<float>(wo, "wo", exactly(wo->numel()));
    a.nc = (int)wo->size(1);
  }
  return dtfe::launch_gru_seq_bwd(a, t.stream());
}

// BPTT of one layer of a stack (any I % 4 == 0): dh_t = carry + dhs[t] with dhs [T][B][H] the gradient arriving at
// every output h_t (the layer above's dx); the recurrence starts from dhT, or dl . W_out^T, or zeros when neither is given
bool gru_stack_bwd(const Tensor& xh, const Tensor& Wg, const Tensor& Wc, const Tensor& g, const Tensor& cand,
                   const Tensor& dgg, const Tensor& dgc, const optional<Tensor>& dhs, const optional<Tensor>& dhT,
                   const optional<Tensor>& dl, const optional<Tensor>& wo) {
  const TensorArgs t("gru_stack_bwd", cand, "cand");
  TORCH_CHECK(cand.dim() == 3 && cand.size(0) >= 1 && xh.dim() == 3 && xh.size(2) > cand.size(2),
              "gru_stack_bwd: cand [T][B][H], xh [T][B][I+H]");
  TORCH_CHECK(has(dhs) || has(dhT) || has(dl), "gru_stack_bwd: no gradient given (dhs, dhT or dl / wo)");
  dtfe::GruSeqArgs a{};
  a.T = (int)cand.size(0); a.B = (int)cand.size(1); a.H = (int)cand.size(2); a.I = (int)xh.size(2) - a.H;
  const int64_t TB = (int64_t)a.T * a.B;
  a.xh = const_cast<float*>(t.in<float>(xh, "xh", exactly(TB * (a.I + a.H))));
  gru_weights(t, a, Wg, Wc);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.Wg) % 16 == 0 && reinterpret_cast<uintptr_t>(a.Wc) % 16 == 0,
              "gru_stack_bwd: Wg and Wc must be 16-byte aligned");
  a.g = const_cast<float*>(t.in<float>(g, "g", exactly(TB * 2 * a.H)));
  a.cand = const_cast<float*>(t.in<float>(cand, "cand", exactly(TB * a.H)));
  a.dgg = t.out<float>(dgg, "dgg", exactly(TB * 2 * a.H)); a.dgc = t.out<float>(dgc, "dgc", exactly(TB * a.H));
  a.dhs = t.in<float>(dhs, "dhs", exactly(TB * a.H));
  a.dhT = t.in<float>(dhT, "dhT", exactly((int64_t)a.B * a.H));
  if (has(dl)) {
    TORCH_CHECK(has(wo) && wo->dim() == 2 && wo->size(0) == a.H && dl->dim() == 2 && dl->size(0) == a.B &&
                    dl->size(1) == wo->size(1), "gru_stack_bwd: dl [B][NC] with W_out [H][NC]");
    a.dl = t.in<float>(dl, "dl", exactly(dl->numel())); a.wo = t.in<float>(wo, "wo", exactly(wo->numel()));
    a.nc = (int)wo->size(1);
  }
  return dtfe::launch_gru_stack_bwd(a, t.stream());
}

// the four variables of both directions of a bidirectional layer (separate tensors: fw / bw variables of the model)
void gru_bidir_weights(const TensorArgs& t, dtfe::GruBidirArgs& a, const Tensor* const (&Wg)[2],
                       const Tensor* const (&Wc)[2]) {
  static const char* const gname[2] = {"Wg0", "Wg1"};
  static const char* const cname[2] = {"Wc0", "Wc1"};
  const int64_t KT = a.I + a.H;
  for (int d = 0; d < 2; ++d) {
    a.Wg[d] = t.in<float>(*Wg[d], gname[d], exactly(KT * 2 * a.H));
    a.Wc[d] = t.in<float>(*Wc[d], cname[d], exactly(KT * a.H));
  }
}

// both directions of a bidirectional GRU layer in one launch (gru_bidir.hip): every buffer [2][T][B][..], feat [B][2H];
// false (nothing written) outside H = 128, I = 28, B % 16 == 0
bool gru_bidir_fwd(const Tensor& xh, const Tensor& xrh, const Tensor& Wg0, const Tensor& bg0, const Tensor& Wc0,
                   const Tensor& bc0, const Tensor& Wg1, const Tensor& bg1, const Tensor& Wc1, const Tensor& bc1,
                   const Tensor& g, const Tensor& cand, const Tensor& feat) {
  const TensorArgs t("gru_bidir_fwd", xh, "xh");
  TORCH_CHECK(xh.dim() == 4 && xh.size(0) == 2 && xh.size(1) >= 1 && feat.dim() == 2 && feat.size(1) % 2 == 0 &&
                  xh.size(3) > feat.size(1) / 2 && feat.size(0) == xh.size(2),
              "gru_bidir_fwd: xh [2][T][B][I+H] f32, feat [B][2H]");
  dtfe::GruBidirArgs a{};
  a.T = (int)xh.size(1); a.B = (int)xh.size(2); a.H = (int)feat.size(1) / 2; a.I = (int)xh.size(3) - a.H;
  const int64_t TB2 = 2 * (int64_t)a.T * a.B;
  a.xh = t.out<float>(xh, "xh", exactly(TB2 * (a.I + a.H)));
  a.xrh = t.out<float>(xrh, "xrh", exactly(TB2 * (a.I + a.H)));
  gru_bidir_weights(t, a, {&Wg0, &Wg1}, {&Wc0, &Wc1});
  a.bg[0] = t.in<float>(bg0, "bg0", exactly(2 * a.H)); a.bc[0] = t.in<float>(bc0, "bc0", exactly(a.H));
  a.bg[1] = t.in<float>(bg1, "bg1", exactly(2 * a.H)); a.bc[1] = t.in<float>(bc1, "bc1", exactly(a.H));
  a.g = t.out<float>(g, "g", exactly(TB2 * 2 * a.H)); a.cand = t.out<float>(cand, "cand", exactly(TB2 * a.H));
  a.feat = t.out<float>(feat, "feat", exactly((int64_t)a.B * 2 * a.H));
  return dtfe::launch_gru_bidir_fwd(a, t.stream());
}

// BPTT of both directions in one launch; direction d starts from columns d H .. of dhT [B][2H], or from
// dl . wo[d H : (d + 1) H]^T when dl [B][NC] / wo [2H][NC] (the fused head's dlogits) are given
bool gru_bidir_bwd(const Tensor& xh, const Tensor& Wg0, const Tensor& Wc0, const Tensor& Wg1, const Tensor& Wc1,
                   const Tensor& g, const Tensor& cand, const Tensor& dhT, const Tensor& dgg, const Tensor& dgc,
                   const optional<Tensor>& dl, const optional<Tensor>& wo) {
  const TensorArgs t("gru_bidir_bwd", cand, "cand");
  TORCH_CHECK(cand.dim() == 4 && cand.size(0) == 2 && cand.size(1) >= 1 && xh.dim() == 4 && xh.size(3) > cand.size(3),
              "gru_bidir_bwd: cand [2][T][B][H], xh [2][T][B][I+H]");
  dtfe::GruBidirArgs a{};
  a.T = (int)cand.size(1); a.B = (int)cand.size(2); a.H = (int)cand.size(3); a.I = (int)xh.size(3) - a.H;
  const int64_t TB2 = 2 * (int64_t)a.T * a.B;
  a.xh = const_cast<float*>(t.in<float>(xh, "xh", exactly(TB2 * (a.I + a.H))));
  gru_bidir_weights(t, a, {&Wg0, &Wg1}, {&Wc0, &Wc1});
  // the kernel reads the recurrent rows with 16-byte loads
  for (int d = 0; d < 2; ++d)
    TORCH_CHECK(reinterpret_cast<uintptr_t>(a.Wg[d]) % 16 == 0 && reinterpret_cast<uintptr_t>(a.Wc[d]) % 16 == 0,
                "gru_bidir_bwd: Wg and Wc of both directions must be 16-byte aligned");
  a.g = const_cast<float*>(t.in<float>(g, "g", exactly(TB2 * 2 * a.H)));
  a.cand = const_cast<float*>(t.in<float>(cand, "cand", exactly(TB2 * a.H)));
  a.dhT = t.in<float>(dhT, "dhT", exactly((int64_t)a.B * 2 * a.H));
  a.dgg = t.out<float>(dgg, "dgg", exactly(TB2 * 2 * a.H)); a.dgc = t.out<float>(dgc, "dgc", exactly(TB2 * a.H));
  if (has(dl)) {
    TORCH_CHECK(has(wo) && wo->dim() == 2 && wo->size(0) == 2 * a.H && dl->dim() == 2 && dl->size(0) == a.B &&
                    dl->size(1) == wo->size(1), "gru_bidir_bwd: dl [B][NC] with W_out [2H][NC]");
    a.dl = t.in<float>(dl, "dl", exactly(dl->numel())); a.wo = t.in<float>(wo, "wo", exactly(wo->numel()));
    a.nc = (int)wo->size(1);
  }
  return dtfe::launch_gru_bidir_bwd(a, t.stream());
}

// whole-sequence layer-normalised LSTM forward (lnlstm_seq.hip): false (nothing written) outside H = 128, I = 28,
// B % 16 == 0, B >= 16
bool lnlstm_seq_fwd(const Tensor& xh, const Tensor& K, const Tensor& ln, const Tensor& zhat, const Tensor& chat,
                    const Tensor& rs, const Tensor& hT, double forget_bias) {
  const TensorArgs t("lnlstm_seq_fwd", xh, "xh");
  TORCH_CHECK(xh.dim() == 3 && hT.dim() == 2 && xh.size(2) > hT.size(1) && xh.size(0) >= 1 && hT.size(0) == xh.size(1),
              "lnlstm_seq_fwd: xh [T][B][I+H] f32, hT [B][H]");
  dtfe::LnLstmSeqArgs a{};
  a.T = (int)xh.size(0); a.B = (int)xh.size(1); a.H = (int)hT.size(1); a.I = (int)xh.size(2) - a.H;
  a.forget_bias = (float)forget_bias;
  const int64_t TB = (int64_t)a.T * a.B;
  a.xh = t.out<float>(xh, "xh", exactly(TB * (a.I + a.H)));
  a.K = t.in<float>(K, "K", exactly((int64_t)(a.I + a.H) * 4 * a.H));
  a.ln = t.in<float>(ln, "ln", exactly((int64_t)dtfe::LNLSTM_NLN * a.H));
  a.zhat = t.out<float>(zhat, "zhat", exactly(TB * 4 * a.H));
  a.chat = t.out<float>(chat, "chat", exactly(TB * a.H));
  a.rs = t.out<float>(rs, "rs", exactly(TB * dtfe::LNLSTM_NRS));
  a.hT = t.out<float>(hT, "hT", exactly((int64_t)a.B * a.H));
  return dtfe::launch_lnlstm_seq_fwd(a, t.stream());
}

// whole-sequence layer-normalised LSTM BPTT; dh_T is dhT, or dl . W_out^T when dl / wo are given.  ws holds one
// [10][H] slab of gamma / beta gradients per 16-row workgroup
bool lnlstm_seq_bwd(const Tensor& K, const Tensor& ln, const Tensor& zhat, const Tensor& chat, const Tensor& rs,
                    const Tensor& dhT, const Tensor& dg, const Tensor& dln, const Tensor& ws,
                    const optional<Tensor>& dl, const optional<Tensor>& wo, double forget_bias) {
  const TensorArgs t("lnlstm_seq_bwd", chat, "chat");
  TORCH_CHECK(chat.dim() == 3 && chat.size(0) >= 1 && K.dim() == 2 && K.size(0) > chat.size(2),
              "lnlstm_seq_bwd: chat [T][B][H], K [I+H][4H]");
  dtfe::LnLstmSeqArgs a{};
  a.T = (int)chat.size(0); a.B = (int)chat.size(1); a.H = (int)chat.size(2); a.I = (int)K.size(0) - a.H;
  a.forget_bias = (float)forget_bias;
  const int64_t TB = (int64_t)a.T * a.B;
  a.K = t.in<float>(K, "K", exactly((int64_t)(a.I + a.H) * 4 * a.H));
  // the kernel reads the recurrent rows with 16-byte loads
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.K) % 16 == 0, "lnlstm_seq_bwd: K must be 16-byte aligned");
  a.ln = t.in<float>(ln, "ln", exactly((int64_t)dtfe::LNLSTM_NLN * a.H));
  a.zhat = const_cast<float*>(t.in<float>(zhat, "zhat", exactly(TB * 4 * a.H)));
  a.chat = const_cast<float*>(t.in<float>(chat, "chat", exactly(TB * a.H)));
  a.rs = const_cast<float*>(t.in<float>(rs, "rs", exactly(TB * dtfe::LNLSTM_NRS)));
  a.dhT = t.in<float>(dhT, "dhT", exactly((int64_t)a.B * a.H));
  a.dg = t.out<float>(dg, "dg", exactly(TB * 4 * a.H));
  a.dln = t.out<float>(dln, "dln", exactly((int64_t)dtfe::LNLSTM_NLN * a.H));
  a.ws = t.out<float>(ws, "ws", at_least((int64_t)(a.B / 16) * dtfe::LNLSTM_NLN * a.H));
  if (has(dl)) {
    TORCH_CHECK(has(wo) && wo->dim() == 2 && wo->size(0) == a.H && dl->dim() == 2 && dl->size(0) == a.B &&
                    dl->size(1) == wo->size(1), "lnlstm_seq_bwd: dl [B][NC] with W_out [H][NC]");
    a.dl = t.in<float>(dl, "dl", exactly(dl->numel())); a.wo = t.in<float>(wo, "wo", exactly(wo->numel()));
    a.nc = (int)wo->size(1);
  }
  return dtfe::launch_lnlstm_seq_bwd(a, t.stream());
}

}  // namespace

TORCH_LIBRARY(dtfe_rnn, m) {
  m.def("lnlstm_seq_fwd(Tensor(a!) xh, Tensor K, Tensor ln, Tensor(b!) zhat, Tensor(c!) chat, Tensor(d!) rs,"
        " Tensor(e!) hT, float forget_bias=1.0) -> bool");
  m.def("lnlstm_seq_bwd(Tensor K, Tensor ln, Tensor zhat, Tensor chat, Tensor rs, Tensor dhT, Tensor(a!) dg,"
        " Tensor(b!) dln, Tensor(c!) ws, Tensor? dl=None, Tensor? wo=None, float forget_bias=1.0) -> bool");
  m.def("gru_seq_fwd(Tensor(a!) xh, Tensor(b!) xrh, Tensor Wg, Tensor bg, Tensor Wc, Tensor bc, Tensor(c!) g,"
        " Tensor(d!) cand, Tensor(e!) hT, Tensor(f!)? h2=None) -> bool");
  m.def("gru_seq_bwd(Tensor xh, Tensor Wg, Tensor Wc, Tensor g, Tensor cand, Tensor dhT, Tensor(a!) dgg,"
        " Tensor(b!) dgc, Tensor? dl=None, Tensor? wo=None) -> bool");
  m.def("gru_proj_fwd(Tensor(a!) xh, Tensor(b!) xrh, Tensor xpg, Tensor xpc, Tensor Wg, Tensor Wc, Tensor(c!) g,"
        " Tensor(d!) cand, Tensor(e!) hT, Tensor(f!)? h2=None) -> bool");
  m.def("gru_stack_bwd(Tensor xh, Tensor Wg, Tensor Wc, Tensor g, Tensor cand, Tensor(a!) dgg, Tensor(b!) dgc,"
        " Tensor? dhs=None, Tensor? dhT=None, Tensor? dl=None, Tensor? wo=None) -> bool");
  m.def("gru_bidir_fwd(Tensor(a!) xh, Tensor(b!) xrh, Tensor Wg0, Tensor bg0, Tensor Wc0, Tensor bc0, Tensor Wg1,"
        " Tensor bg1, Tensor Wc1, Tensor bc1, Tensor(c!) g, Tensor(d!) cand, Tensor(e!) feat) -> bool");
  m.def("gru_bidir_bwd(Tensor xh, Tensor Wg0, Tensor Wc0, Tensor Wg1, Tensor Wc1, Tensor g, Tensor cand, Tensor dhT,"
        " Tensor(a!) dgg, Tensor(b!) dgc, Tensor? dl=None, Tensor? wo=None) -> bool");
}

TORCH_LIBRARY_IMPL(dtfe_rnn, CUDA, m) {
  m.impl("lnlstm_seq_fwd", &lnlstm_seq_fwd);
  m.impl("lnlstm_seq_bwd", &lnlstm_seq_bwd);
  m.impl("gru_seq_fwd", &gru_seq_fwd);
  m.impl("gru_seq_bwd", &gru_seq_bwd);
  m.impl("gru_proj_fwd", &gru_proj_fwd);
  m.impl("gru_stack_bwd", &gru_stack_bwd);
  m.impl("gru_bidir_fwd", &gru_bidir_fwd);
  m.impl("gru_bidir_bwd", &gru_bidir_bwd);
}
