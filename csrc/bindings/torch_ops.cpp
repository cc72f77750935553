// torch.ops.dtfe.* bindings for the gfx950 kernel library.
//
// Every op writes into caller-provided (pre-allocated) tensors and launches on
// the current HIP stream, so a whole training step built from these ops can be
// captured into a hipGraph (torch.cuda.CUDAGraph) with zero allocations.
//
// The kernels trust their pointers completely, so every tensor argument of every op goes through
// one TensorArgs (tensor_args.h): device, dtype and extent are checked before a pointer leaves it,
// and the extent is what the kernel reads or writes.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <torch/custom_class.h>
#include <torch/library.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../kernels/augment.h"
#include "../kernels/conv.h"
#include "../kernels/conv_f32.h"
#include "../kernels/imgconv.h"
#include "../kernels/norm.h"
#include "../kernels/elementwise.h"
#include "../kernels/eval.h"
#include "../kernels/gemm_dense.h"
#include "../kernels/head.h"
#include "../kernels/lstm_seq.h"
#include "../kernels/gradnorm.h"
#include "../kernels/lars.h"
#include "../kernels/optim.h"
#include "opt_state.h"
#include "tensor_args.h"

using at::Tensor;
using c10::optional;
using dtfe::at_least;
using dtfe::exactly;
using dtfe::has;
using dtfe::spans;
using dtfe::TensorArgs;

namespace {

// ------------------------------------------------------------------- gemm
// torch.classes.dtfe.GemmGroup: the pieces of one grouped launch (gemm_dense.h), added by gemm /
// head_wgrad calls that name the group, plus references to the tensors whose pointers the pieces
// hold - kept until launch() or clear().  Destroying a non-empty group launches nothing.
struct GemmGroupObj : torch::CustomClassHolder {
  dtfe::GemmGroup g;
  std::vector<Tensor> held;
  int dev = -1;  // device index of the pieces
  void hold(const Tensor& t) { held.push_back(t); }
  void hold(const optional<Tensor>& t) { if (has(t)) held.push_back(*t); }
  // a piece on the device of tensor `on`: add(g) records it (false: it does not fit, the caller launches it now)
  template <typename F, typename... T>
  bool join(F&& add, const Tensor& on, const T&... rest) {
    TORCH_CHECK(dev < 0 || dev == on.get_device(), "gemm group: a piece on device ", on.get_device(),
                " cannot join a group on device ", dev);
    if (!add(g)) return false;
    dev = on.get_device();
    (hold(on), ..., hold(rest));
    return true;
  }
  void clear() { g = dtfe::GemmGroup(); held.clear(); dev = -1; }
  void launch() {  // on the pieces' device (made current) and its current stream; an empty group does nothing
    if (g.pieces()) {
      const c10::DeviceGuard guard(c10::Device(c10::kCUDA, (c10::DeviceIndex)dev));
      dtfe::launch_gemm_group(g, at::hip::getCurrentHIPStream(dev).stream());
    }
    clear();
  }
  int64_t pieces() const { return g.pieces(); }
};
using GroupArg = optional<c10::intrusive_ptr<GemmGroupObj>>;

void gemm(const Tensor& A, int64_t amode, int64_t lda, const Tensor& B, int64_t bmode, int64_t ldb, int64_t M,
          int64_t N, int64_t K, const Tensor& out, int64_t ldc, const optional<Tensor>& bias, int64_t bias_axis,
          int64_t act, double alpha, double beta, bool atomic, int64_t splits, int64_t tile,
          const optional<Tensor>& aux, int64_t ld_aux, int64_t aux_act, int64_t b_ones_row, double keep, int64_t seed,
          const optional<Tensor>& counter, const optional<Tensor>& pooled, const optional<Tensor>& argmax,
          int64_t PH, int64_t PW, int64_t PC, const optional<Tensor>& out2, int64_t ldc2, bool out2_trans,
          const optional<Tensor>& bias_out, const optional<Tensor>& ws, const optional<Tensor>& tile_ctr,
          int64_t a_ones_row, const optional<Tensor>& ones, const GroupArg& group) {
  const TensorArgs t("gemm", out, "out");
  TORCH_CHECK(A.scalar_type() == B.scalar_type(), "gemm: A and B dtypes differ");
  TORCH_CHECK(a_ones_row < 0 || b_ones_row < 0, "gemm: at most one of a_ones_row / b_ones_row");
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && lda >= 0 && ldb >= 0 && ldc >= 0, "gemm: M, N, K >= 1 and leading dimensions >= 0");
  // every kernel reads whole operand rows with no bounds checks beyond M / N / K: every element they may
  // touch must lie inside the tensors.  A trailing ones row reads as 1.0 and has no memory behind it; with
  // bias_out its output row / column goes there and not to out / aux / out2
  const int64_t a_rows = a_ones_row == M - 1 ? M - 1 : M, b_rows = b_ones_row == N - 1 ? N - 1 : N;
  const int64_t c_rows = has(bias_out) ? a_rows : M, c_cols = has(bias_out) ? b_rows : N;
  const int64_t c_need = (c_rows - 1) * ldc + c_cols;
  dtfe::DenseGemmArgs a{};
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  const dtfe::AnyPtr pa = t.any(A, "A", dtfe::F32_OR_BF16, spans(amode == 0 ? (a_rows - 1) * lda + K : (K - 1) * lda + a_rows));
  const int dt = pa.f32() ? 1 : 0;
  a.A = pa.p; a.lda = lda;
  a.B = t.any(B, "B", dtfe::F32_OR_BF16, spans(bmode == 0 ? (b_rows - 1) * ldb + K : (K - 1) * ldb + b_rows)).p;
  a.ldb = ldb;
  a.b_ones_row = (int)b_ones_row;
  a.a_ones_row = (int)a_ones_row;
  if (splits < 1) splits = 1;
  int bm = 0, bn = 0;
  const int kt = dtfe::gemm_dense_tile_dims((int)tile, bm, bn);
  TORCH_CHECK(kt > 0, "gemm: bad tile id");
  int chunk = (int)((K + splits - 1) / splits);
  chunk = ((chunk + kt - 1) / kt) * kt;
  if (chunk < kt) chunk = kt;
  const int real_splits = (int)((K + chunk - 1) / chunk);
  a.k_chunk = chunk;
  a.unpool = has(pooled) ? 1 : 0;
  if (a.unpool) {  // out is the bf16 [B][2PH][2PW][C] tensor that the pooled [M][N] gradient is routed into
    TORCH_CHECK(has(argmax) && PH >= 1 && PW >= 1 && PC >= 1, "gemm: the unpool epilogue needs argmax and PH, PW, PC");
    a.out = t.out<dtfe::bf16>(out, "out", at_least(4 * c_need));
    a.up.pooled = t.in<dtfe::bf16>(pooled, "pooled", at_least(c_need));
    a.up.argmax = t.in<uint8_t>(argmax, "argmax", at_least(c_need));
    a.up.PH = (int)PH; a.up.PW = (int)PW; a.up.C = (int)PC;
  } else {
    const dtfe::AnyPtr po = t.any(out, "out", dtfe::F32_OR_BF16, spans(c_need));
    a.out = po.p; a.out_f32 = po.f32();
  }
  a.ldc = ldc;
  a.bias = t.in<float>(bias, "bias", at_least(bias_axis ? M : N)); a.bias_axis = (int)bias_axis;
  a.act = (int)act; a.alpha = (float)alpha; a.beta = (float)beta; a.atomic = atomic;
  if (real_splits > 1 && !atomic) {
    const int64_t ntiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    TORCH_CHECK(has(ws) && has(tile_ctr), "gemm: split-K with a fused epilogue needs ws/tile_ctr");
    a.ws = t.out<float>(ws, "ws (the split-K workspace)", at_least(real_splits * ntiles * bm * bn));
    a.tile_ctr = t.out<int32_t>(tile_ctr, "tile_ctr (the split-K tile counters)", at_least(ntiles));
  }
  TORCH_CHECK(!atomic || a.out_f32, "gemm: atomic accumulation needs an fp32 output");
  const dtfe::AnyPtr p2 = t.any(out2, "out2", dtfe::F32_OR_BF16,
                                spans(out2_trans ? (c_cols - 1) * ldc2 + c_rows : (c_rows - 1) * ldc2 + c_cols));
  a.out2 = p2.p; a.ldc2 = ldc2; a.out2_f32 = p2.f32(); a.out2_trans = out2_trans;
  const dtfe::AnyPtr px = t.any(aux, "aux", dtfe::F32_OR_BF16, spans((c_rows - 1) * ld_aux + c_cols));
  a.aux = px.p; a.ld_aux = ld_aux; a.aux_f32 = px.f32(); a.aux_act = (int)aux_act;
  a.keep = (float)keep; a.seed = (uint64_t)seed; a.counter = t.in<int64_t>(counter, "counter", at_least(1));
  a.bias_out = t.out<float>(bias_out, "bias_out", at_least(a_ones_row >= 0 ? N : M));
  TORCH_CHECK(!a.bias_out || b_ones_row >= 0 || a_ones_row >= 0, "gemm: bias_out needs a ones row");
  a.ones = t.in<dtfe::bf16>(ones, "ones", at_least(512));  // the 1 KB page of ops.ones_page
  if (tile == dtfe::GEMM_TILE_SMALL) {
    TORCH_CHECK(real_splits == 1 && dtfe::gemm_small_eligible(dt, a),
                "gemm: the small-tile kernel takes fp32 operands, one split, no un-pool epilogue");
  } else if (tile >= 5) {
    TORCH_CHECK(dtfe::gemm_glds_eligible(dt, (int)amode, (int)bmode, (int)tile, a),
                "gemm: shape / layout not eligible for the global_load_lds tile ", tile);
  }
  auto add = [&](dtfe::GemmGroup& g) {
    return dtfe::gemm_group_add(g, dt, (int)amode, (int)bmode, (int)tile, real_splits, a);
  };  // (a piece has one split: no ws / tile_ctr to hold)
  if (group.has_value() && (*group)->join(add, out, A, B, bias, aux, counter, pooled, argmax, out2, bias_out, ones))
    return;
  dtfe::launch_gemm_dense(dt, (int)amode, (int)bmode, (int)tile, real_splits, a, t.stream());
}

// ------------------------------------------------------------------- conv
dtfe::ConvGeom geom(int64_t B, int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t OH, int64_t OW, int64_t KH,
                    int64_t KW, int64_t stride, int64_t pad, int64_t pool) {
  TORCH_CHECK(std::min({B, H, W, C, Cout, OH, OW, KH, KW, stride}) >= 1 && pad >= 0, "conv: geometry must be positive");
  dtfe::ConvGeom g;
  g.B = (int)B; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.Cout = (int)Cout; g.OH = (int)OH; g.OW = (int)OW;
  g.KH = (int)KH; g.KW = (int)KW; g.stride = (int)stride; g.pad = (int)pad; g.pool_order = (int)pool;
  return g;
}

void conv_fwd(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, const Tensor& y,
              const optional<Tensor>& argmax, int64_t B, int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t OH,
              int64_t OW, int64_t KH, int64_t KW, int64_t stride, int64_t pad, bool pool, int64_t act,
              const optional<Tensor>& bn_stats) {
  const TensorArgs t("conv_fwd", x, "x");
  const int64_t nx = B * H * W * C, nw = Cout * KH * KW * C, ny = B * OH * OW * Cout / (pool ? 4 : 1);
  if (x.scalar_type() == at::kFloat) {  // exact-fp32 path (--dtype fp32): conv_f32.hip
    TORCH_CHECK(!has(bn_stats), "conv_fwd (fp32): fp32 x / w / y, no BatchNorm statistics");
    TORCH_CHECK(!pool || ((OH | OW) & 1) == 0, "conv_fwd (fp32): pool needs even output dims");
    dtfe::ConvF32Args f{};
    f.g = geom(B, H, W, C, Cout, OH, OW, KH, KW, stride, pad, pool);
    f.src = t.in<float>(x, "x", exactly(nx)); f.w = t.in<float>(w, "w", exactly(nw));
    f.bias = t.in<float>(bias, "bias", at_least(Cout));
    f.out = t.out<float>(y, "y", exactly(ny)); f.argmax = t.out<uint8_t>(argmax, "argmax", at_least(ny)); f.act = (int)act;
    dtfe::launch_conv_fwd_f32(f, t.stream());
    return;
  }
  dtfe::ConvFwdArgs a{};
  a.bn_stats = t.out<float>(bn_stats, "bn_stats", at_least(2 * Cout));
  a.g = geom(B, H, W, C, Cout, OH, OW, KH, KW, stride, pad, pool);
  a.x = t.in<dtfe::bf16>(x, "x", at_least(nx));
  a.w = t.in<dtfe::bf16>(w, "w", at_least(nw));
  a.bias = t.in<float>(bias, "bias", at_least(Cout));
  a.y = t.out<dtfe::bf16>(y, "y", at_least(ny));
  a.argmax = t.out<uint8_t>(argmax, "argmax", at_least(ny));
  a.act = (int)act;
  dtfe::launch_conv_fwd(a, t.stream());
}

void conv_dgrad(const Tensor& dy, const Tensor& wt, const Tensor& dx, int64_t B, int64_t H, int64_t W, int64_t C,
                int64_t Cout, int64_t OH, int64_t OW, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                const optional<Tensor>& pooled, const optional<Tensor>& argmax, const optional<Tensor>& relu_mask,
                bool accumulate, const optional<Tensor>& bnb_x, const optional<Tensor>& bnb_y,
                const optional<Tensor>& bnb_mean, const optional<Tensor>& bnb_invstd, const optional<Tensor>& bnb_gamma,
                const optional<Tensor>& bnb_beta, const optional<Tensor>& bnb_stats, int64_t bnb_act,
                const optional<Tensor>& acc_src, const optional<Tensor>& acc_mask) {
  const TensorArgs t("conv_dgrad", dy, "dy");
  const int64_t ndx = B * H * W * C, ndy = B * OH * OW * Cout, nw = C * KH * KW * Cout;
  if (dy.scalar_type() == at::kFloat) {  // exact-fp32 path (--dtype fp32): conv_f32.hip
    TORCH_CHECK(stride == 1 && !accumulate && !has(pooled) && !has(bnb_stats),
                "conv_dgrad (fp32): fp32 tensors, stride 1, optional ReLU mask only");
    dtfe::ConvF32Args f{};
    f.g = geom(B, H, W, C, Cout, OH, OW, KH, KW, stride, pad, 0);
    f.src = t.in<float>(dy, "dy", exactly(ndy)); f.w = t.in<float>(wt, "wt", exactly(nw));
    f.out = t.out<float>(dx, "dx", exactly(ndx));
    f.relu_mask = t.in<float>(relu_mask, "relu_mask", exactly(ndx));
    dtfe::launch_conv_dgrad_f32(f, t.stream());
    return;
  }
  dtfe::ConvDgradArgs a{};
  a.accumulate = accumulate ? 1 : 0;
  a.unpool = has(pooled) ? 1 : 0;
  // with the un-pool epilogue [B][H][W][C] is the pooled tensor and dx its [B][2H][2W][C] source
  const int64_t nout = a.unpool ? 4 * ndx : ndx;
  if (has(bnb_stats)) {
    TORCH_CHECK(has(bnb_x) && has(bnb_mean) && has(bnb_invstd) && has(bnb_gamma),
                "conv_dgrad: BN-backward statistics need x, mean, invstd, gamma");
    a.bnb_x = t.in<dtfe::bf16>(bnb_x, "bnb_x", exactly(dx.numel()));
    // the forward output (bf16), or its uint8 [R][C/8] ReLU bit mask
    if (has(bnb_y) && bnb_y->scalar_type() == at::kByte) a.bnb_ymask = t.in<uint8_t>(bnb_y, "bnb_y", exactly(dx.numel() / 8));
    else a.bnb_y = t.in<dtfe::bf16>(bnb_y, "bnb_y", exactly(dx.numel()));
    a.bnb_mean = t.in<float>(bnb_mean, "bnb_mean", at_least(C));
    a.bnb_invstd = t.in<float>(bnb_invstd, "bnb_invstd", at_least(C));
    a.bnb_gamma = t.in<float>(bnb_gamma, "bnb_gamma", at_least(C));
    a.bnb_beta = t.in<float>(bnb_beta, "bnb_beta", at_least(C));
    a.bnb_stats = t.out<float>(bnb_stats, "bnb_stats", at_least(2 * C));
    a.bnb_act = (int)bnb_act;
  }
  if (has(acc_src)) {
    TORCH_CHECK(accumulate && has(acc_mask), "conv_dgrad: acc_src (bf16, dx's shape) needs accumulate and its uint8 [R][C/8] bit mask");
    a.acc_src = t.in<dtfe::bf16>(acc_src, "acc_src", exactly(dx.numel()));
    a.acc_mask = t.in<uint8_t>(acc_mask, "acc_mask", exactly(dx.numel() / 8));
  }
  a.g = geom(B, H, W, C, Cout, OH, OW, KH, KW, stride, pad, 0);
  a.dy = t.in<dtfe::bf16>(dy, "dy", at_least(ndy));
  a.wt = t.in<dtfe::bf16>(wt, "wt", at_least(nw));
  a.dx = t.out<dtfe::bf16>(dx, "dx", at_least(nout));
  a.relu_mask = t.in<dtfe::bf16>(relu_mask, "relu_mask", at_least(ndx));
  if (a.unpool) {
    TORCH_CHECK(has(argmax), "conv_dgrad: pooled needs argmax");
    a.up.pooled = t.in<dtfe::bf16>(pooled, "pooled", at_least(ndx));
    a.up.argmax = t.in<uint8_t>(argmax, "argmax", at_least(ndx));
    a.up.PH = (int)H; a.up.PW = (int)W; a.up.C = (int)C;
  }
  dtfe::launch_conv_dgrad(a, t.stream());
}

// [stats, gamma, beta, mean, invstd, moving_mean, moving_var] of a BatchNorm + ReLU formed on a
// whole-image conv's source (the last four may be undefined: nothing saved / updated)
dtfe::BnSrc bn_src_of(const TensorArgs& t, const optional<at::TensorList>& l, long R, int64_t C, double eps,
                      double momentum, bool save) {
  dtfe::BnSrc b{};
  if (!l.has_value() || l->empty()) return b;
  TORCH_CHECK(l->size() == 7, "bn_src: [stats, gamma, beta, mean, invstd, moving_mean, moving_var]");
  const auto& v = *l;
  b.stats = t.out<float>(v[0], "bn_src[0] (stats)", at_least(2 * C));
  b.gamma = t.in<float>(v[1], "bn_src[1] (gamma)", at_least(C));
  b.beta = t.in<float>(v[2], "bn_src[2] (beta)", at_least(C));
  static const char* const names[7] = {"", "", "", "bn_src[3] (mean)", "bn_src[4] (invstd)", "bn_src[5] (moving_mean)",
                                       "bn_src[6] (moving_var)"};
  auto saved = [&](int i) { return save && v[i].defined() ? t.out<float>(v[i], names[i], at_least(C)) : nullptr; };
  b.mean = saved(3); b.invstd = saved(4); b.moving_mean = saved(5); b.moving_var = saved(6);
  TORCH_CHECK((b.moving_mean == nullptr) == (b.moving_var == nullptr), "bn_src: both moving averages or neither");
  b.R = R; b.eps = (float)eps; b.momentum = (float)momentum;
  return b;
}

// the B .. pad geometry fields that ImgConvArgs and ImgWgradArgs share
template <typename A>
void img_geom(A& a, int64_t B, int64_t SH, int64_t SW, int64_t CS, int64_t OH, int64_t OW, int64_t N, int64_t KH,
              int64_t KW, int64_t stride, int64_t pad) {
  TORCH_CHECK(std::min({B, SH, SW, CS, OH, OW, N, KH, KW, stride}) >= 1 && pad >= 0, "imgconv: geometry must be positive");
  a.B = (int)B; a.SH = (int)SH; a.SW = (int)SW; a.CS = (int)CS; a.OH = (int)OH; a.OW = (int)OW; a.N = (int)N;
  a.KH = (int)KH; a.KW = (int)KW; a.stride = (int)stride; a.pad = (int)pad;
}

bool imgconv(const optional<Tensor>& src, const optional<Tensor>& src_pooled, const optional<Tensor>& src_argmax,
             const Tensor& w, const optional<Tensor>& bias, const Tensor& y, const optional<Tensor>& argmax,
             const optional<Tensor>& relu_mask, int64_t B, int64_t SH, int64_t SW, int64_t CS, int64_t OH, int64_t OW,
             int64_t N, int64_t KH, int64_t KW, int64_t stride, int64_t pad, bool flip_taps, int64_t act, bool pool,
             int64_t dil, const optional<Tensor>& sc_src, int64_t sc_stride, const optional<Tensor>& tstamp,
             const optional<at::TensorList>& bn_src, double bn_eps, double bn_momentum, bool bn_save) {
  const TensorArgs t("imgconv", w, "w");
  TORCH_CHECK(has(src) != has(src_pooled), "imgconv: exactly one of src / src_pooled");
  TORCH_CHECK(has(src) || has(src_argmax), "imgconv: src_pooled needs src_argmax");
  dtfe::ImgConvArgs a{};
  img_geom(a, B, SH, SW, CS, OH, OW, N, KH, KW, stride, pad);
  a.flip_taps = flip_taps;
  a.dil = (int)dil;
  const int64_t ny = B * OH * OW * N / (pool ? 4 : 1), npooled = B * (SH / 2) * (SW / 2) * CS;
  a.src = t.in<dtfe::bf16>(src, "src", at_least(B * SH * SW * CS));
  a.src_pooled = t.in<dtfe::bf16>(src_pooled, "src_pooled", at_least(npooled));
  a.src_argmax = t.in<uint8_t>(src_argmax, "src_argmax", at_least(npooled));
  a.w = t.in<dtfe::bf16>(w, "w", exactly(N * KH * KW * CS));
  a.bias = t.in<float>(bias, "bias", at_least(N));
  a.act = (int)act; a.pool = pool;
  a.y = t.out<dtfe::bf16>(y, "y", exactly(ny));
  a.argmax = t.out<uint8_t>(argmax, "argmax", at_least(ny));
  a.relu_mask = t.in<dtfe::bf16>(relu_mask, "relu_mask", at_least(ny));
  a.tstamp = t.out<uint64_t>(tstamp, "tstamp", at_least(8 * std::min<int64_t>(B, 256)));  // [grid][8]
  a.bns = bn_src_of(t, bn_src, (long)B * SH * SW, CS, bn_eps, bn_momentum, bn_save);
  TORCH_CHECK(!a.bns.stats || a.src, "imgconv: BN-on-load needs a plain source");
  if (has(sc_src)) {
    TORCH_CHECK(sc_stride >= 1 && OH % sc_stride == 0 && OW % sc_stride == 0 && sc_src->dim() == 4 &&
                    sc_src->size(0) == B && sc_src->size(1) == OH / sc_stride && sc_src->size(2) == OW / sc_stride &&
                    sc_src->size(3) >= N,
                "imgconv: shortcut gradient [B][OH/s][OW/s][>= N]");
    a.sc_src = t.in<dtfe::bf16>(sc_src, "sc_src", exactly(sc_src->numel()));
    a.sc_stride = (int)sc_stride;
    a.sc_C = (int)sc_src->size(3);
  }
  return dtfe::launch_imgconv(a, t.stream());
}

// MNIST conv1 forward with the step's batch sampling fused in (imgconv1_copies.hip): samples B rows
// of the uint8 dataset, writes the bf16 images to x (the weight gradient's input) and the labels,
// clears the accumulators in `zero`, and runs conv1 + bias + ReLU + 2x2 max-pool(+argmax).
dtfe::ImgConvArgs conv1_gather_args(const TensorArgs& t, const Tensor& images, const Tensor& labels_src, int64_t seed,
                                    const Tensor& counter, const Tensor& done, const Tensor& labels_dst, const Tensor& x,
                                    const Tensor& w, const optional<Tensor>& bias, const Tensor& y, const Tensor& argmax,
                                    at::TensorList zero) {
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784 && images.size(0) >= 1, "conv1_gather_fwd: uint8 [rows][784] dataset");
  TORCH_CHECK(x.numel() % 784 == 0 && x.numel() >= 784, "conv1_gather_fwd: bf16 x [B][28][28]");
  dtfe::ImgConvArgs a{};
  const int64_t B = x.numel() / 784;
  img_geom(a, B, 28, 28, 1, 28, 28, 32, 5, 5, 1, 2);
  a.dil = 1;
  a.src = t.out<dtfe::bf16>(x, "x", exactly(B * 784));
  a.w = t.in<dtfe::bf16>(w, "w", exactly(32 * 25));
  a.bias = t.in<float>(bias, "bias", at_least(32));
  a.act = dtfe::ACT_RELU; a.pool = 1;
  a.y = t.out<dtfe::bf16>(y, "y", exactly(B * 14 * 14 * 32));
  a.argmax = t.out<uint8_t>(argmax, "argmax", exactly(B * 14 * 14 * 32));
  a.g_src = t.in<uint8_t>(images, "images", exactly(images.size(0) * 784)); a.g_rows = images.size(0);
  a.g_seed = (uint64_t)seed;
  // an empty `done` leaves the counter alone (the caller advances it later in the step)
  a.g_counter = t.out<int64_t>(counter, "counter", at_least(1));
  a.g_done = done.numel() ? t.out<uint32_t>(done, "done", at_least(1)) : nullptr;
  a.g_labels_src = t.in<int32_t>(labels_src, "labels_src", at_least(a.g_rows));
  a.g_labels_dst = t.out<int32_t>(labels_dst, "labels_dst", at_least(B));
  t.zero_ranges(zero, a.zptr, a.zlen, a.nz);
  return a;
}

void conv1_gather_fwd(const Tensor& images, const Tensor& labels_src, int64_t seed, const Tensor& counter,
                      const Tensor& done, const Tensor& labels_dst, const Tensor& x, const Tensor& w,
                      const optional<Tensor>& bias, const Tensor& y, const Tensor& argmax, at::TensorList zero) {
  const TensorArgs t("conv1_gather_fwd", images, "images");
  const dtfe::ImgConvArgs a = conv1_gather_args(t, images, labels_src, seed, counter, done, labels_dst, x, w, bias, y,
                                                argmax, zero);
  TORCH_CHECK(dtfe::launch_conv1_copies_fwd(a, t.stream()), "conv1_gather_fwd: needs B >= 256");
}

// conv1_gather_fwd and MNIST conv2's forward (w2 [64][25][32], +bias, ReLU, 2x2 max-pool(+argmax) -> p2 / a2)
// as ONE persistent launch (imgconv12_fused.hip): the same x, labels, p1 / a1 (y / argmax) and p2 / a2 as the
// two launches, bit for bit.
void conv12_gather_fwd(const Tensor& images, const Tensor& labels_src, int64_t seed, const Tensor& counter,
                       const Tensor& done, const Tensor& labels_dst, const Tensor& x, const Tensor& w,
                       const optional<Tensor>& bias, const Tensor& y, const Tensor& argmax, at::TensorList zero,
                       const Tensor& w2, const optional<Tensor>& bias2, const Tensor& p2, const Tensor& a2) {
  const TensorArgs t("conv12_gather_fwd", images, "images");
  const dtfe::ImgConvArgs a = conv1_gather_args(t, images, labels_src, seed, counter, done, labels_dst, x, w, bias, y,
                                                argmax, zero);
  const int64_t n2 = (int64_t)a.B * 7 * 7 * 64;
  TORCH_CHECK(dtfe::launch_conv12_fused_fwd(a, t.in<dtfe::bf16>(w2, "w2", exactly(64 * 25 * 32)),
                                            t.in<float>(bias2, "bias2", at_least(64)),
                                            t.out<dtfe::bf16>(p2, "p2", exactly(n2)), t.out<uint8_t>(a2, "a2", exactly(n2)),
                                            t.stream()),
              "conv12_gather_fwd: needs B >= 256");
}

// defer: the persistent kernel leaves its partial-slab reduce to a later wgrad_reduce_group and the call
// returns that reduce's descriptor [nblk, plen, MT, CTW, KC, N]; empty: the reduce (if any) already ran
std::vector<int64_t> imgwgrad(const Tensor& src, const optional<Tensor>& dy, const optional<Tensor>& dy_pooled,
                              const optional<Tensor>& dy_argmax, const Tensor& dw, const optional<Tensor>& db,
                              int64_t B, int64_t SH, int64_t SW, int64_t CS, int64_t OH, int64_t OW, int64_t N,
                              int64_t KH, int64_t KW, int64_t stride, int64_t pad, double scale,
                              const optional<Tensor>& ws, int64_t max_blocks, const optional<at::TensorList>& bn_src,
                              double bn_eps, bool defer) {
  const TensorArgs t("imgwgrad", src, "src");
  dtfe::ImgWgradArgs a{};
  img_geom(a, B, SH, SW, CS, OH, OW, N, KH, KW, stride, pad);
  a.defer_reduce = defer ? 1 : 0;
  a.bns = bn_src_of(t, bn_src, (long)B * SH * SW, CS, bn_eps, 0.0, false);
  a.max_blocks = (int)max_blocks;
  a.ws = t.out<float>(ws, "ws (ops.wgrad_ws_floats)", at_least(dtfe::imgwgrad_ws_floats((int)N, (int)(KH * KW * CS))));
  const int64_t npooled = B * (OH / 2) * (OW / 2) * N;
  a.src = t.in<dtfe::bf16>(src, "src", at_least(B * SH * SW * CS));
  a.dy = t.in<dtfe::bf16>(dy, "dy", at_least(B * OH * OW * N));
  a.dy_pooled = t.in<dtfe::bf16>(dy_pooled, "dy_pooled", at_least(npooled));
  a.dy_argmax = t.in<uint8_t>(dy_argmax, "dy_argmax", at_least(npooled));
  TORCH_CHECK((a.dy != nullptr) != (a.dy_pooled != nullptr), "imgwgrad: exactly one of dy / dy_pooled");
  TORCH_CHECK(a.dy || a.dy_argmax, "imgwgrad: dy_pooled needs dy_argmax");
  a.dw = t.out<float>(dw, "dw", exactly(N * KH * KW * CS));
  a.db = t.out<float>(db, "db", at_least(N));
  a.scale = (float)scale;
  dtfe::WpReduceItem r;
  dtfe::launch_imgwgrad(a, t.stream(), r);
  if (r.nblk == 0) return {};
  return {r.nblk, r.plen, r.MT, r.CTW, r.KC, r.N};
}

// the reduces that imgwgrad(defer=True) calls left out (desc: their six ints each, in order; every item
// its own workspace) as ONE grouped launch on the current stream
void wgrad_reduce_group(at::TensorList ws, at::TensorList dw, const c10::List<optional<Tensor>>& db,
                        at::ArrayRef<double> scale, at::IntArrayRef desc) {
  const size_t n = ws.size();
  TORCH_CHECK(n <= (size_t)dtfe::WP_GROUP_MAX, "wgrad_reduce_group: at most ", dtfe::WP_GROUP_MAX, " reduces");
  TORCH_CHECK(dw.size() == n && db.size() == n && scale.size() == n && desc.size() == 6 * n,
              "wgrad_reduce_group: one entry per reduce in every list");
  if (n == 0) return;
  const TensorArgs t("wgrad_reduce_group", ws[0], "ws");
  dtfe::WpReduceItem it[dtfe::WP_GROUP_MAX];
  for (size_t i = 0; i < n; ++i) {
    const int64_t* d = desc.data() + 6 * i;
    const optional<Tensor> b = db.get(i);
    TORCH_CHECK(d[0] > 0 && d[1] > 0 && d[4] > 0 && d[5] > 0, "wgrad_reduce_group: a descriptor of imgwgrad(defer=True)");
    it[i] = dtfe::WpReduceItem{t.in<float>(ws[i], "ws", at_least(d[0] * d[1])), t.out<float>(dw[i], "dw", exactly(d[5] * d[4])),
                               t.out<float>(b, "db", at_least(d[5])), (float)scale[i],
                               (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5]};
  }
  dtfe::launch_wgrad_reduce_group(it, (int)n, t.stream());
}

void conv_wgrad(const Tensor& dz, const Tensor& x, const Tensor& dw, const optional<Tensor>& db, int64_t B, int64_t H,
                int64_t W, int64_t C, int64_t Cout, int64_t OH, int64_t OW, int64_t KH, int64_t KW, int64_t stride,
                int64_t pad, double scale) {
  const TensorArgs t("conv_wgrad", dz, "dz");
  const int64_t ndz = B * OH * OW * Cout, nx = B * H * W * C, nw = Cout * KH * KW * C;
  if (dz.scalar_type() == at::kFloat) {  // exact-fp32 path (--dtype fp32): conv_f32.hip
    dtfe::ConvF32Args f{};
    f.g = geom(B, H, W, C, Cout, OH, OW, KH, KW, stride, pad, 0);
    f.src = t.in<float>(dz, "dz", exactly(ndz)); f.x = t.in<float>(x, "x", exactly(nx));
    f.dw = t.out<float>(dw, "dw", exactly(nw));
    f.db = t.out<float>(db, "db", at_least(Cout)); f.scale = (float)scale;
    dtfe::launch_conv_wgrad_f32(f, t.stream());
    return;
  }
  dtfe::ConvWgradArgs a{};
  a.g = geom(B, H, W, C, Cout, OH, OW, KH, KW, stride, pad, 0);
  a.dz = t.in<dtfe::bf16>(dz, "dz", at_least(ndz));
  a.x = t.in<dtfe::bf16>(x, "x", at_least(nx));
  a.dw = t.out<float>(dw, "dw", at_least(nw));
  a.db = t.out<float>(db, "db", at_least(Cout));
  a.scale = (float)scale;
  dtfe::launch_conv_wgrad(a, t.stream());
}

// 2x2 un-pool of a pooled fp32 gradient (argmax routing) and the [O][T][C] -> [C][T][O] weight
// transpose: the two data movers of the fp32 CNN step (conv_f32.hip)
void unpool_f32(const Tensor& g, const Tensor& argmax, const Tensor& out, int64_t B, int64_t PH, int64_t PW,
                int64_t C) {
  const TensorArgs t("unpool_f32", g, "g");
  const int64_t n = B * PH * PW * C;  // g [B][PH][PW][C], argmax alike, out [B][2PH][2PW][C]
  dtfe::launch_unpool_f32(t.in<float>(g, "g", exactly(n)), t.in<uint8_t>(argmax, "argmax", exactly(n)),
                          t.out<float>(out, "out", exactly(4 * n)), (int)B, (int)PH, (int)PW, (int)C, t.stream());
}

// MNIST conv1 weight gradient at fp32 from the pooled gradient (conv_f32.hip); false: shape not covered
bool conv1_wgrad_pooled_f32(const Tensor& dp, const Tensor& argmax, const Tensor& x, const Tensor& dw,
                            const optional<Tensor>& db, const Tensor& ws, int64_t B, int64_t H, int64_t W, int64_t K,
                            double scale) {
  const TensorArgs t("conv1_wgrad_pooled_f32", dp, "dp");
  const int64_t np = B * (H / 2) * (W / 2) * 32;  // dp [B][H/2][W/2][32], x [B][H][W][1], dw [32][K][K][1], db [32]
  const dtfe::ConvGeom g = geom(B, H, W, 1, 32, H, W, K, K, 1, K / 2, 0);
  return dtfe::launch_conv1_wgrad_pooled_f32(t.in<float>(dp, "dp", exactly(np)), t.in<uint8_t>(argmax, "argmax", exactly(np)),
                                             t.in<float>(x, "x", exactly(B * H * W)), t.out<float>(dw, "dw", exactly(32 * K * K)),
                                             t.out<float>(db, "db", exactly(32)), t.out<float>(ws, "ws", at_least(0)),
                                             ws.numel(), g, (float)scale, t.stream());
}

void transpose_taps_f32(const Tensor& in, const Tensor& out, int64_t O, int64_t T, int64_t C) {
  const TensorArgs t("transpose_taps_f32", in, "in");
  dtfe::launch_transpose_taps_f32(t.in<float>(in, "in", exactly(O * T * C)), t.out<float>(out, "out", exactly(O * T * C)),
                                  (int)O, (int)T, (int)C, t.stream());
}

// ------------------------------------------------------------------- head
// fp32 fused head (head.hip head_xent_f32_kernel); false: shape not instantiated (caller: GEMMs + softmax_xent)
bool head_xent_f32(const Tensor& h, const Tensor& w, const optional<Tensor>& b, const Tensor& labels, const Tensor& dz,
                   const Tensor& dl, const Tensor& loss_sum, const Tensor& correct, const optional<Tensor>& logits,
                   double scale, double inv_keep, const optional<Tensor>& step_counter) {
  const TensorArgs t("head_xent_f32", h, "h");
  TORCH_CHECK(h.dim() == 2 && w.dim() == 2 && w.size(1) == h.size(1), "head_xent_f32: fp32 h [B][K], W [NC][K]");
  dtfe::HeadF32Args a{};
  a.B = (int)h.size(0); a.K = (int)h.size(1); a.NC = (int)w.size(0);
  const int64_t nl = (int64_t)a.B * a.NC;
  a.h = t.in<float>(h, "h", exactly(h.numel())); a.w = t.in<float>(w, "w", exactly(w.numel()));
  a.b = t.in<float>(b, "b", at_least(a.NC));
  a.labels = t.in<int32_t>(labels, "labels", at_least(a.B));
  a.scale = (float)scale; a.inv_keep = (float)inv_keep;
  a.dz = t.out<float>(dz, "dz", exactly(h.numel())); a.dl = t.out<float>(dl, "dl", exactly(nl));
  a.logits_out = t.out<float>(logits, "logits", exactly(nl));
  a.loss_sum = t.out<float>(loss_sum, "loss_sum", at_least(1)); a.correct = t.out<int32_t>(correct, "correct", at_least(1));
  a.step_counter = t.out<int64_t>(step_counter, "step_counter", at_least(1));
  return dtfe::launch_head_xent_f32(a, t.stream());
}

void head_xent(const Tensor& h, const Tensor& w, const optional<Tensor>& b, const Tensor& labels, const Tensor& dz,
               const Tensor& dl, const optional<Tensor>& loss_sum, const optional<Tensor>& correct,
               const optional<Tensor>& logits, double scale, double inv_keep, const optional<Tensor>& step_counter,
               const optional<Tensor>& parts) {
  const TensorArgs t("head_xent", h, "h");
  TORCH_CHECK(h.dim() == 2 && h.size(1) >= 1 && dl.dim() == 2, "head_xent: bf16 h [B][K], dl [B][ld]");
  dtfe::HeadArgs a{};
  a.B = (int)h.size(0); a.K = (int)h.size(1); a.NC = (int)(w.numel() / a.K);
  TORCH_CHECK(dl.size(1) >= a.NC && dl.size(1) <= 64, "head_xent: dl row must hold NC classes");
  a.h = t.in<dtfe::bf16>(h, "h", exactly(h.numel()));
  a.w = t.in<dtfe::bf16>(w, "w", exactly((int64_t)a.NC * a.K));
  a.b = t.in<float>(b, "b", at_least(a.NC));
  a.labels = t.in<int32_t>(labels, "labels", at_least(a.B));
  a.scale = (float)scale; a.inv_keep = (float)inv_keep;
  a.dz = t.out<dtfe::bf16>(dz, "dz", at_least(h.numel()));
  a.dl = t.out<dtfe::bf16>(dl, "dl", at_least(a.B * dl.size(1))); a.ld_dl = (int)dl.size(1);
  a.loss_sum = t.out<float>(loss_sum, "loss_sum", at_least(1)); a.correct = t.out<int32_t>(correct, "correct", at_least(1));
  a.logits_out = t.out<float>(logits, "logits", at_least((int64_t)a.B * a.NC));
  a.step_counter = t.out<int64_t>(step_counter, "step_counter", at_least(1));
  a.parts = t.out<float>(parts, "parts", at_least(2 * ((a.B + 3) / 4)));  // [>= 2 * ceil(B / 4)]
  dtfe::launch_head_xent(a, t.stream());
}

void head_wgrad(const Tensor& dl, const Tensor& h, const Tensor& dw, const optional<Tensor>& db, int64_t nc,
                double scale, const optional<Tensor>& parts, const optional<Tensor>& loss_sum,
                const optional<Tensor>& correct, const GroupArg& group) {
  const TensorArgs t("head_wgrad", h, "h");
  TORCH_CHECK(dl.dim() == 2 && h.dim() == 2, "head_wgrad: bf16 dl [B][ld] and h [B][K]");
  TORCH_CHECK(dw.dim() == 2 && dw.size(0) == nc, "head_wgrad: fp32 dw [NC][>=K]");
  TORCH_CHECK(dl.size(0) == h.size(0) && dl.size(1) >= nc, "head_wgrad: batch / layout mismatch");
  dtfe::HeadWgradArgs a{};
  a.B = (int)h.size(0); a.K = (int)h.size(1); a.NC = (int)nc;
  TORCH_CHECK(dw.size(1) >= a.K, "head_wgrad: dw rows shorter than K");
  a.ld_dl = (int)dl.stride(0); a.ldh = (int)h.stride(0); a.ldw = (int)dw.stride(0);
  // the kernels read whole 16-B chunks: the first 16 columns of every dl row, K (% 8 == 0) of every h row
  a.dl = t.in<dtfe::bf16>(dl, "dl", spans((int64_t)(a.B - 1) * a.ld_dl + 16));
  a.h = t.in<dtfe::bf16>(h, "h", spans((int64_t)(a.B - 1) * a.ldh + a.K));
  a.dw = t.out<float>(dw, "dw", spans((nc - 1) * a.ldw + a.K));
  a.db = t.out<float>(db, "db", at_least(nc));
  a.scale = (float)scale;
  if (has(parts)) {
    TORCH_CHECK(has(loss_sum) && has(correct), "head_wgrad: parts need fp32 loss_sum and int32 correct");
    a.nparts = (a.B + 3) / 4;
    a.parts = t.in<float>(parts, "parts (head_xent's)", at_least(2 * a.nparts));
    a.loss_sum = t.out<float>(loss_sum, "loss_sum", at_least(1));
    a.correct = t.out<int32_t>(correct, "correct", at_least(1));
  }
  auto add = [&](dtfe::GemmGroup& g) { return dtfe::gemm_group_add_head(g, a); };
  if (group.has_value() && (*group)->join(add, h, dl, dw, db, parts, loss_sum, correct)) return;
  dtfe::launch_head_wgrad(a, t.stream());
}

// an optional tensor of a bound optimizer: checked, and held by the state for as long as its pointer is
template <typename T>
T* held_out(OptStateObj& o, const TensorArgs& t, const optional<Tensor>& x, const char* name, dtfe::Extent e) {
  T* p = t.out<T>(x, name, e);
  if (p) o.held.push_back(*x);
  return p;
}

}  // namespace

// -------------------------------------------------------------- optimizer
// torch.classes.dtfe.OptState (opt_state.h).  Everything a launch will dereference is checked here, once: the tensors (device, dtype, contiguity,
// length) and the plan (every segment inside p, every work item inside its segment).
OptStateObj::OptStateObj(int64_t kind, Tensor p, optional<Tensor> s1, optional<Tensor> s2, double beta1, double beta2,
                         double eps, double momentum, double rho, optional<Tensor> beta_pow,
                         optional<Tensor> global_step, Tensor done, const Tensor& segs_t, const Tensor& work_t,
                         const optional<Tensor>& wd, optional<Tensor> sched, optional<Tensor> lr_out, bool nesterov,
                         bool decay, optional<Tensor> ema, double ema_decay, bool ema_num_updates,
                         optional<Tensor> ema_out, optional<Tensor> seg_lr) {
  TORCH_CHECK(kind >= dtfe::OPT_SGD && kind <= dtfe::OPT_RMSPROP, "OptState: kind is 0 (sgd) .. 3 (rmsprop)");
  const TensorArgs t("OptState", p, "p");
  auto& a = args;
  a.kind = (int)kind;
  a.p = t.out<float>(p, "p", exactly(p.numel()));
  dev = p.get_device();
  numel = p.numel();
  held.push_back(p);
  a.s1 = held_out<float>(*this, t, s1, "s1", exactly(numel));
  a.s2 = held_out<float>(*this, t, s2, "s2", exactly(numel));
  a.beta1 = (float)beta1; a.beta2 = (float)beta2; a.eps = (float)eps; a.momentum = (float)momentum; a.rho = (float)rho;
  a.beta_pow = held_out<float>(*this, t, beta_pow, "beta_pow", at_least(2));
  a.global_step = held_out<int32_t>(*this, t, global_step, "global_step", at_least(1));
  a.done_counter = held_out<uint32_t>(*this, t, done, "done", at_least(1));
  TORCH_CHECK(a.done_counter, "OptState: done is required");
  if (kind == dtfe::OPT_ADAM) TORCH_CHECK(a.beta_pow && a.s1 && a.s2, "OptState: adam needs slots and beta powers");
  if (kind == dtfe::OPT_RMSPROP) TORCH_CHECK(a.s1 && a.s2, "OptState: rmsprop needs slots");
  if (kind == dtfe::OPT_MOMENTUM) TORCH_CHECK(a.s1, "OptState: momentum needs a slot");
  a.sched = reinterpret_cast<const dtfe::LrSchedule*>(held_out<uint8_t>(
      *this, t, sched, "sched (the blob of lr_schedule_pack)", exactly((int64_t)sizeof(dtfe::LrSchedule))));
  TORCH_CHECK(!a.sched || a.global_step, "OptState: a learning-rate schedule needs a global_step");
  a.lr_out = held_out<float>(*this, t, lr_out, "lr_out", at_least(1));
  TORCH_CHECK(!nesterov || kind == dtfe::OPT_MOMENTUM, "OptState: nesterov is for the momentum optimizer");
  a.nesterov = nesterov ? 1 : 0;
  a.decay = decay ? 1 : 0;
  // the shadow buffer of an exponential moving average: full size, p's offsets
  a.ema = held_out<float>(*this, t, ema, "ema", exactly(numel));
  a.ema_out = held_out<float>(*this, t, ema_out, "ema_out", at_least(1));
  if (a.ema) {
    TORCH_CHECK(a.ema != a.p, "OptState: ema is a buffer of its own, not p");
    TORCH_CHECK(ema_decay >= 0.0 && (float)ema_decay < 1.f, "OptState: ema_decay lies in [0, 1), got ", ema_decay);
    TORCH_CHECK(!ema_num_updates || a.global_step, "OptState: ema_num_updates needs a global_step");
    a.ema_decay = (float)ema_decay;
    a.ema_num_updates = ema_num_updates ? 1 : 0;
  } else {
    TORCH_CHECK(!a.ema_out && !ema_num_updates && ema_decay == 0.0, "OptState: ema_decay, ema_num_updates and ema_out "
                "need the ema buffer");
  }

  auto table = [](const Tensor& t, const char* name, int64_t cols) {
    TORCH_CHECK(t.device().is_cpu() && t.scalar_type() == at::kLong && t.dim() == 2 && t.size(1) == cols, "OptState: ",
                name, " is a CPU int64 [n, ", cols, "] table");
    return t.contiguous();
  };
  const Tensor S = table(segs_t, "segs", 6), W = table(work_t, "work", 7);
  const int64_t ns = S.size(0), nw = W.size(0);
  // a factor of the rate per segment (the trust ratios of ops.layer_trust): one float for every segment
  a.seg_lr = held_out<float>(*this, t, seg_lr, "seg_lr", at_least(ns));
  TORCH_CHECK(!a.seg_lr || kind == dtfe::OPT_MOMENTUM, "OptState: seg_lr (a per-segment rate) is for the momentum "
              "optimizer, not kind ", kind);
  TORCH_CHECK(nw <= INT32_MAX, "OptState: work has too many items");
  Tensor D;
  if (has(wd)) {
    TORCH_CHECK(wd->device().is_cpu() && wd->scalar_type() == at::kFloat && wd->dim() == 1 && wd->size(0) == ns,
                "OptState: wd is a CPU float32 [nseg] vector");
    D = wd->contiguous();
  }
  segs.resize((size_t)ns);
  work.resize((size_t)nw);
  std::vector<int64_t> len((size_t)ns);  // R * T * C of each segment
  for (int64_t i = 0; i < ns; ++i) {
    const int64_t* s = S.data_ptr<int64_t>() + i * 6;
    const int64_t off = s[0], R = s[1], T = s[2], C = s[3];
    // in this order no product overflows: each factor is at most numel before the next multiplies it
    TORCH_CHECK(off >= 0 && off <= numel && R >= 1 && T >= 1 && C >= 1 && R <= numel && T <= numel / R &&
                    C <= (numel - off) / (R * T) && std::max({R, T, C}) <= INT32_MAX,
                "OptState: segs[", i, "] (off ", off, ", R ", R, ", T ", T, ", C ", C, ") does not lie inside p [", numel, "]");
    const float w = D.defined() ? D.data_ptr<float>()[i] : 0.f;
    TORCH_CHECK(std::isfinite(w) && w >= 0.f, "OptState: wd[", i, "] is finite and >= 0, got ", w);
    len[(size_t)i] = R * T * C;
    auto& g = segs[(size_t)i];
    g.off = off; g.R = (int)R; g.T = (int)T; g.C = (int)C; g.wd = w;
    g.w16 = reinterpret_cast<dtfe::bf16*>(s[4]);
    g.wt16 = reinterpret_cast<dtfe::bf16*>(s[5]);
  }
  for (int64_t i = 0; i < nw; ++i) {
    const int64_t* w = W.data_ptr<int64_t>() + i * 7;
    const int64_t k = w[0], sg = w[1], t = w[2], r0 = w[3], c0 = w[4], start = w[5], count = w[6];
    TORCH_CHECK((k == 0 || k == 1) && sg >= 0 && sg < ns, "OptState: work[", i, "] has kind ", k, " (0 flat, 1 tile) and"
                " segment ", sg, " of ", ns);
    const auto& g = segs[(size_t)sg];
    if (k == 0) {
      TORCH_CHECK(start >= 0 && count >= 0 && start <= len[(size_t)sg] && count <= len[(size_t)sg] - start,
                  "OptState: work[", i, "] flat range (start ", start, ", count ", count, ") runs past segment ", sg,
                  " [", len[(size_t)sg], "]");
    } else {
      TORCH_CHECK(t >= 0 && t < g.T && r0 >= 0 && r0 < g.R && c0 >= 0 && c0 < g.C && g.wt16, "OptState: work[", i,
                  "] tile (t ", t, ", r0 ", r0, ", c0 ", c0, ") needs a segment with a wt16 copy and t < T, r0 < R, c0 < C");
    }
    work[(size_t)i] = dtfe::OptWork{(int)k, (int)sg, (int)t, (int)r0, (int)c0, start, count};
  }
  // the device blob: both struct arrays (optim.h opt_blob_work_offset)
  const size_t bs = ns * sizeof(dtfe::OptSeg), bw = nw * sizeof(dtfe::OptWork), off_w = dtfe::opt_blob_work_offset(ns);
  Tensor host = at::empty({(int64_t)(off_w + bw)}, at::TensorOptions().dtype(at::kByte));
  if (bs) std::memcpy(host.data_ptr(), segs.data(), bs);
  if (bw) std::memcpy((char*)host.data_ptr() + off_w, work.data(), bw);
  held.push_back(host.to(p.device()));
  dtfe::opt_blob_plan(held.back().data_ptr(), (size_t)ns, a);
  a.nwork = (int)nw;
}

namespace {

using OptStateArg = c10::intrusive_ptr<OptStateObj>;

void epoch_signal(const Tensor& ctr) {
  const TensorArgs t("epoch_signal", ctr, "ctr");
  dtfe::launch_epoch_signal(t.out<int32_t>(ctr, "ctr", at_least(1)), t.stream());
}

// sum of squares of (gscale * g) over the plan's chunks -> out[0] = norm, out[1] = clip_norm / max(norm, clip_norm).
// plan: int64 [nchunk, 2] device table of (offset, count <= 8192) (ops.grad_norm_plan); partials: fp32 [>= nchunk];
// ticket: zeroed int32 [1] (the kernel resets it); max_blocks: 0 = default grid (a test forces 1)
void grad_sumsq(const optional<Tensor>& g, const optional<Tensor>& g16, double gscale, double clip_norm,
                const Tensor& plan, const Tensor& partials, const Tensor& ticket, const Tensor& out,
                int64_t max_blocks) {
  const TensorArgs t("grad_sumsq", plan, "plan");
  dtfe::GradNormArgs a{};
  // (the plan's offsets are the caller's: ops.grad_norm_plan builds it from the buffer it is used on)
  a.g = t.in<float>(g, "g", at_least(0));
  a.g16 = t.in<dtfe::bf16>(g16, "g16", at_least(0));
  TORCH_CHECK((a.g != nullptr) != (a.g16 != nullptr), "grad_sumsq: exactly one of g / g16");
  TORCH_CHECK(plan.dim() == 2 && plan.size(1) == 2, "grad_sumsq: plan is a contiguous int64 [nchunk, 2] table");
  static_assert(sizeof(dtfe::GradChunk) == 2 * sizeof(int64_t), "plan rows are GradChunk");
  TORCH_CHECK(clip_norm >= 0 && max_blocks >= 0, "grad_sumsq: clip_norm and max_blocks are >= 0");
  a.gscale = (float)gscale; a.clip_norm = (float)clip_norm;
  a.plan = reinterpret_cast<const dtfe::GradChunk*>(t.in<int64_t>(plan, "plan", exactly(plan.numel())));
  a.nchunk = (int)plan.size(0);
  a.partials = t.out<float>(partials, "partials (one per chunk)", at_least(plan.size(0)));
  a.ticket = reinterpret_cast<uint32_t*>(t.out<int32_t>(ticket, "ticket", at_least(1)));
  a.out = t.out<float>(out, "out", at_least(2));
  a.max_blocks = (int)max_blocks;
  dtfe::launch_grad_sumsq(a, t.stream());
}

// LARS: the norms of master and gradient of every adaptive variable and from them its trust ratio (kernels/lars.h).
// plan: int64 [nchunk, 3] device table of (seg, offset, count <= 8192); segs: int32 [nadapt, 3] device table of
// (seg, first chunk, chunks) - both from ops.layer_trust_plan, which checks them against the buffers; limit: the
// largest offset + count of the plan; wd: float32 [nseg]; partials: fp32 [>= 2 nchunk]; ticket: zeroed int32 [1]
// (the kernel resets it); sums: fp32 [nseg, 2]; trust: fp32 [nseg]; max_blocks: 0 = default grid (a test forces 1)
void layer_trust(const Tensor& p, const optional<Tensor>& g, const optional<Tensor>& g16, double gscale,
                 const Tensor& plan, const Tensor& segs, int64_t limit, const Tensor& wd, double eeta, double eps,
                 const optional<Tensor>& clip_scale, const Tensor& partials, const Tensor& ticket, const Tensor& sums,
                 const Tensor& trust, int64_t max_blocks) {
  const TensorArgs t("layer_trust", p, "p");
  TORCH_CHECK(limit >= 0, "layer_trust: limit is >= 0");
  dtfe::LarsArgs a{};
  a.p = t.in<float>(p, "p", at_least(limit));
  a.g = t.in<float>(g, "g", at_least(limit));
  a.g16 = t.in<dtfe::bf16>(g16, "g16", at_least(limit));
  TORCH_CHECK((a.g != nullptr) != (a.g16 != nullptr), "layer_trust: exactly one of g / g16");
  static_assert(sizeof(dtfe::LarsChunk) == 3 * sizeof(int64_t), "plan rows are LarsChunk");
  static_assert(sizeof(dtfe::LarsSeg) == 3 * sizeof(int32_t), "segs rows are LarsSeg");
  TORCH_CHECK(plan.dim() == 2 && plan.size(1) == 3 && plan.size(0) <= INT32_MAX,
              "layer_trust: plan is a contiguous int64 [nchunk, 3] table");
  TORCH_CHECK(segs.dim() == 2 && segs.size(1) == 3, "layer_trust: segs is a contiguous int32 [nadapt, 3] table");
  const int64_t nseg = wd.numel();
  TORCH_CHECK(segs.size(0) <= nseg, "layer_trust: wd is contiguous float32 [nseg], nseg at least the adaptive segments");
  TORCH_CHECK(std::isfinite(eeta) && eeta > 0 && std::isfinite(eps) && eps >= 0 && max_blocks >= 0,
              "layer_trust: eeta > 0, eps >= 0, max_blocks >= 0");
  a.gscale = (float)gscale;
  a.plan = reinterpret_cast<const dtfe::LarsChunk*>(t.in<int64_t>(plan, "plan", exactly(plan.numel())));
  a.nchunk = (int)plan.size(0);
  a.segs = reinterpret_cast<const dtfe::LarsSeg*>(t.in<int32_t>(segs, "segs", exactly(segs.numel())));
  a.nadapt = (int)segs.size(0);
  a.wd = t.in<float>(wd, "wd", exactly(nseg));
  a.eeta = (float)eeta; a.eps = (float)eps;
  a.clip_scale = t.in<float>(clip_scale, "clip_scale", at_least(1));
  a.partials = t.out<float>(partials, "partials (two per chunk)", at_least(2 * plan.size(0)));
  a.ticket = reinterpret_cast<uint32_t*>(t.out<int32_t>(ticket, "ticket", at_least(1)));
  a.sums = t.out<float>(sums, "sums", exactly(2 * nseg));
  a.trust = t.out<float>(trust, "trust", exactly(nseg));
  a.max_blocks = (int)max_blocks;
  dtfe::launch_layer_trust(a, t.stream());
}

// t[i] *= scale[0] over the plan's chunks (same table as grad_sumsq's)
void scale_(const Tensor& x, const Tensor& scale, const Tensor& plan) {
  const TensorArgs t("scale_", x, "t");
  TORCH_CHECK(plan.dim() == 2 && plan.size(1) == 2, "scale_: plan is a contiguous int64 [nchunk, 2] table");
  dtfe::launch_scale_ranges(t.out<float>(x, "t", at_least(0)), t.in<float>(scale, "scale", at_least(1)),
                            reinterpret_cast<const dtfe::GradChunk*>(t.in<int64_t>(plan, "plan", exactly(plan.numel()))),
                            (int)plan.size(0), t.stream());
}

// one chunk of an on-device evaluation pass (kernels/eval.h)
void eval_metrics(const Tensor& logits, const Tensor& labels, int64_t k, const Tensor& state,
                  const optional<Tensor>& idx, const Tensor& ws, const Tensor& ticket) {
  const TensorArgs t("eval_metrics", logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.size(1) >= 1 && logits.numel() < (int64_t(1) << 31),
              "eval_metrics: logits are contiguous float32 [B][NC]");
  const int64_t B = logits.size(0), NC = logits.size(1);
  TORCH_CHECK(k >= 1 && k <= NC, "eval_metrics: 1 <= k <= NC, got k = ", k, " for ", NC, " classes");
  static_assert(sizeof(dtfe::EvalState) == dtfe::EVAL_STATE_WORDS * sizeof(int64_t), "the state is 64-bit words");
  dtfe::EvalMetricsArgs a{};
  a.logits = t.in<float>(logits, "logits", exactly(B * NC));
  a.labels = t.in<int32_t>(labels, "labels", exactly(B));
  a.idx = t.out<int32_t>(idx, "idx", at_least(B));
  a.B = (int)B; a.NC = (int)NC; a.k = (int)k;
  a.state = reinterpret_cast<dtfe::EvalState*>(t.out<int64_t>(state, "state", at_least(dtfe::EVAL_STATE_WORDS)));
  a.ws = reinterpret_cast<uint32_t*>(t.out<int32_t>(ws, "ws (2 * B words)", at_least(2 * B)));
  a.ticket = reinterpret_cast<uint32_t*>(t.out<int32_t>(ticket, "ticket", at_least(1)));
  dtfe::launch_eval_metrics(a, t.stream());
}

// the device copy of an LrSchedule (optim.h).  kind: 0 constant, 1 piecewise, 2 linear.  The floats arrive
// as the float32 values the host mirror (ops.lr_schedule_value) computes with, so the casts are exact
Tensor lr_schedule_pack(int64_t kind, at::IntArrayRef bounds, at::ArrayRef<double> values, double lr, double end,
                        int64_t decay_steps, double inv_decay, int64_t warmup, double inv_warmup,
                        const Tensor& device_like) {
  TORCH_CHECK(kind >= dtfe::LR_CONSTANT && kind <= dtfe::LR_LINEAR, "lr_schedule_pack: kind is 0, 1 or 2");
  dtfe::LrSchedule h{};
  h.kind = (int)kind;
  if (kind == dtfe::LR_PIECEWISE) {
    TORCH_CHECK(bounds.size() >= 1 && bounds.size() <= (size_t)dtfe::LR_MAX_BOUNDS && values.size() == bounds.size() + 1,
                "lr_schedule_pack: 1..8 boundaries and one more value than boundaries");
    h.nb = (int)bounds.size();
    for (size_t i = 0; i < bounds.size(); ++i) {
      TORCH_CHECK(bounds[i] >= 0 && bounds[i] <= INT32_MAX && (i == 0 || bounds[i] > bounds[i - 1]),
                  "lr_schedule_pack: boundaries are strictly increasing int32 steps");
      h.bounds[i] = (int)bounds[i];
    }
    for (size_t i = 0; i < values.size(); ++i) h.values[i] = (float)values[i];
  }
  if (kind == dtfe::LR_LINEAR)
    TORCH_CHECK(decay_steps >= 1 && decay_steps <= INT32_MAX, "lr_schedule_pack: decay_steps >= 1");
  TORCH_CHECK(warmup >= 0 && warmup <= INT32_MAX, "lr_schedule_pack: warmup >= 0");
  h.lr = (float)lr; h.end = (float)end;
  h.decay_steps = (int)decay_steps; h.inv_decay = (float)inv_decay;
  h.warmup = (int)warmup; h.inv_warmup = (float)inv_warmup;
  Tensor host = at::empty({(int64_t)sizeof(h)}, at::TensorOptions().dtype(at::kByte));
  std::memcpy(host.data_ptr(), &h, sizeof(h));
  return host.to(device_like.device());
}

// one launch of a bound optimizer: its template plus what varies, the gradient checked against it.
// t: anchored on the optimizer's p (held[0]), so g / g16 / clip_scale must be on the optimizer's GPU
dtfe::OptArgs opt_launch_args(const TensorArgs& t, const OptStateObj& o, const optional<Tensor>& g,
                              const optional<Tensor>& g16, double gscale, double lr, int64_t gs_inc,
                              const optional<Tensor>& clip_scale) {
  TORCH_CHECK(has(g) != has(g16), "apply_gradients: exactly one of g / g16");
  TORCH_CHECK(o.dev == t.device().index(), "apply_gradients: every optimizer of a group on one GPU");
  dtfe::OptArgs a = o.args;
  a.g = t.in<float>(g, "g", at_least(o.numel));  // at least p's elements
  a.g16 = t.in<dtfe::bf16>(g16, "g16", at_least(o.numel));
  a.gscale = (float)gscale;
  a.lr = (float)lr;
  a.gs_inc = (int)gs_inc;
  // the device scalar of a global-norm clip (grad_sumsq's out[1:]) multiplied into gscale; null when not given
  a.clip_scale = t.in<float>(clip_scale, "clip_scale", at_least(1));
  return a;
}

// wait_done / wait_seen / wait_segs: this launch's items of the segments in the bit mask wait on the
// device-side counter pair (OptArgs::wait_done / wait_seen) - a gradient produced on another stream with
// no graph edge to the optimizer launch (the CNN's conv2 weight-gradient branch)
void apply_gradients(const OptStateArg& o, const optional<Tensor>& g, const optional<Tensor>& g16, double gscale,
                     double lr, int64_t gs_inc, const optional<Tensor>& wait_done, const optional<Tensor>& wait_seen,
                     int64_t wait_segs, const optional<Tensor>& clip_scale) {
  const TensorArgs t("apply_gradients", o->held.front(), "p");
  dtfe::OptArgs a = opt_launch_args(t, *o, g, g16, gscale, lr, gs_inc, clip_scale);
  const bool waits = has(wait_done);
  TORCH_CHECK(waits == has(wait_seen) && (waits || wait_segs == 0),
              "apply_gradients: wait_done, wait_seen and wait_segs go together");
  if (waits) {
    TORCH_CHECK(wait_segs >= 0 && wait_segs >> 32 == 0, "apply_gradients: int32 wait counters and a 32-bit segment mask");
    a.wait_done = t.out<int32_t>(wait_done, "wait_done", at_least(1));
    a.wait_seen = t.out<int32_t>(wait_seen, "wait_seen", at_least(1));
    a.wait_segs = (uint32_t)wait_segs;
  }
  dtfe::launch_apply_gradients(a, t.stream());
}

// 2..OPT_GROUP_MAX optimizers of one kind over disjoint var lists of one parameter buffer (e.g. the GAN's
// two Adams) in ONE grouped launch, each with its own rate, step increment and clip scale
void apply_gradients_group(const c10::List<OptStateArg>& o, const optional<Tensor>& g, const optional<Tensor>& g16,
                           double gscale, at::ArrayRef<double> lr, at::IntArrayRef gs_inc,
                           const optional<c10::List<optional<Tensor>>>& clip_scale) {
  const size_t n = o.size();
  TORCH_CHECK(n >= 1 && n <= (size_t)dtfe::OPT_GROUP_MAX, "apply_gradients_group: 1..4 optimizers");
  TORCH_CHECK(lr.size() == n && gs_inc.size() == n && (!clip_scale.has_value() || clip_scale->size() == n),
              "apply_gradients_group: one entry per optimizer in every list");
  const OptStateArg first = o.get(0);
  const TensorArgs t("apply_gradients_group", first->held.front(), "p");
  dtfe::OptArgs q[dtfe::OPT_GROUP_MAX];
  for (size_t i = 0; i < n; ++i) {
    const OptStateArg oi = o.get(i);
    q[i] = opt_launch_args(t, *oi, g, g16, gscale, lr[i], gs_inc[i],
                           clip_scale.has_value() ? clip_scale->get(i) : optional<Tensor>());
  }
  dtfe::launch_apply_gradients_group(q, (int)n, t.stream());
}

// exchanges the masters of the optimizer's var list with their EMA shadows and rewrites the bf16 copies from
// the new masters (kernels/optim.h launch_ema_swap); every pointer was checked when the state was built
void ema_swap(const OptStateArg& o) {
  TORCH_CHECK(o->args.ema, "ema_swap: the optimizer has no EMA (OptState built without an ema buffer)");
  const TensorArgs t("ema_swap", o->held.front(), "p");
  dtfe::launch_ema_swap(o->args, t.stream());
}

}  // namespace

// "apply" is apply_gradients as a method: from Python a method call costs a third of an op call that has to
// convert the object argument (the eager launch's host cost; Optimizer.step goes this way)
void opt_state_register() {
  static auto cls = torch::class_<OptStateObj>("dtfe", "OptState")
      .def(torch::init<int64_t, Tensor, optional<Tensor>, optional<Tensor>, double, double, double, double, double,
                       optional<Tensor>, optional<Tensor>, Tensor, const Tensor&, const Tensor&, const optional<Tensor>&,
                       optional<Tensor>, optional<Tensor>, bool, bool, optional<Tensor>, double, bool,
                       optional<Tensor>, optional<Tensor>>())
      .def("apply", &apply_gradients)
      .def("ema_swap", &ema_swap);
}

namespace {

// ---------------------------------------------------------- elementwise
void wgrad_tallk(const Tensor& A, int64_t lda, const Tensor& B, int64_t ldb, int64_t M, int64_t N, int64_t K,
                 const Tensor& out, int64_t ldc, const optional<Tensor>& bias, const Tensor& ws, int64_t splits,
                 double scale) {
  const TensorArgs t("wgrad_tallk", out, "out");
  dtfe::TallKArgs a{};
  a.A = t.in<float>(A, "A", spans((K - 1) * lda + M)); a.lda = (int)lda;
  a.B = t.in<float>(B, "B", spans((K - 1) * ldb + N)); a.ldb = (int)ldb;
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.out = t.out<float>(out, "out", spans((M - 1) * ldc + N)); a.ldc = (int)ldc;
  a.bias = t.out<float>(bias, "bias", at_least(N));
  a.ws = t.out<float>(ws, "ws", at_least(dtfe::tallk_ws_floats((int)M, (int)N, (int)splits))); a.splits = (int)splits;
  a.scale = (float)scale;
  dtfe::launch_wgrad_tallk(a, t.stream());
}

dtfe::SeqStageArgs seq_stage_args(const TensorArgs& t, const Tensor& x, const Tensor& xh, int64_t T, int64_t I,
                                   const Tensor& ysrc, const Tensor& ydst, at::TensorList zero) {
  TORCH_CHECK(xh.dim() == 3 && xh.size(0) == T && xh.size(2) > I && T >= 1 && I >= 1,
              "seq_stage: x f32 [B][T*I], xh f32 [T][B][ld > I] contiguous");
  const int64_t B = xh.size(1);
  TORCH_CHECK(B >= 1 && ysrc.numel() % B == 0, "seq_stage: label rows f32 [B][*], same size, contiguous");
  dtfe::SeqStageArgs a{};
  a.x = t.in<float>(x, "x", exactly(B * T * I));
  a.xh = t.out<float>(xh, "xh", exactly(xh.numel()));
  a.B = (int)B; a.T = (int)T; a.I = (int)I; a.ld = (int)xh.size(2);
  a.ysrc = t.in<float>(ysrc, "ysrc", exactly(ysrc.numel()));
  a.ydst = t.out<float>(ydst, "ydst", exactly(ysrc.numel())); a.ny = ysrc.numel();
  t.zero_ranges(zero, a.zptr, a.zlen, a.nz);
  return a;
}

void seq_stage(const Tensor& x, const Tensor& xh, int64_t T, int64_t I, const Tensor& ysrc, const Tensor& ydst,
               at::TensorList zero) {
  const TensorArgs t("seq_stage", xh, "xh");
  dtfe::launch_seq_stage(seq_stage_args(t, x, xh, T, I, ysrc, ydst, zero), t.stream());
}

void gather_rows(const Tensor& src, const Tensor& dst, const optional<Tensor>& idx, const optional<Tensor>& labels_src,
                 const optional<Tensor>& labels_dst, int64_t seed, const optional<Tensor>& counter,
                 const optional<Tensor>& done, at::TensorList zero, const optional<Tensor>& onehot, bool shuffle) {
  const TensorArgs t("gather_rows", src, "src");
  TORCH_CHECK(src.dim() >= 1 && src.size(0) >= 1 && dst.dim() >= 1, "gather_rows: src [n_rows][...], dst [B][...]");
  TORCH_CHECK(!shuffle || !has(idx), "gather_rows: shuffle samples the rows itself, it takes no idx");
  TORCH_CHECK(!shuffle || src.size(0) <= (int64_t(1) << 31), "gather_rows: shuffle needs 1 <= n_rows <= 2^31");
  dtfe::GatherArgs a{};
  a.sample = shuffle ? dtfe::SAMPLE_SHUFFLE : dtfe::SAMPLE_REPLACE;
  const int64_t B = dst.size(0), D = src.numel() / src.size(0);
  if (has(onehot)) {
    TORCH_CHECK(onehot->dim() == 2 && onehot->size(0) == B && has(labels_src),
                "gather_rows: onehot must be contiguous f32 [B][ncls] and needs labels_src");
    a.onehot = t.out<float>(onehot, "onehot", exactly(onehot->numel()));
    a.ncls = (int)onehot->size(1);
  }
  t.zero_ranges(zero, a.zptr, a.zlen, a.nz);
  const dtfe::AnyPtr ps = t.any(src, "src", dtfe::ANY_DATA, exactly(src.numel()));
  const dtfe::AnyPtr pd = t.any(dst, "dst", dtfe::F32_OR_BF16, exactly(B * D));  // f32 or bf16 rows of src's length
  a.src = ps.p; a.src_dtype = ps.code; a.n_rows = src.size(0); a.D = (int)D;
  a.dst = pd.p; a.dst_dtype = pd.code; a.B = (int)B;
  a.idx = t.in<int32_t>(idx, "idx", at_least(B));
  a.labels_src = t.in<int32_t>(labels_src, "labels_src", at_least(a.n_rows));
  a.labels_dst = t.out<int32_t>(labels_dst, "labels_dst", at_least(B));
  a.seed = (uint64_t)seed; a.counter = t.out<int64_t>(counter, "counter", at_least(1));
  a.done = t.out<uint32_t>(done, "done", at_least(1));
  dtfe::launch_gather_rows(a, t.stream());
}

// gather_rows for image rows with the input transforms in the same launch (kernels/augment.h)
void augment_rows(const Tensor& src, const Tensor& dst, int64_t H, int64_t W, int64_t C, int64_t pad, bool flip,
                  const optional<Tensor>& mean, const optional<Tensor>& inv_std, const optional<Tensor>& idx,
                  const optional<Tensor>& labels_src, const optional<Tensor>& labels_dst, int64_t seed,
                  const optional<Tensor>& counter, const optional<Tensor>& done, at::TensorList zero,
                  const optional<Tensor>& onehot, bool shuffle, int64_t mix, double label_smoothing) {
  const TensorArgs t("augment_rows", src, "src");
  TORCH_CHECK(mix >= dtfe::MIX_NONE && mix <= dtfe::MIX_CUTMIX, "augment_rows: mix is 0 (none), 1 (mixup) or 2 (cutmix)");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0, "augment_rows: label_smoothing must lie in [0, 1)");
  const bool soft = mix != dtfe::MIX_NONE || label_smoothing > 0.0;
  TORCH_CHECK(!soft || (has(onehot) && has(labels_src)),
              "augment_rows: mix / label_smoothing write soft label rows: they need onehot and labels_src");  TORCH_CHECK(H >= 1 && W >= 1 && C >= 1 && H * W * C < (int64_t(1) << 31), "augment_rows: bad image shape");
  const int64_t D = H * W * C;
  TORCH_CHECK(src.dim() == 2 && src.size(0) >= 1 && src.size(0) < (int64_t(1) << 31) && src.size(1) == D,
              "augment_rows: src must be [n_rows][H*W*C]");
  TORCH_CHECK(dst.dim() >= 1 && dst.size(0) >= 1 && dst.size(0) < (int64_t(1) << 31), "augment_rows: dst must hold [B][H][W][C]");
  TORCH_CHECK(pad >= 0 && pad <= dtfe::AUG_MAX_PAD && pad < std::min(H, W),
              "augment_rows: 0 <= pad <= 15 and pad < min(H, W)");
  TORCH_CHECK(has(mean) == has(inv_std), "augment_rows: mean and inv_std come together");
  const int64_t B = dst.size(0);
  TORCH_CHECK(mix == dtfe::MIX_NONE || B >= 2, "augment_rows: mix needs a batch of B >= 2 (dst)");
  dtfe::AugmentArgs a{};
  const dtfe::AnyPtr ps = t.any(src, "src", dtfe::U8_OR_F32, exactly(src.size(0) * D));
  const dtfe::AnyPtr pd = t.any(dst, "dst", dtfe::F32_OR_BF16, exactly(B * D));
  a.mean = t.in<float>(mean, "mean", exactly(C));
  a.inv_std = t.in<float>(inv_std, "inv_std", exactly(C));
  a.idx = t.in<int32_t>(idx, "idx", at_least(B));
  TORCH_CHECK(!shuffle || !a.idx, "augment_rows: shuffle samples the rows itself, it takes no idx");
  a.sample = shuffle ? dtfe::SAMPLE_SHUFFLE : dtfe::SAMPLE_REPLACE;
  a.labels_src = t.in<int32_t>(labels_src, "labels_src", at_least(src.size(0)));
  a.labels_dst = t.out<int32_t>(labels_dst, "labels_dst", at_least(B));
  TORCH_CHECK(!a.labels_dst || a.labels_src, "augment_rows: labels_dst needs labels_src");
  if (has(onehot)) {
    TORCH_CHECK(onehot->dim() == 2 && onehot->size(0) == B && a.labels_src,
                "augment_rows: onehot must be contiguous f32 [B][ncls] and needs labels_src");
    a.onehot = t.out<float>(onehot, "onehot", exactly(onehot->numel()));
    a.ncls = (int)onehot->size(1);
  }
  a.counter = t.out<int64_t>(counter, "counter", at_least(1));
  a.done = t.out<uint32_t>(done, "done", at_least(1));
  t.zero_ranges(zero, a.zptr, a.zlen, a.nz);
  a.src = ps.p; a.src_dtype = ps.code; a.n_rows = src.size(0);
  a.dst = pd.p; a.dst_dtype = pd.code; a.B = (int)B;
  a.H = (int)H; a.W = (int)W; a.C = (int)C; a.pad = (int)pad; a.flip = flip ? 1 : 0;
  a.seed = (uint64_t)seed;
  a.mix = (int)mix;
  if (label_smoothing > 0.0) {  // float32 throughout, as ops.smoothing_values: off = E / ncls, on = (1 - E) + off
    const float e = (float)label_smoothing;
    a.smooth_off = e / (float)a.ncls;
    a.smooth_on = (1.f - e) + a.smooth_off;
  }
  a.inv_hw = 1.f / (float)(H * W);
  dtfe::launch_augment_rows(a, t.stream());
}

void uniform_fill(const Tensor& out, double lo, double hi, int64_t seed, const optional<Tensor>& counter,
                  const optional<Tensor>& done, const optional<Tensor>& copy_src, const optional<Tensor>& copy_dst) {
  const TensorArgs t("uniform_fill", out, "out");
  const float* cs = nullptr;
  float* cd = nullptr;
  long nc = 0;
  if (has(copy_src)) {
    TORCH_CHECK(has(copy_dst), "uniform_fill: copy_src without copy_dst");
    nc = copy_src->numel();
    cs = t.in<float>(copy_src, "copy_src", exactly(nc));
    cd = t.out<float>(copy_dst, "copy_dst", exactly(nc));
    TORCH_CHECK(nc % 4 == 0 && ((uintptr_t)cs & 15) == 0 && ((uintptr_t)cd & 15) == 0,
                "uniform_fill: the fused copy takes equal-size contiguous 16-B aligned fp32 tensors (numel % 4 == 0)");
  }
  dtfe::launch_uniform_fill(t.out<float>(out, "out", exactly(out.numel())), out.numel(), (float)lo, (float)hi,
                            (uint64_t)seed, t.out<int64_t>(counter, "counter", at_least(1)),
                            t.out<uint32_t>(done, "done", at_least(1)), t.stream(), cs, cd, nc);
}

void cast_(const Tensor& src, const Tensor& dst) {
  const TensorArgs t("cast_", src, "src");
  const int64_t n = src.numel();
  const dtfe::AnyPtr ps = t.any(src, "src", dtfe::F32_OR_BF16, exactly(n));
  if (ps.f32())
    dtfe::launch_cast_f32_bf16(static_cast<const float*>(ps.p), t.out<dtfe::bf16>(dst, "dst (f32<->bf16 only)", exactly(n)), n,
                               t.stream());
  else
    dtfe::launch_cast_bf16_f32(static_cast<const dtfe::bf16*>(ps.p), t.out<float>(dst, "dst (f32<->bf16 only)", exactly(n)), n,
                               t.stream());
}

void softmax_xent(const Tensor& logits, const optional<Tensor>& labels_i, const optional<Tensor>& labels_oh,
                  double scale, const optional<Tensor>& dlogits, const optional<Tensor>& loss_rows,
                  const optional<Tensor>& loss_sum, const optional<Tensor>& correct, const optional<Tensor>& probs) {
  const TensorArgs t("softmax_xent", logits, "logits");
  TORCH_CHECK(logits.dim() == 2, "softmax_xent: fp32 logits [B][NC]");
  dtfe::XentArgs a{};
  a.B = (int)logits.size(0); a.NC = (int)logits.size(1);
  const int64_t n = logits.numel();
  a.logits = t.in<float>(logits, "logits", exactly(n));
  a.labels_i = t.in<int32_t>(labels_i, "labels_i", at_least(a.B));
  a.labels_oh = t.in<float>(labels_oh, "labels_oh", at_least(n));
  TORCH_CHECK(a.labels_i || a.labels_oh, "softmax_xent: labels required");
  a.scale = (float)scale;
  a.dlogits = t.out<float>(dlogits, "dlogits", at_least(n)); a.loss_rows = t.out<float>(loss_rows, "loss_rows", at_least(a.B));
  a.loss_sum = t.out<float>(loss_sum, "loss_sum", at_least(1)); a.correct = t.out<int32_t>(correct, "correct", at_least(1));
  a.probs = t.out<float>(probs, "probs", at_least(n));
  dtfe::launch_softmax_xent(a, t.stream());
}

bool dense_head(const Tensor& feat, const Tensor& w, const optional<Tensor>& bias, const Tensor& y,
                const optional<Tensor>& logits, const optional<Tensor>& loss_sum, const optional<Tensor>& correct,
                const Tensor& dw, const optional<Tensor>& db, const optional<Tensor>& dfeat, double scale,
                bool w_fmajor, bool store, const optional<Tensor>& dl_out) {
  const TensorArgs t("dense_head", feat, "feat");
  TORCH_CHECK(feat.dim() == 2 && w.dim() == 2, "dense_head: bf16 / fp32 feat [B][F], fp32 w [NC][F] / [F][NC]");
  const int64_t B = feat.size(0), F = feat.size(1), NC = w_fmajor ? w.size(1) : w.size(0);
  dtfe::DenseHeadArgs a{};
  const dtfe::AnyPtr pf = t.any(feat, "feat", dtfe::F32_OR_BF16, exactly(B * F));
  a.feat = pf.p;
  a.f32 = pf.f32() ? 1 : 0;
  a.w_fmajor = w_fmajor ? 1 : 0;
  a.store = store ? 1 : 0;
  a.w = t.in<float>(w, "w", exactly(NC * F)); a.bias = t.in<float>(bias, "bias", at_least(NC));
  a.y = t.in<float>(y, "y (one-hot)", exactly(B * NC));
  a.logits = t.out<float>(logits, "logits", exactly(B * NC)); a.loss_sum = t.out<float>(loss_sum, "loss_sum", at_least(1));
  a.correct = t.out<int32_t>(correct, "correct", at_least(1));
  a.dw = t.out<float>(dw, "dw", exactly(NC * F)); a.db = t.out<float>(db, "db", at_least(NC));
  // dfeat: feat's dtype and shape
  a.dfeat = pf.f32() ? (void*)t.out<float>(dfeat, "dfeat", exactly(B * F)) : (void*)t.out<dtfe::bf16>(dfeat, "dfeat", exactly(B * F));
  a.dl_out = t.out<float>(dl_out, "dl_out", exactly(B * NC));
  a.B = (int)B; a.F = (int)F; a.NC = (int)NC; a.scale = (float)scale;
  return dtfe::launch_dense_head(a, t.stream());
}

void gan_loss(const Tensor& d_real, const Tensor& d_fake, const Tensor& gen_loss, const Tensor& disc_loss,
              const Tensor& dz_real_disc, const Tensor& dz_fake_disc, const Tensor& dz_fake_gen, double clamp_eps) {
  const TensorArgs t("gan_loss", d_real, "d_real");
  const int64_t B = d_real.numel();
  dtfe::GanLossArgs a{};
  a.B = (int)B;
  a.d_real = t.in<float>(d_real, "d_real", exactly(B)); a.d_fake = t.in<float>(d_fake, "d_fake", at_least(B));
  a.gen_loss = t.out<float>(gen_loss, "gen_loss", at_least(1)); a.disc_loss = t.out<float>(disc_loss, "disc_loss", at_least(1));
  a.dz_real_disc = t.out<float>(dz_real_disc, "dz_real_disc", at_least(B));
  a.dz_fake_disc = t.out<float>(dz_fake_disc, "dz_fake_disc", at_least(B));
  a.dz_fake_gen = t.out<float>(dz_fake_gen, "dz_fake_gen", at_least(B));
  a.clamp_eps = (float)clamp_eps;
  dtfe::launch_gan_loss(a, t.stream());
}

bool gan_disc_head(const Tensor& d1, const Tensor& w, const optional<Tensor>& b, const optional<Tensor>& p,
                   const optional<Tensor>& dlog, const optional<Tensor>& dlog_g, const Tensor& gw,
                   const optional<Tensor>& gb, const Tensor& dd1, const Tensor& ddf, const Tensor& gen_loss,
                   const Tensor& disc_loss, const Tensor& ws, double clamp_eps) {
  const TensorArgs t("gan_disc_head", d1, "d1");
  TORCH_CHECK(d1.dim() == 2 && d1.size(0) % 2 == 0, "gan_disc_head: d1 f32 [2B][DH] contiguous");
  const int64_t B = d1.size(0) / 2, DH = d1.size(1);
  dtfe::GanHeadArgs a{};
  a.B = (int)B; a.DH = (int)DH;
  a.d1 = t.in<float>(d1, "d1", exactly(2 * B * DH)); a.w = t.in<float>(w, "w (Wd2 [DH])", exactly(DH));
  a.b = t.in<float>(b, "b", at_least(1));
  a.p = t.out<float>(p, "p", exactly(2 * B));
  a.dlog = t.out<float>(dlog, "dlog", exactly(2 * B));
  a.dlog_g = t.out<float>(dlog_g, "dlog_g", exactly(B));
  a.gw = t.out<float>(gw, "gw (dWd2 [DH])", exactly(DH)); a.gb = t.out<float>(gb, "gb", at_least(1));
  a.dd1 = t.out<float>(dd1, "dd1", exactly(2 * B * DH)); a.ddf = t.out<float>(ddf, "ddf", exactly(B * DH));
  a.gen_loss = t.out<float>(gen_loss, "gen_loss", exactly(1)); a.disc_loss = t.out<float>(disc_loss, "disc_loss", exactly(1));
  a.clamp_eps = (float)clamp_eps;
  a.ws = t.out<float>(ws, "ws (zeroed, ops.gan_head_ws_floats)", at_least(dtfe::gan_head_ws_floats((int)B, (int)DH)));
  return dtfe::launch_gan_disc_head(a, t.stream());
}

int64_t gan_head_ws_floats(int64_t B, int64_t DH) { return dtfe::gan_head_ws_floats((int)B, (int)DH); }

void mse_sigmoid(const Tensor& y, const Tensor& target, const Tensor& loss, const Tensor& dz, const optional<Tensor>& ws) {
  const TensorArgs t("mse_sigmoid", y, "y");
  const int64_t n = y.numel();
  // ws: zero-initialised
  dtfe::launch_mse_sigmoid(t.in<float>(y, "y", exactly(n)), t.in<float>(target, "t", exactly(n)), n,
                           t.out<float>(loss, "loss", at_least(1)), t.out<float>(dz, "dz", exactly(n)), t.stream(),
                           t.out<float>(ws, "ws", at_least(dtfe::MSE_WS_FLOATS)));
}

void colsum(const Tensor& x, int64_t M, int64_t N, int64_t ld, const Tensor& db, double scale) {
  const TensorArgs t("colsum", x, "x");
  const dtfe::AnyPtr px = t.any(x, "x", dtfe::F32_OR_BF16, spans((M - 1) * ld + N));
  dtfe::launch_colsum(px.p, px.f32(), (int)M, (int)N, ld, t.out<float>(db, "db", at_least(N)), (float)scale, t.stream());
}

void act_grad(const Tensor& dy, const Tensor& y, const Tensor& dz, int64_t act) {
  const TensorArgs t("act_grad", dy, "dy");
  const int64_t n = dy.numel();
  dtfe::launch_act_grad(t.in<float>(dy, "dy", exactly(n)), t.in<float>(y, "y", at_least(n)), t.out<float>(dz, "dz", at_least(n)),
                        n, (int)act, t.stream());
}

void bias_act(const Tensor& x, const optional<Tensor>& bias, const Tensor& out, int64_t act, double keep,
              int64_t seed, const optional<Tensor>& counter) {
  const TensorArgs t("bias_act", x, "x");
  TORCH_CHECK(x.dim() >= 1 && x.size(0) >= 1, "bias_act: x [M][N]");
  dtfe::BiasActArgs a{};
  a.M = (int)x.size(0); a.N = (int)(x.numel() / x.size(0)); a.act = (int)act;
  a.x = t.in<float>(x, "x", exactly(x.numel())); a.bias = t.in<float>(bias, "bias", at_least(a.N));
  a.keep = (float)keep; a.seed = (uint64_t)seed; a.counter = t.in<int64_t>(counter, "counter", at_least(1));
  const dtfe::AnyPtr po = t.any(out, "out", dtfe::F32_OR_BF16, at_least(x.numel()));
  a.out = po.p; a.out_f32 = po.f32();
  dtfe::launch_bias_act(a, t.stream());
}

void lstm_cell_fwd(const Tensor& gates, const Tensor& act, const optional<Tensor>& c_prev, const Tensor& c,
                   const Tensor& h_out, int64_t ld_h, double forget_bias) {
  const TensorArgs t("lstm_cell_fwd", gates, "gates");
  TORCH_CHECK(c.dim() == 2, "lstm_cell_fwd: c [B][H]");
  dtfe::LstmCellArgs a{};
  const int64_t B = c.size(0), H = c.size(1);
  a.B = (int)B; a.H = (int)H;
  a.gates = t.in<float>(gates, "gates", at_least(4 * B * H)); a.act = t.out<float>(act, "act", at_least(4 * B * H));
  a.c_prev = t.in<float>(c_prev, "c_prev", at_least(B * H));
  a.c = t.out<float>(c, "c", exactly(B * H));
  a.h_out = t.out<float>(h_out, "h_out", spans((B - 1) * ld_h + H)); a.ld_h = ld_h;
  a.forget_bias = (float)forget_bias;
  dtfe::launch_lstm_cell_fwd(a, t.stream());
}

void lstm_cell_bwd(const Tensor& act, const optional<Tensor>& c_prev, const Tensor& c, const optional<Tensor>& dh,
                   const optional<Tensor>& dh2, const optional<Tensor>& dc_next, const Tensor& dgates,
                   const Tensor& dc_prev) {
  const TensorArgs t("lstm_cell_bwd", act, "act");
  TORCH_CHECK(c.dim() == 2, "lstm_cell_bwd: c [B][H]");
  dtfe::LstmCellArgs a{};
  const int64_t B = c.size(0), H = c.size(1), n = B * H;
  a.B = (int)B; a.H = (int)H;
  a.act = const_cast<float*>(t.in<float>(act, "act", at_least(4 * n)));
  a.c_prev = t.in<float>(c_prev, "c_prev", at_least(n)); a.c = const_cast<float*>(t.in<float>(c, "c", exactly(n)));
  a.dh = t.in<float>(dh, "dh", at_least(n)); a.dh2 = t.in<float>(dh2, "dh2", at_least(n));
  a.dc_next = t.in<float>(dc_next, "dc_next", at_least(n));
  a.dgates = t.out<float>(dgates, "dgates", at_least(4 * n)); a.dc_prev = t.out<float>(dc_prev, "dc_prev", at_least(n));
  dtfe::launch_lstm_cell_bwd(a, t.stream());
}

// whole-sequence LSTM (lstm_seq.hip): returns false when the shape needs the per-step path
bool lstm_seq_fwd(const Tensor& xh, const Tensor& K, const Tensor& bias, double forget_bias, const Tensor& act,
                  const Tensor& c, const Tensor& hT, const optional<Tensor>& xsrc, const optional<Tensor>& ysrc,
                  const optional<Tensor>& ydst, const optional<Tensor>& zero0, const optional<Tensor>& zero1) {
  const TensorArgs t("lstm_seq_fwd", xh, "xh");
  TORCH_CHECK(xh.dim() == 3 && hT.dim() == 2 && xh.size(2) > hT.size(1), "lstm_seq_fwd: xh [T][B][I+H] f32, hT [B][H]");
  dtfe::LstmSeqArgs a{};
  a.T = (int)xh.size(0); a.B = (int)xh.size(1); a.H = (int)hT.size(1); a.I = (int)xh.size(2) - a.H;
  const int64_t TB = (int64_t)a.T * a.B;
  a.xh = t.out<float>(xh, "xh", exactly(xh.numel()));
  a.K = t.in<float>(K, "K", exactly((int64_t)(a.I + a.H) * 4 * a.H)); a.bias = t.in<float>(bias, "bias", exactly(4 * a.H));
  a.forget_bias = (float)forget_bias;
  a.act = t.out<float>(act, "act", exactly(TB * 4 * a.H)); a.c = t.out<float>(c, "c", exactly(TB * a.H));
  a.hT = t.out<float>(hT, "hT", exactly((int64_t)a.B * a.H));
  if (has(xsrc)) {  // seq_stage folded into the forward launch
    TORCH_CHECK(has(ysrc) && has(ydst), "lstm_seq_fwd: xsrc needs ysrc / ydst");
    std::vector<Tensor> zero;
    for (const optional<Tensor>* z : {&zero0, &zero1})
      if (has(*z)) zero.push_back(**z);
    a.st = seq_stage_args(t, *xsrc, xh, a.T, a.I, *ysrc, *ydst, zero);
  }
  return dtfe::launch_lstm_seq_fwd(a, t.stream());
}

int64_t lstm_status(bool reset) { return dtfe::lstm_split_status(reset); }

int64_t lstm_last_split() { return dtfe::lstm_last_split(); }

bool lstm_seq_bwd(const Tensor& K, const Tensor& act, const Tensor& c, const Tensor& dhT, const Tensor& dg,
                  int64_t I, const optional<Tensor>& dl, const optional<Tensor>& wo) {
  const TensorArgs t("lstm_seq_bwd", act, "act");
  TORCH_CHECK(c.dim() == 3 && I >= 1, "lstm_seq_bwd: c [T][B][H]");
  dtfe::LstmSeqArgs a{};
  a.T = (int)c.size(0); a.B = (int)c.size(1); a.H = (int)c.size(2); a.I = (int)I;
  const int64_t TB = (int64_t)a.T * a.B;
  a.K = t.in<float>(K, "K", exactly((int64_t)(a.I + a.H) * 4 * a.H));
  a.act = const_cast<float*>(t.in<float>(act, "act", exactly(TB * 4 * a.H)));
  a.c = const_cast<float*>(t.in<float>(c, "c", exactly(TB * a.H)));
  a.dhT = t.in<float>(dhT, "dhT", exactly((int64_t)a.B * a.H)); a.dg = t.out<float>(dg, "dg", exactly(TB * 4 * a.H));
  if (has(dl)) {  // dh_T = dl . W_out^T formed by the kernel (the fused head's dlogits)
    TORCH_CHECK(has(wo) && wo->dim() == 2 && wo->size(0) == a.H && dl->dim() == 2 && dl->size(0) == a.B &&
                    dl->size(1) == wo->size(1), "lstm_seq_bwd: dl [B][NC] with W_out [H][NC]");
    a.dl = t.in<float>(dl, "dl", exactly(dl->numel())); a.wo = t.in<float>(wo, "wo", exactly(wo->numel()));
    a.nc = (int)wo->size(1);
  }
  return dtfe::launch_lstm_seq_bwd(a, t.stream());
}

// ------------------------------------------------------------------- norm
// x: bf16 [..., C] viewed as [R][C]; stats (null: bn_infer has none): f32 [2][C]; every per-channel vector of the op is [>= C]
dtfe::BnArgs bn_common(const TensorArgs& t, const Tensor& x, const Tensor* stats, int64_t act) {
  TORCH_CHECK(x.dim() >= 2 && x.size(-1) >= 1, "bn: bf16 [..., C] input");
  dtfe::BnArgs a{};
  a.C = (int)x.size(-1);
  a.R = x.numel() / a.C;
  a.x = t.in<dtfe::bf16>(x, "x", exactly(x.numel()));
  if (stats) a.stats = t.out<float>(*stats, "stats", exactly(2 * a.C));
  a.act = (int)act;
  return a;
}

// the option-A shortcut of bn_apply / bn_infer: res [B][RH][RW][RC] read at (y * rstride, x * rstride, c < RC)
void bn_residual(const TensorArgs& t, dtfe::BnArgs& a, const optional<Tensor>& res, int64_t rstride, int64_t OH,
                 int64_t OW) {
  if (!has(res)) return;
  TORCH_CHECK(res->dim() == 4 && rstride >= 1 && OH >= 1 && OW >= 1 && res->size(0) * OH * OW == a.R &&
                  (OH - 1) * rstride < res->size(1) && (OW - 1) * rstride < res->size(2),
              "bn: residual NHWC [B][> (OH - 1) * rstride][> (OW - 1) * rstride][RC] for B * OH * OW rows");
  a.res = t.in<dtfe::bf16>(res, "res", exactly(res->numel()));
  a.RH = (int)res->size(1); a.RW = (int)res->size(2); a.RC = (int)res->size(3);
  a.rstride = (int)rstride; a.OH = (int)OH; a.OW = (int)OW;
}

void bn_stats(const Tensor& x, const Tensor& stats) {
  const TensorArgs t("bn_stats", x, "x");
  dtfe::launch_bn_stats(bn_common(t, x, &stats, 0), t.stream());
}

void bn_apply(const Tensor& x, const Tensor& stats, const Tensor& gamma, const Tensor& beta,
              const optional<Tensor>& mean, const optional<Tensor>& invstd, const optional<Tensor>& moving_mean,
              const optional<Tensor>& moving_var, double eps, double momentum, int64_t act,
              const optional<Tensor>& res, int64_t rstride, int64_t OH, int64_t OW, const Tensor& out,
              const optional<Tensor>& mask_out, const optional<std::vector<Tensor>>& res_bn) {
  const TensorArgs t("bn_apply", x, "x");
  dtfe::BnArgs a = bn_common(t, x, &stats, act);
  const auto C = at_least(a.C);
  if (res_bn.has_value() && !res_bn->empty()) {
    // [stats, gamma, beta, mean, invstd, moving_mean, moving_var] of the residual's own BatchNorm
    const auto& r = *res_bn;
    TORCH_CHECK(r.size() == 7 && has(res) && res->sizes() == x.sizes(),
                "bn_apply: res_bn = [stats, gamma, beta, mean, invstd, moving_mean, moving_var] of a same-shape raw residual");
    a.r_stats = t.out<float>(r[0], "res_bn[0] (stats)", at_least(2 * a.C));
    a.r_gamma = t.in<float>(r[1], "res_bn[1] (gamma)", C); a.r_beta = t.in<float>(r[2], "res_bn[2] (beta)", C);
    a.r_mean = t.out<float>(r[3], "res_bn[3] (mean)", C); a.r_invstd = t.out<float>(r[4], "res_bn[4] (invstd)", C);
    a.r_moving_mean = t.out<float>(r[5], "res_bn[5] (moving_mean)", C);
    a.r_moving_var = t.out<float>(r[6], "res_bn[6] (moving_var)", C);
  }
  if (has(mask_out)) {
    TORCH_CHECK(act == 1, "bn_apply: mask_out is a uint8 [R][C/8] ReLU bit mask");
    a.mask_out = t.out<uint8_t>(mask_out, "mask_out", exactly(x.numel() / 8));
  }
  a.gamma = t.in<float>(gamma, "gamma", C);
  a.beta = t.in<float>(beta, "beta", C);
  a.mean = t.out<float>(mean, "mean", C);
  a.invstd = t.out<float>(invstd, "invstd", C);
  a.moving_mean = t.out<float>(moving_mean, "moving_mean", C);
  a.moving_var = t.out<float>(moving_var, "moving_var", C);
  a.eps = (float)eps; a.momentum = (float)momentum;
  bn_residual(t, a, res, rstride, OH, OW);
  a.out = t.out<dtfe::bf16>(out, "out", exactly(x.numel()));
  dtfe::launch_bn_apply(a, t.stream());
}

// inference-mode BatchNorm: out = act(gamma * (x - moving_mean) * rsqrt(moving_var + eps) + beta [+ res])
void bn_infer(const Tensor& x, const Tensor& gamma, const Tensor& beta, const Tensor& moving_mean,
              const Tensor& moving_var, double eps, int64_t act, const optional<Tensor>& res, int64_t rstride,
              int64_t OH, int64_t OW, const Tensor& out) {
  const TensorArgs t("bn_infer", x, "x");
  dtfe::BnArgs a = bn_common(t, x, nullptr, act);
  a.infer = 1;
  a.gamma = t.in<float>(gamma, "gamma", at_least(a.C));
  a.beta = t.in<float>(beta, "beta", at_least(a.C));
  a.moving_mean = const_cast<float*>(t.in<float>(moving_mean, "moving_mean", exactly(a.C)));
  a.moving_var = const_cast<float*>(t.in<float>(moving_var, "moving_var", exactly(a.C)));
  a.eps = (float)eps;
  bn_residual(t, a, res, rstride, OH, OW);
  a.out = t.out<dtfe::bf16>(out, "out", exactly(x.numel()));
  dtfe::launch_bn_apply(a, t.stream());
}

// the backward's upstream gradient and ReLU-mask source: the bf16 forward output, or its uint8 [R][C/8] bit mask (ReLU only)
void set_bwd_dy_y(const TensorArgs& t, dtfe::BnArgs& a, const Tensor& dy, const optional<Tensor>& y, const Tensor& x) {
  a.dy = t.in<dtfe::bf16>(dy, "dy", exactly(x.numel()));
  if (has(y) && y->scalar_type() == at::kByte) {
    TORCH_CHECK(a.act == 1, "bn_bwd: bit mask is uint8 [R][C/8], ReLU");
    a.ymask = t.in<uint8_t>(y, "y (bit mask)", exactly(x.numel() / 8));
    return;
  }
  a.y = t.in<dtfe::bf16>(y, "y", exactly(x.numel()));
}

void bn_bwd_stats(const Tensor& dy, const optional<Tensor>& y, const Tensor& x, const Tensor& mean,
                  const Tensor& invstd, const Tensor& stats, int64_t act, const optional<Tensor>& gamma,
                  const optional<Tensor>& beta, const optional<std::vector<Tensor>>& res_bn) {
  const TensorArgs t("bn_bwd_stats", x, "x");
  dtfe::BnArgs a = bn_common(t, x, &stats, act);
  const auto C = at_least(a.C);
  if (res_bn.has_value() && !res_bn->empty()) {
    // [x, mean, invstd, stats] of a projection shortcut's BN: its statistics from the same g
    const auto& r = *res_bn;
    TORCH_CHECK(r.size() == 4 && r[0].sizes() == x.sizes(), "bn_bwd_stats: res_bn = [x bf16 (same shape), mean, invstd, stats [2][C]]");
    a.res = t.in<dtfe::bf16>(r[0], "res_bn[0] (x)", exactly(x.numel()));
    a.r_mean = const_cast<float*>(t.in<float>(r[1], "res_bn[1] (mean)", C));
    a.r_invstd = const_cast<float*>(t.in<float>(r[2], "res_bn[2] (invstd)", C));
    a.r_stats = t.out<float>(r[3], "res_bn[3] (stats)", exactly(2 * a.C));
  }
  set_bwd_dy_y(t, a, dy, y, x);
  a.gamma = t.in<float>(gamma, "gamma", C);
  a.beta = t.in<float>(beta, "beta", C);
  TORCH_CHECK(act == 0 || a.y || a.ymask || (act == 1 && a.gamma && a.beta),
              "bn_bwd: the activation gradient needs the forward output (or, for ReLU, gamma and beta)");
  a.mean = const_cast<float*>(t.in<float>(mean, "mean", C));
  a.invstd = const_cast<float*>(t.in<float>(invstd, "invstd", C));
  dtfe::launch_bn_bwd_stats(a, t.stream());
}

void bn_bwd_apply(const Tensor& dy, const optional<Tensor>& y, const Tensor& x, const Tensor& mean,
                  const Tensor& invstd, const Tensor& gamma, const Tensor& stats, int64_t act, const Tensor& dx,
                  const optional<Tensor>& dres, const optional<Tensor>& dgamma, const optional<Tensor>& dbeta,
                  const optional<Tensor>& beta) {
  const TensorArgs t("bn_bwd_apply", x, "x");
  dtfe::BnArgs a = bn_common(t, x, &stats, act);
  const auto C = at_least(a.C);
  set_bwd_dy_y(t, a, dy, y, x);
  a.beta = t.in<float>(beta, "beta", C);
  TORCH_CHECK(act == 0 || a.y || a.ymask || (act == 1 && a.beta),
              "bn_bwd: the activation gradient needs the forward output (or, for ReLU, beta)");
  a.mean = const_cast<float*>(t.in<float>(mean, "mean", C));
  a.invstd = const_cast<float*>(t.in<float>(invstd, "invstd", C));
  a.gamma = t.in<float>(gamma, "gamma", C);
  a.out = t.out<dtfe::bf16>(dx, "dx", exactly(x.numel()));
  a.dres = t.out<dtfe::bf16>(dres, "dres", exactly(x.numel()));
  a.dgamma = t.out<float>(dgamma, "dgamma", C);
  a.dbeta = t.out<float>(dbeta, "dbeta", C);
  dtfe::launch_bn_bwd_apply(a, t.stream());
}

void shortcut_grad_add(const Tensor& g, const Tensor& dx, int64_t stride) {
  const TensorArgs t("shortcut_grad_add", g, "g");
  // dx[b, y * stride, x * stride, c] += g[b, y, x, c] for c < XC
  TORCH_CHECK(g.dim() == 4 && dx.dim() == 4 && stride >= 1 && g.size(0) == dx.size(0) && g.numel() > 0 &&
                  (g.size(1) - 1) * stride < dx.size(1) && (g.size(2) - 1) * stride < dx.size(2) && dx.size(3) <= g.size(3),
              "shortcut_grad_add: NHWC tensors g [B][OH][OW][C], dx [B][> (OH - 1) * stride][> (OW - 1) * stride][<= C]");
  dtfe::launch_shortcut_grad_add(t.in<dtfe::bf16>(g, "g", exactly(g.numel())), t.out<dtfe::bf16>(dx, "dx", exactly(dx.numel())),
                                 (int)g.size(0), (int)g.size(1), (int)g.size(2), (int)g.size(3), (int)dx.size(1),
                                 (int)dx.size(2), (int)dx.size(3), (int)stride, t.stream());
}

void gap_fwd(const Tensor& x, const Tensor& y) {
  const TensorArgs t("gap_fwd", x, "x");
  TORCH_CHECK(x.dim() == 4, "gap_fwd: NHWC input");
  dtfe::launch_gap_fwd(t.in<dtfe::bf16>(x, "x", exactly(x.numel())), t.out<dtfe::bf16>(y, "y", exactly(x.size(0) * x.size(3))),
                       (int)x.size(0), (int)(x.size(1) * x.size(2)), (int)x.size(3), t.stream());
}

void gap_bwd(const Tensor& dy, const Tensor& dx) {
  const TensorArgs t("gap_bwd", dx, "dx");
  TORCH_CHECK(dx.dim() == 4, "gap_bwd: NHWC output");
  dtfe::launch_gap_bwd(t.in<dtfe::bf16>(dy, "dy", exactly(dx.size(0) * dx.size(3))), t.out<dtfe::bf16>(dx, "dx", exactly(dx.numel())),
                       (int)dx.size(0), (int)(dx.size(1) * dx.size(2)), (int)dx.size(3), t.stream());
}

// 3x3 / stride 2 / pad 1: x [B][H][W][C], y and am [B][ceil(H/2)][ceil(W/2)][C]
void check_pool3(const char* op, const Tensor& x, const Tensor& y) {
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4 && y.size(0) == x.size(0) && y.size(3) == x.size(3) &&
                  y.size(1) == (x.size(1) + 1) / 2 && y.size(2) == (x.size(2) + 1) / 2,
              op, ": NHWC tensors [B][H][W][C] and [B][ceil(H/2)][ceil(W/2)][C]");
}

void maxpool3_fwd(const Tensor& x, const Tensor& y, const Tensor& am) {
  const TensorArgs t("maxpool3_fwd", x, "x");
  check_pool3("maxpool3_fwd", x, y);
  dtfe::launch_maxpool3_fwd(t.in<dtfe::bf16>(x, "x", exactly(x.numel())), t.out<dtfe::bf16>(y, "y", exactly(y.numel())),
                            t.out<uint8_t>(am, "am", exactly(y.numel())), (int)x.size(0), (int)x.size(1), (int)x.size(2),
                            (int)x.size(3), (int)y.size(1), (int)y.size(2), t.stream());
}

void pool3_bn_bwd(const Tensor& dp, const Tensor& am, const Tensor& x, const Tensor& mean, const Tensor& invstd,
                  const Tensor& gamma, const Tensor& beta, const Tensor& stats, const Tensor& dx,
                  const optional<Tensor>& dgamma, const optional<Tensor>& dbeta) {
  const TensorArgs t("pool3_bn_bwd", x, "x");
  TORCH_CHECK(dp.dim() == 4 && x.dim() == 4 && dp.size(0) == x.size(0) && dp.size(3) == x.size(3),
              "pool3_bn_bwd: dp / am [B][OH][OW][C], x / dx [B][H][W][C]");
  dtfe::BnArgs a = bn_common(t, x, &stats, 1);
  const auto C = at_least(a.C);
  a.dy = t.in<dtfe::bf16>(dp, "dp", exactly(dp.numel()));
  a.mean = const_cast<float*>(t.in<float>(mean, "mean", C));
  a.invstd = const_cast<float*>(t.in<float>(invstd, "invstd", C));
  a.gamma = t.in<float>(gamma, "gamma", C);
  a.beta = t.in<float>(beta, "beta", C);
  a.out = t.out<dtfe::bf16>(dx, "dx", exactly(x.numel()));
  a.dgamma = t.out<float>(dgamma, "dgamma", C);
  a.dbeta = t.out<float>(dbeta, "dbeta", C);
  dtfe::launch_pool3_bn_bwd(a, t.in<uint8_t>(am, "am", exactly(dp.numel())), (int)x.size(0), (int)x.size(1), (int)x.size(2),
                            (int)dp.size(1), (int)dp.size(2), t.stream());
}

void bn_relu_pool3(const Tensor& x, const Tensor& stats, const Tensor& gamma, const Tensor& beta,
                   const optional<Tensor>& mean, const optional<Tensor>& invstd, const optional<Tensor>& moving_mean,
                   const optional<Tensor>& moving_var, double eps, double momentum, const Tensor& y,
                   const Tensor& am) {
  const TensorArgs t("bn_relu_pool3", x, "x");
  check_pool3("bn_relu_pool3", x, y);
  dtfe::BnArgs a = bn_common(t, x, &stats, 1);
  const auto C = at_least(a.C);
  a.gamma = t.in<float>(gamma, "gamma", C);
  a.beta = t.in<float>(beta, "beta", C);
  a.mean = t.out<float>(mean, "mean", C);
  a.invstd = t.out<float>(invstd, "invstd", C);
  a.moving_mean = t.out<float>(moving_mean, "moving_mean", C);
  a.moving_var = t.out<float>(moving_var, "moving_var", C);
  a.eps = (float)eps; a.momentum = (float)momentum;
  dtfe::launch_bn_relu_pool3(a, t.out<dtfe::bf16>(y, "y", exactly(y.numel())), t.out<uint8_t>(am, "am", exactly(y.numel())),
                             (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)y.size(1), (int)y.size(2), t.stream());
}

void maxpool3_bwd(const Tensor& dy, const Tensor& am, const Tensor& dx) {
  const TensorArgs t("maxpool3_bwd", dx, "dx");
  check_pool3("maxpool3_bwd", dx, dy);
  dtfe::launch_maxpool3_bwd(t.in<dtfe::bf16>(dy, "dy", exactly(dy.numel())), t.in<uint8_t>(am, "am", exactly(dy.numel())),
                            t.out<dtfe::bf16>(dx, "dx", exactly(dx.numel())), (int)dx.size(0), (int)dx.size(1),
                            (int)dx.size(2), (int)dx.size(3), (int)dy.size(1), (int)dy.size(2), t.stream());
}

}  // namespace

TORCH_LIBRARY(dtfe, m) {
  m.def("conv1_gather_fwd(Tensor images, Tensor labels_src, int seed, Tensor(a!) counter, Tensor(b!) done,"
        " Tensor(c!) labels_dst, Tensor(d!) x, Tensor w, Tensor? bias, Tensor(e!) y, Tensor(f!) argmax,"
        " Tensor(g!)[] zero) -> ()");
  m.def("conv12_gather_fwd(Tensor images, Tensor labels_src, int seed, Tensor(a!) counter, Tensor(b!) done,"
        " Tensor(c!) labels_dst, Tensor(d!) x, Tensor w, Tensor? bias, Tensor(e!) y, Tensor(f!) argmax,"
        " Tensor(g!)[] zero, Tensor w2, Tensor? bias2, Tensor(h!) p2, Tensor(i!) a2) -> ()");
  m.def("lstm_seq_fwd(Tensor(a!) xh, Tensor K, Tensor bias, float forget_bias, Tensor(b!) act, Tensor(c!) c,"
        " Tensor(d!) hT, Tensor? xsrc=None, Tensor? ysrc=None, Tensor(e!)? ydst=None, Tensor(f!)? zero0=None,"
        " Tensor(g!)? zero1=None) -> bool");
  m.def("lstm_seq_bwd(Tensor K, Tensor act, Tensor c, Tensor dhT, Tensor(a!) dg, int I, Tensor? dl=None,"
        " Tensor? wo=None) -> bool");
  m.def("lstm_status(bool reset=False) -> int", &lstm_status);
  m.def("lstm_last_split() -> int", &lstm_last_split);
  m.def("bn_stats(Tensor x, Tensor(a!) stats) -> ()");
  m.def("bn_infer(Tensor x, Tensor gamma, Tensor beta, Tensor moving_mean, Tensor moving_var, float eps, int act,"
        " Tensor? res, int rstride, int OH, int OW, Tensor(a!) out) -> ()");
  m.def("bn_apply(Tensor x, Tensor stats, Tensor gamma, Tensor beta, Tensor(a!)? mean, Tensor(b!)? invstd,"
        " Tensor(c!)? moving_mean, Tensor(d!)? moving_var, float eps, float momentum, int act, Tensor? res,"
        " int rstride, int OH, int OW, Tensor(e!) out, Tensor(f!)? mask_out=None, Tensor(g!)[]? res_bn=None) -> ()");
  m.def("bn_bwd_stats(Tensor dy, Tensor? y, Tensor x, Tensor mean, Tensor invstd, Tensor(a!) stats, int act,"
        " Tensor? gamma=None, Tensor? beta=None, Tensor(b!)[]? res_bn=None) -> ()");
  m.def("bn_bwd_apply(Tensor dy, Tensor? y, Tensor x, Tensor mean, Tensor invstd, Tensor gamma, Tensor stats,"
        " int act, Tensor(a!) dx, Tensor(b!)? dres, Tensor(c!)? dgamma, Tensor(d!)? dbeta, Tensor? beta=None) -> ()");
  m.def("shortcut_grad_add(Tensor g, Tensor(a!) dx, int stride) -> ()");
  m.def("gap_fwd(Tensor x, Tensor(a!) y) -> ()");
  m.def("gap_bwd(Tensor dy, Tensor(a!) dx) -> ()");
  m.def("maxpool3_fwd(Tensor x, Tensor(a!) y, Tensor(b!) am) -> ()");
  m.def("maxpool3_bwd(Tensor dy, Tensor am, Tensor(a!) dx) -> ()");
  m.def("bn_relu_pool3(Tensor x, Tensor stats, Tensor gamma, Tensor beta, Tensor(a!)? mean, Tensor(b!)? invstd,"
        " Tensor(c!)? moving_mean, Tensor(d!)? moving_var, float eps, float momentum, Tensor(e!) y,"
        " Tensor(f!) am) -> ()");
  m.def("pool3_bn_bwd(Tensor dp, Tensor am, Tensor x, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta,"
        " Tensor(a!) stats, Tensor(b!) dx, Tensor(c!)? dgamma, Tensor(d!)? dbeta) -> ()");
  m.def("lstm_cell_fwd(Tensor gates, Tensor(a!) act, Tensor? c_prev, Tensor(b!) c, Tensor(c!) h_out, int ld_h,"
        " float forget_bias) -> ()");
  m.def("lstm_cell_bwd(Tensor act, Tensor? c_prev, Tensor c, Tensor? dh, Tensor? dh2, Tensor? dc_next,"
        " Tensor(a!) dgates, Tensor(b!) dc_prev) -> ()");
  // (registered before the schemas that name it)
  m.class_<GemmGroupObj>("GemmGroup")
      .def(torch::init<>())
      .def("launch", &GemmGroupObj::launch)
      .def("clear", &GemmGroupObj::clear)
      .def("pieces", &GemmGroupObj::pieces);
  m.def(
      "gemm(Tensor A, int amode, int lda, Tensor B, int bmode, int ldb, int M, int N, int K, Tensor(a!) out, int ldc,"
      " Tensor? bias, int bias_axis, int act, float alpha, float beta, bool atomic, int splits, int tile,"
      " Tensor? aux, int ld_aux, int aux_act, int b_ones_row, float keep, int seed, Tensor? counter,"
      " Tensor? pooled, Tensor? argmax, int PH, int PW, int PC, Tensor(b!)? out2, int ldc2, bool out2_trans,"
      " Tensor(c!)? bias_out, Tensor(d!)? ws, Tensor(e!)? tile_ctr, int a_ones_row=-1, Tensor? ones=None,"
      " __torch__.torch.classes.dtfe.GemmGroup? group=None) -> ()");
  m.def(
      "conv_fwd(Tensor x, Tensor w, Tensor? bias, Tensor(a!) y, Tensor(b!)? argmax, int B, int H, int W, int C,"
      " int Cout, int OH, int OW, int KH, int KW, int stride, int pad, bool pool, int act, Tensor(c!)? bn_stats=None)"
      " -> ()");
  m.def(
      "conv_dgrad(Tensor dy, Tensor wt, Tensor(a!) dx, int B, int H, int W, int C, int Cout, int OH, int OW, int KH,"
      " int KW, int stride, int pad, Tensor? pooled, Tensor? argmax, Tensor? relu_mask, bool accumulate=False,"
      " Tensor? bnb_x=None, Tensor? bnb_y=None, Tensor? bnb_mean=None, Tensor? bnb_invstd=None,"
      " Tensor? bnb_gamma=None, Tensor? bnb_beta=None, Tensor(b!)? bnb_stats=None, int bnb_act=0,"
      " Tensor? acc_src=None, Tensor? acc_mask=None) -> ()");
  m.def(
      "dense_head(Tensor feat, Tensor w, Tensor? bias, Tensor y, Tensor(a!)? logits, Tensor(b!)? loss_sum,"
      " Tensor(c!)? correct, Tensor(d!) dw, Tensor(e!)? db, Tensor(f!)? dfeat, float scale, bool w_fmajor=False,"
      " bool store=False, Tensor(g!)? dl_out=None) -> bool");
  m.def(
      "imgconv(Tensor? src, Tensor? src_pooled, Tensor? src_argmax, Tensor w, Tensor? bias, Tensor(a!) y,"
      " Tensor(b!)? argmax, Tensor? relu_mask, int B, int SH, int SW, int CS, int OH, int OW, int N, int KH, int KW,"
      " int stride, int pad, bool flip_taps, int act, bool pool, int dil=1, Tensor? sc_src=None,"
      " int sc_stride=1, Tensor(e!)? tstamp=None, Tensor(f!)[]? bn_src=None, float bn_eps=0.001,"
      " float bn_momentum=0.99, bool bn_save=False) -> bool");
  m.def(
      "imgwgrad(Tensor src, Tensor? dy, Tensor? dy_pooled, Tensor? dy_argmax, Tensor(a!) dw, Tensor(b!)? db, int B,"
      " int SH, int SW, int CS, int OH, int OW, int N, int KH, int KW, int stride, int pad, float scale, Tensor(c!)? ws=None,"
      " int max_blocks=0, Tensor[]? bn_src=None, float bn_eps=0.001, bool defer=False) -> int[]");
  m.def("wgrad_reduce_group(Tensor[] ws, Tensor(a!)[] dw, Tensor?[] db, float[] scale, int[] desc) -> ()");
  m.def(
      "conv_wgrad(Tensor dz, Tensor x, Tensor(a!) dw, Tensor(b!)? db, int B, int H, int W, int C, int Cout, int OH,"
      " int OW, int KH, int KW, int stride, int pad, float scale) -> ()");
  m.def(
      "head_xent(Tensor h, Tensor w, Tensor? b, Tensor labels, Tensor(a!) dz, Tensor(b!) dl,"
      " Tensor(c!)? loss_sum, Tensor(d!)? correct, Tensor(e!)? logits, float scale, float inv_keep,"
      " Tensor(f!)? step_counter=None, Tensor(g!)? parts=None) -> ()");
  m.def("head_wgrad(Tensor dl, Tensor h, Tensor(a!) dw, Tensor(b!)? db, int nc, float scale, Tensor? parts=None,"
        " Tensor(c!)? loss_sum=None, Tensor(d!)? correct=None,"
        " __torch__.torch.classes.dtfe.GemmGroup? group=None) -> ()");
  m.def(
      "lr_schedule_pack(int kind, int[] bounds, float[] values, float lr, float end, int decay_steps, float inv_decay,"
      " int warmup, float inv_warmup, Tensor device_like) -> Tensor");
  opt_state_register();
  m.def("apply_gradients(__torch__.torch.classes.dtfe.OptState o, Tensor? g, Tensor? g16, float gscale, float lr,"
        " int gs_inc, Tensor? wait_done=None, Tensor(a!)? wait_seen=None, int wait_segs=0, Tensor? clip_scale=None)"
        " -> ()");
  m.def("apply_gradients_group(__torch__.torch.classes.dtfe.OptState[] o, Tensor? g, Tensor? g16, float gscale,"
        " float[] lr, int[] gs_inc, Tensor?[]? clip_scale=None) -> ()");
  m.def("ema_swap(__torch__.torch.classes.dtfe.OptState o) -> ()");
  m.def("grad_sumsq(Tensor? g, Tensor? g16, float gscale, float clip_norm, Tensor plan, Tensor(a!) partials,"
        " Tensor(b!) ticket, Tensor(c!) out, int max_blocks=0) -> ()");
  m.def("scale_(Tensor(a!) t, Tensor scale, Tensor plan) -> ()");
  m.def("layer_trust(Tensor p, Tensor? g, Tensor? g16, float gscale, Tensor plan, Tensor segs, int limit, Tensor wd,"
        " float eeta, float eps, Tensor? clip_scale, Tensor(a!) partials, Tensor(b!) ticket, Tensor(c!) sums,"
        " Tensor(d!) trust, int max_blocks=0) -> ()");
  m.def("eval_metrics(Tensor logits, Tensor labels, int k, Tensor(a!) state, Tensor(b!)? idx, Tensor(c!) ws,"
        " Tensor(d!) ticket) -> ()");
  m.def("wgrad_tallk(Tensor A, int lda, Tensor B, int ldb, int M, int N, int K, Tensor(a!) out, int ldc,"
        " Tensor(b!)? bias, Tensor(c!) ws, int splits, float scale) -> ()");
  m.def("seq_stage(Tensor x, Tensor(a!) xh, int T, int I, Tensor ysrc, Tensor(b!) ydst, Tensor(c!)[] zero) -> ()");
  m.def(
      "gather_rows(Tensor src, Tensor(a!) dst, Tensor? idx, Tensor? labels_src, Tensor(b!)? labels_dst, int seed,"
      " Tensor(c!)? counter, Tensor(d!)? done, Tensor(e!)[] zero, Tensor(f!)? onehot=None, bool shuffle=False) -> ()");
  m.def(
      "augment_rows(Tensor src, Tensor(a!) dst, int H, int W, int C, int pad, bool flip, Tensor? mean, Tensor? inv_std,"
      " Tensor? idx, Tensor? labels_src, Tensor(b!)? labels_dst, int seed, Tensor(c!)? counter, Tensor(d!)? done,"
      " Tensor(e!)[] zero, Tensor(f!)? onehot=None, bool shuffle=False, int mix=0, float label_smoothing=0.0) -> ()");
  m.def("uniform_fill(Tensor(a!) out, float lo, float hi, int seed, Tensor(b!)? counter, Tensor(c!)? done,"
        " Tensor? copy_src=None, Tensor(d!)? copy_dst=None) -> ()");
  m.def("cast_(Tensor src, Tensor(a!) dst) -> ()");
  m.def(
      "softmax_xent(Tensor logits, Tensor? labels_i, Tensor? labels_oh, float scale, Tensor(a!)? dlogits,"
      " Tensor(b!)? loss_rows, Tensor(c!)? loss_sum, Tensor(d!)? correct, Tensor(e!)? probs) -> ()");
  m.def(
      "gan_loss(Tensor d_real, Tensor d_fake, Tensor(a!) gen_loss, Tensor(b!) disc_loss, Tensor(c!) dz_real_disc,"
      " Tensor(d!) dz_fake_disc, Tensor(e!) dz_fake_gen, float clamp_eps) -> ()");
  m.def("gan_disc_head(Tensor d1, Tensor w, Tensor? b, Tensor(a!)? p, Tensor(b!)? dlog, Tensor(c!)? dlog_g,"
        " Tensor(d!) gw, Tensor(e!)? gb, Tensor(f!) dd1, Tensor(g!) ddf, Tensor(h!) gen_loss, Tensor(i!) disc_loss,"
        " Tensor(j!) ws, float clamp_eps=0.0) -> bool");
  m.def("gan_head_ws_floats(int B, int DH) -> int");
  m.def("epoch_signal(Tensor(a!) ctr) -> ()");
  m.def("mse_sigmoid(Tensor y, Tensor t, Tensor(a!) loss, Tensor(b!) dz, Tensor(c!)? ws=None) -> ()");
  m.def("colsum(Tensor x, int M, int N, int ld, Tensor(a!) db, float scale) -> ()");
  m.def("unpool_f32(Tensor g, Tensor argmax, Tensor(a!) out, int B, int PH, int PW, int C) -> ()");
  m.def("head_xent_f32(Tensor h, Tensor w, Tensor? b, Tensor labels, Tensor(a!) dz, Tensor(b!) dl, Tensor(c!) loss_sum,"
        " Tensor(d!) correct, Tensor(e!)? logits, float scale, float inv_keep, Tensor(f!)? step_counter) -> bool");
  m.def("conv1_wgrad_pooled_f32(Tensor dp, Tensor argmax, Tensor x, Tensor(a!) dw, Tensor(b!)? db, Tensor(c!) ws,"
        " int B, int H, int W, int K, float scale) -> bool");
  m.def("transpose_taps_f32(Tensor input, Tensor(a!) out, int O, int T, int C) -> ()");
  m.def("act_grad(Tensor dy, Tensor y, Tensor(a!) dz, int act) -> ()");
  m.def("bias_act(Tensor x, Tensor? bias, Tensor(a!) out, int act, float keep, int seed, Tensor? counter) -> ()");
}

TORCH_LIBRARY_IMPL(dtfe, CUDA, m) {
  m.impl("conv1_gather_fwd", &conv1_gather_fwd);
  m.impl("conv12_gather_fwd", &conv12_gather_fwd);
  m.impl("lstm_seq_fwd", &lstm_seq_fwd);
  m.impl("lstm_seq_bwd", &lstm_seq_bwd);
  m.impl("bn_stats", &bn_stats);
  m.impl("bn_apply", &bn_apply);
  m.impl("bn_infer", &bn_infer);
  m.impl("bn_bwd_stats", &bn_bwd_stats);
  m.impl("bn_bwd_apply", &bn_bwd_apply);
  m.impl("shortcut_grad_add", &shortcut_grad_add);
  m.impl("gap_fwd", &gap_fwd);
  m.impl("gap_bwd", &gap_bwd);
  m.impl("maxpool3_fwd", &maxpool3_fwd);
  m.impl("maxpool3_bwd", &maxpool3_bwd);
  m.impl("bn_relu_pool3", &bn_relu_pool3);
  m.impl("pool3_bn_bwd", &pool3_bn_bwd);
  m.impl("gemm", &gemm);
  m.impl("conv_fwd", &conv_fwd);
  m.impl("conv_dgrad", &conv_dgrad);
  m.impl("conv_wgrad", &conv_wgrad);
  m.impl("head_xent", &head_xent);
  m.impl("head_wgrad", &head_wgrad);
  m.impl("grad_sumsq", &grad_sumsq);
  m.impl("scale_", &scale_);
  m.impl("layer_trust", &layer_trust);
  m.impl("eval_metrics", &eval_metrics);
  m.impl("gather_rows", &gather_rows);
  m.impl("augment_rows", &augment_rows);
  m.impl("seq_stage", &seq_stage);
  m.impl("wgrad_tallk", &wgrad_tallk);
  m.impl("uniform_fill", &uniform_fill);
  m.impl("cast_", &cast_);
  m.impl("softmax_xent", &softmax_xent);
  m.impl("gan_loss", &gan_loss);
  m.impl("mse_sigmoid", &mse_sigmoid);
  m.impl("gan_disc_head", &gan_disc_head);
  m.impl("epoch_signal", &epoch_signal);
  m.impl("colsum", &colsum);
  m.impl("unpool_f32", &unpool_f32);
  m.impl("head_xent_f32", &head_xent_f32);
  m.impl("conv1_wgrad_pooled_f32", &conv1_wgrad_pooled_f32);
  m.impl("transpose_taps_f32", &transpose_taps_f32);
  m.impl("act_grad", &act_grad);
  m.impl("bias_act", &bias_act);
  m.impl("imgconv", &imgconv);
  m.impl("dense_head", &dense_head);
  m.impl("imgwgrad", &imgwgrad);
  m.impl("wgrad_reduce_group", &wgrad_reduce_group);
  m.impl("lstm_cell_fwd", &lstm_cell_fwd);
  m.impl("lstm_cell_bwd", &lstm_cell_bwd);
}

TORCH_LIBRARY_IMPL(dtfe, CompositeExplicitAutograd, m) {
  // not by backend: a gradient on the wrong device reaches the op's own check
  m.impl("apply_gradients", &apply_gradients);
  m.impl("apply_gradients_group", &apply_gradients_group);
  m.impl("ema_swap", &ema_swap);
  m.impl("lr_schedule_pack", &lr_schedule_pack);
  m.impl("gan_head_ws_floats", &gan_head_ws_floats);
}
