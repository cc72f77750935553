// torch.classes.dtfe.OptState: one optimizer bound to the native side - built and validated once
// (torch_ops.cpp), launched by apply_gradients / apply_gradients_group and by the ps service with
// only what varies per launch.
#pragma once
#include <ATen/ATen.h>
#include <torch/custom_class.h>

#include <vector>

#include "../kernels/optim.h"

struct OptStateObj : torch::CustomClassHolder {
  // segs: int64 [nseg, 6] = (off, R, T, C, w16_ptr, wt16_ptr); work: int64 [nwork, 7] = (kind, seg, t, r0,
  // c0, start, count); wd: float32 [nseg], the L2 weight decay of each segment (absent: 0 everywhere) - all
  // three on the CPU.  The w16 / wt16 addresses are the caller's to keep alive (FlatParams does).
  // ema: the shadow buffer of an exponential moving average, float32 as long as p (absent: none), with its
  // decay, the num_updates form and the scalar that receives the decay a launch used (OptArgs::ema*).
  // seg_lr: a device float32 [>= nseg] factor of the rate per segment (OptArgs::seg_lr; absent: none), momentum only.
  OptStateObj(int64_t kind, at::Tensor p, c10::optional<at::Tensor> s1, c10::optional<at::Tensor> s2, double beta1,
              double beta2, double eps, double momentum, double rho, c10::optional<at::Tensor> beta_pow,
              c10::optional<at::Tensor> global_step, at::Tensor done, const at::Tensor& segs, const at::Tensor& work,
              const c10::optional<at::Tensor>& wd, c10::optional<at::Tensor> sched, c10::optional<at::Tensor> lr_out,
              bool nesterov, bool decay, c10::optional<at::Tensor> ema, double ema_decay, bool ema_num_updates,
              c10::optional<at::Tensor> ema_out, c10::optional<at::Tensor> seg_lr);

  // every field that holds for the optimizer's life; a launch copies it and sets g / g16, gscale, lr,
  // gs_inc, wait_* and clip_scale
  dtfe::OptArgs args{};
  std::vector<dtfe::OptSeg> segs;    // the plan as packed into the device blob
  std::vector<dtfe::OptWork> work;
  int64_t numel = 0;                 // of p: the least a gradient may have
  int dev = -1;
  std::vector<at::Tensor> held;      // every tensor whose pointer args holds, and the plan blob
};

// registers the class, once; every library block whose schemas name it calls this first (the blocks of
// different files initialise in no fixed order)
void opt_state_register();
