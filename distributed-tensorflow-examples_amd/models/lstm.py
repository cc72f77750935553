"""MNIST row-sequence LSTM classifier (reference ``lstm/distributed_lstm.py``).

x[B,28,28] -> 28 steps of BasicLSTMCell(128, forget_bias=1.0) -> h_T . W_out + b_out
-> softmax cross-entropy; GradientDescent(0.001); accuracy on 128 test images.
Variables in creation order: Variable (W_out [128,10]), Variable_1 (b_out [10]),
rnn/basic_lstm_cell/kernel [156,512] (glorot-uniform), rnn/basic_lstm_cell/bias
[512] (zeros), Variable_2 (global_step).

MI355X step program (fp32): the per-step gate GEMM reads one [x_t, h_{t-1}]
row buffer (h_{t-1} is written straight into it by the previous cell kernel),
so each timestep is one exact-fp32 MFMA GEMM + one fused cell kernel; BPTT is
one fused cell-backward kernel + one dgrad GEMM per step, and the kernel
gradient is a single [156 x 512] GEMM reducing over all T*B rows at the end
(TF accumulates 28 separate MatMul grads).  On the GPU the whole forward
recurrence and the whole BPTT recurrence are each ONE persistent kernel
(csrc/kernels/lstm_seq.hip); the per-step path remains for the
CPU reference and unsupported shapes (DTFE_LSTM_PERSIST=0 forces it).

``set_cell("gru")`` (``--cell gru``) swaps the cell for tf.nn.rnn_cell.GRUCell(128): variables
rnn/gru_cell/gates/{kernel [156,256], bias [256] (ones)} and rnn/gru_cell/candidate/{kernel [156,128],
bias [128] (zeros)} in that order, and the step program GruProgram below (csrc/kernels/gru_seq.hip).

``set_cell("lnlstm")`` (``--cell lnlstm``) is tf.contrib.rnn.LayerNormBasicLSTMCell(128): variables
rnn/layer_norm_basic_lstm_cell/kernel [156,512] (no bias), then .../<scope>/gamma [128] (ones) and .../<scope>/beta
[128] (zeros) for scope = input, transform, forget_gate, output, state, and the step program LnLstmProgram
(csrc/kernels/lnlstm_seq.hip).  One layer, one direction.

``set_cell("gru", layers=L)`` (``--rnn_layers L``, 2..4) stacks L GRU cells, TF1's
MultiRNNCell([GRUCell(128)] * L): the four variables of every cell under rnn/multi_rnn_cell/cell_<l>/gru_cell/, the
kernels of cell_0 with 156 rows and of the cells above with 256, and the step program GruStackProgram.

``set_cell("gru", bidirectional=True)`` (``--bidirectional``) is TF1's bidirectional_dynamic_rnn(GRUCell(128),
GRUCell(128), x): the four variables of each cell under bidirectional_rnn/{fw,bw}/gru_cell/, a head over both final
states (Variable [256, 10]) and the step program GruBidirProgram (csrc/kernels/gru_bidir.hip).
"""
from __future__ import annotations

import os

import torch

from .. import ops
from ..optim import OptimizerConfig, VarSpec
from .base import ModelDef, ScaledScalar, StepProgram, glorot_uniform_init, normal_init, ones_init, zeros_init

T, I, H, NC = 28, 28, 128, 10
LR = 0.001
CELLS = ("lstm", "gru", "lnlstm")
MAX_LAYERS = 4
LN_SCOPES = ("input", "transform", "forget_gate", "output", "state")  # LayerNormBasicLSTMCell's creation order


class LstmModel(ModelDef):
    name = "lstm"
    default_batch = 128
    default_steps = 10000

    def __init__(self, lr: float = LR, cell: str = "lstm", layers: int = 1, bidirectional: bool = False):
        self.lr = lr
        self.set_cell(cell, layers, bidirectional)

    def set_cell(self, cell: str, layers: int = 1, bidirectional: bool = False):
        """--cell: ``lstm`` = BasicLSTMCell(128) (the reference), ``gru`` = tf.nn.rnn_cell.GRUCell(128) with its
        TF1 variable names, creation order and initialisers (gates bias ones, candidate bias zeros), ``lnlstm`` =
        tf.contrib.rnn.LayerNormBasicLSTMCell(128): the kernel, then gamma (ones) and beta (zeros) of the scopes
        input, transform, forget_gate, output, state.
        --rnn_layers: ``layers`` > 1 (gru only) = MultiRNNCell of that many GRUCell(128), each cell's four variables
        in TF1's static_rnn creation order; layers == 1 is the single cell, unchanged.
        --bidirectional (gru, one layer): a forward and a backward GRUCell(128) over the same rows, the head on both
        final states; the fw cell's variables are created before the bw cell's."""
        if cell not in CELLS:
            raise ValueError("--cell=%s: the row-sequence model has %s" % (cell, " / ".join(CELLS)))
        if not 1 <= layers <= MAX_LAYERS:
            raise ValueError("--rnn_layers=%d: 1 to %d recurrent layers" % (layers, MAX_LAYERS))
        if layers > 1 and cell != "gru":
            raise ValueError("--rnn_layers=%d needs --cell=gru: a stacked %s is not implemented (its split "
                             "kernels exchange h across workgroups; only the GRU kernels stack)" % (layers, cell))
        if bidirectional and cell != "gru":
            raise ValueError("--bidirectional needs --cell=gru")
        if bidirectional and layers != 1:
            raise ValueError("--bidirectional with --rnn_layers=%d: a stacked bidirectional GRU is not implemented"
                             % layers)
        self.cell, self.layers, self.bidirectional = cell, layers, bool(bidirectional)
        head = [VarSpec("Variable", ((2 * H if bidirectional else H), NC), normal_init(1.0)),
                VarSpec("Variable_1", (NC,), normal_init(1.0))]
        if bidirectional:
            self.cells, self.specs = [], list(head)  # per direction: (gates kernel, gates bias, candidate kernel, bias)
            for d in ("fw", "bw"):
                pre = "bidirectional_rnn/%s/gru_cell/" % d
                names = tuple(pre + n for n in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias"))
                self.cells.append(names)
                self.specs += [VarSpec(names[0], (I + H, 2 * H), glorot_uniform_init), VarSpec(names[1], (2 * H,), ones_init),
                               VarSpec(names[2], (I + H, H), glorot_uniform_init), VarSpec(names[3], (H,), zeros_init)]
        elif layers > 1:
            self.cells, self.specs = [], list(head)  # per layer: (gates kernel, gates bias, candidate kernel, bias)
            for l in range(layers):
                pre, rows = "rnn/multi_rnn_cell/cell_%d/gru_cell/" % l, (I if l == 0 else H) + H
                names = tuple(pre + n for n in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias"))
                self.cells.append(names)
                self.specs += [VarSpec(names[0], (rows, 2 * H), glorot_uniform_init), VarSpec(names[1], (2 * H,), ones_init),
                               VarSpec(names[2], (rows, H), glorot_uniform_init), VarSpec(names[3], (H,), zeros_init)]
        elif cell == "lnlstm":
            # kernel (no bias: TF creates none with layer_norm), then gamma (ones), beta (zeros) per scope
            pre = "rnn/layer_norm_basic_lstm_cell/"
            self.kname = pre + "kernel"
            self.ln_names = [pre + s + "/" + v for s in LN_SCOPES for v in ("gamma", "beta")]
            self.specs = head + [VarSpec(self.kname, (I + H, 4 * H), glorot_uniform_init)] + [
                VarSpec(n, (H,), ones_init if n.endswith("gamma") else zeros_init) for n in self.ln_names]
        elif cell == "gru":
            self.gk, self.gb = "rnn/gru_cell/gates/kernel", "rnn/gru_cell/gates/bias"
            self.ck, self.cb = "rnn/gru_cell/candidate/kernel", "rnn/gru_cell/candidate/bias"
            self.specs = head + [
                VarSpec(self.gk, (I + H, 2 * H), glorot_uniform_init),
                VarSpec(self.gb, (2 * H,), ones_init),
                VarSpec(self.ck, (I + H, H), glorot_uniform_init),
                VarSpec(self.cb, (H,), zeros_init),
            ]
        else:
            self.kname, self.bname = "rnn/basic_lstm_cell/kernel", "rnn/basic_lstm_cell/bias"
            self.specs = head + [
                VarSpec(self.kname, (I + H, 4 * H), glorot_uniform_init),
                VarSpec(self.bname, (4 * H,), zeros_init),
            ]
        self.var_order = [s.name for s in self.specs] + ["Variable_2"]
        self.gs_name = "Variable_2"
        self.opt_groups = [(OptimizerConfig(kind="sgd", lr=self.lr), [s.name for s in self.specs],
                            ("beta1_power", "beta2_power"))]

    def program(self, device, batch_size=None, seed: int = 0):
        cls = (GruBidirProgram if self.bidirectional else GruStackProgram if self.layers > 1
               else GruProgram if self.cell == "gru" else LnLstmProgram if self.cell == "lnlstm" else LstmProgram)
        return cls(self, device, batch_size or self.default_batch, seed)


class LstmProgram(StepProgram):
    def __init__(self, model: LstmModel, device, batch_size: int, seed: int = 0):
        super().__init__(model, device, batch_size, seed)
        B = batch_size
        f = dict(device=self.device, dtype=torch.float32)
        self.xh = torch.zeros(T, B, I + H, **f)      # [x_t, h_{t-1}] rows
        self.gates = torch.empty(T, B, 4 * H, **f)
        self.act = torch.empty(T, B, 4 * H, **f)
        self.c = torch.empty(T, B, H, **f)
        self.hT = torch.empty(B, H, **f)
        self.logits = torch.empty(B, NC, **f)
        self.y = torch.empty(B, NC, **f)
        self.dlogits = torch.empty(B, NC, **f)
        self.dh = torch.empty(B, H, **f)
        self.dc = torch.empty(B, H, **f)
        self.dg = torch.empty(T, B, 4 * H, **f)
        self.loss = torch.zeros(1, **f)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.device)
        m = model
        self.Wo, self.bo = self.P.view("Variable"), self.P.view("Variable_1")
        self.K, self.b = self.P.view(m.kname), self.P.view(m.bname)
        self.gWo, self.gbo = self.P.gview("Variable"), self.P.gview("Variable_1")
        self.gK, self.gb = self.P.gview(m.kname), self.P.gview(m.bname)
        # the kernel gradient's own split-K workspace (DTFE_LSTM_TALLK=0: the generic GEMM instead)
        self.k_splits = 32  # tall-K kernel-gradient splits (profiles/r2_lstm_wgrad_sweep.txt)
        self.ws_k = None
        if self.device.type == "cuda" and os.environ.get("DTFE_LSTM_TALLK", "1") != "0":
            self.ws_k = torch.empty(ops.tallk_ws_floats(I + H, 4 * H, self.k_splits), **f)
        self._stage = None  # (x, y) of a batch the next forward launch stages (load_batch, GPU)

    def load_batch(self, batch):
        x, y = batch
        B = self.batch_size
        # batch_x.reshape((B, timesteps, num_input)) (LSTM:127): row t of the image is step t.
        # One launch stages x, zeroes h_{-1}, copies the labels and clears the step's loss / hit
        # accumulators (compute_grads then skips its own clearing) - on the GPU the forward launch itself
        # (the split recurrence reads x_t from the images and writes xh in its prologue) when the load is
        # captured together with the step.
        if x.dtype == torch.float32 and y.dtype == torch.float32 and x.numel() == B * T * I and y.numel() == B * NC:
            if (self._persistent() and x.is_contiguous() and y.is_contiguous()
                    and torch.cuda.is_current_stream_capturing()):
                # batch load captured with the step (bench/ref_models.py): staged by the forward launch itself
                # (lstm_seq_fwd xsrc: seq_stage folded in).  An eager load_batch before a graph replay
                # (train.py) must stage now - the replayed forward would not see a later batch.
                self._stage = (x, y)
            else:
                ops.seq_stage(x, self.xh, T, I, y, self.y, zero=(self.loss, self.correct))
            self._acc_cleared = True
            return
        self.xh[:, :, :I].copy_(x.reshape(B, T, I).transpose(0, 1))
        self.xh[0, :, I:].zero_()
        self.y.copy_(y.reshape(B, NC))

    def _persistent(self):
        return self.device.type == "cuda" and os.environ.get("DTFE_LSTM_PERSIST", "1") != "0"

    def forward(self, head=False):
        """``head`` (compute_grads, GPU): the classifier head forward + backward as ONE single-workgroup
        launch (ops.dense_head: logits, softmax-xent, dW_out / db_out stored, dh) instead of the head
        GEMM, softmax_xent and two gradient GEMMs; returns whether it ran."""
        B = self.batch_size
        st, self._stage = self._stage, None
        if st is not None:  # the batch load_batch left for this launch to stage
            xs, ys, ydst, z0, z1 = st[0], st[1], self.y, self.loss, self.correct
        else:
            xs = ys = ydst = z0 = z1 = None
        if self._persistent() and ops.require().lstm_seq_fwd(self.xh, self.K, self.b, 1.0, self.act, self.c,
                                                               self.hT, xs, ys, ydst, z0, z1):
            # (dfeat = dh_T is formed by the BPTT kernel from these dlogits: lstm_seq_bwd(dl=...))
            if head and ops.dense_head(self.hT, self.Wo, self.bo, self.y, self.logits, self.loss, self.correct,
                                       self.gWo, self.gbo, None, 1.0 / B, w_fmajor=True, store=True,
                                       dl_out=self.dlogits):
                return True
            ops.gemm(self.hT, self.Wo, self.logits, M=B, N=NC, K=H, bmode=ops.RMAJ, ldb=NC, bias=self.bo)
            return False
        if st is not None:
            ops.seq_stage(st[0], self.xh, T, I, st[1], self.y, zero=(self.loss, self.correct))
        for t in range(T):
            ops.gemm(self.xh[t], self.K, self.gates[t], M=B, N=4 * H, K=I + H, bmode=ops.RMAJ, ldb=4 * H,
                     bias=self.b)
            if t + 1 < T:
                h_out, ld = self.xh[t + 1, :, I:], I + H
            else:
                h_out, ld = self.hT, H
            ops.lstm_cell_fwd(self.gates[t], self.act[t], self.c[t - 1] if t > 0 else None, self.c[t], h_out, ld,
                              1.0)
        ops.gemm(self.hT, self.Wo, self.logits, M=B, N=NC, K=H, bmode=ops.RMAJ, ldb=NC, bias=self.bo)

    def compute_grads(self):
        B = self.batch_size
        # no P.grad.zero_(): every gradient element is stored (not accumulated) by this step's kernels
        if not getattr(self, "_acc_cleared", False):
            self.loss.zero_()
            self.correct.zero_()
        self._acc_cleared = False
        fused = self.forward(head=True)
        if not fused:
            ops.softmax_xent(self.logits, labels_oh=self.y, scale=1.0 / B, dlogits=self.dlogits, loss_sum=self.loss,
                             correct=self.correct)
            ops.gemm(self.hT, self.dlogits, self.gWo, M=H + 1, N=NC, K=B, amode=ops.RMAJ, lda=H, bmode=ops.RMAJ,
                     ldb=NC, a_ones_row=H, bias_out=self.gbo)
            ops.gemm(self.dlogits, self.Wo, self.dh, M=B, N=H, K=NC, bmode=ops.KMAJ, ldb=NC)
        if fused:
            # the fused head left dlogits (not dh_T): the persistent BPTT forms dh_T = dlogits . W_out^T
            if not ops.require().lstm_seq_bwd(self.K, self.act, self.c, self.dh, self.dg, I, dl=self.dlogits,
                                              wo=self.Wo):
                ops.gemm(self.dlogits, self.Wo, self.dh, M=B, N=H, K=NC, bmode=ops.KMAJ, ldb=NC)
                self._bptt_steps()
        elif self._persistent() and ops.require().lstm_seq_bwd(self.K, self.act, self.c, self.dh, self.dg, I):
            pass  # whole BPTT recurrence in one launch (dc / dh stay on chip)
        else:
            self._bptt_steps()
        if self.ws_k is not None:  # kernel + bias gradient over all T*B rows: split-K slabs (wgrad_tallk.hip)
            ops.wgrad_tallk(self.xh, I + H, self.dg, 4 * H, I + H, 4 * H, T * B, self.gK, bias=self.gb,
                            splits=self.k_splits, workspace=self.ws_k)
        else:
            ops.gemm(self.xh, self.dg, self.gK, M=I + H + 1, N=4 * H, K=T * B, amode=ops.RMAJ, lda=I + H,
                     bmode=ops.RMAJ, ldb=4 * H, a_ones_row=I + H, bias_out=self.gb)
        return {"loss": ScaledScalar(self.loss, 1.0 / B)}

    def _bptt_steps(self):
        """Per-step BPTT: fused cell-backward kernel + dgrad GEMM per timestep (CPU reference /
        shapes the persistent kernel does not cover)."""
        B = self.batch_size
        self.dc.zero_()
        Kh = self.K[I:]  # recurrent rows [H][4H]
        for t in range(T - 1, -1, -1):
            ops.lstm_cell_bwd(self.act[t], self.c[t - 1] if t > 0 else None, self.c[t], self.dh, None, self.dc,
                              self.dg[t], self.dc)
            if t > 0:
                ops.gemm(self.dg[t], Kh, self.dh, M=B, N=H, K=4 * H, bmode=ops.KMAJ, ldb=4 * H)

    def check_health(self):
        """The split persistent kernels (4 CUs per row group) exchange h / dh through memory; a
        peer workgroup that never ran makes the poll time out and set an error word, after which
        that launch's outputs are wrong.  Raise instead of training on them."""
        if self.device.type == "cuda" and int(ops.require().lstm_status(True)) != 0:
            raise RuntimeError("LSTM split kernel: a cross-workgroup h exchange timed out (a peer workgroup "
                               "was not co-resident); that step's activations / gradients are invalid")

    def evaluate(self, images, labels) -> float:
        """accuracy = mean(argmax(softmax(logits)) == argmax(Y)) (LSTM:98-100, 134-138).  Any number
        of images: evaluated in program-batch chunks, the last one padded by repeating rows (only
        the real rows are counted)."""
        n, B = images.shape[0], self.batch_size
        if n == B:
            self.load_batch((images, labels))
            self._acc_cleared = False
            self.forward()
            self.correct.zero_()
            ops.softmax_xent(self.logits, labels_oh=self.y, correct=self.correct)
            return int(self.correct.item()) / n
        hits = 0
        for lo in range(0, n, B):
            m = min(B, n - lo)
            idx = torch.arange(lo, lo + B, device=images.device).clamp_max(n - 1)
            xb, yb = images[idx], labels[idx]
            self.load_batch((xb, yb))
            self._acc_cleared = False
            self.forward()
            hits += int((self.logits[:m].argmax(1) == self.y[:m].argmax(1)).sum().item())
        return hits / n


class GruProgram(StepProgram):
    """The row-sequence model with tf.nn.rnn_cell.GRUCell(128) (LstmModel.set_cell("gru")).

    A GRU step is two dependent GEMMs - the gates over [x_t, h], then the candidate over [x_t, r * h] - so the
    step program keeps TWO row buffers, xh and xrh, each the A operand of one kernel gradient.  On the GPU the
    whole forward and the whole BPTT recurrence are one persistent launch each (csrc/kernels/gru_seq.hip, a
    workgroup per 16 batch rows); there is no per-step HIP path, so the batch must be a multiple of 16 there.
    On the CPU the same ops run their step-by-step fp32 paths."""

    def __init__(self, model: LstmModel, device, batch_size: int, seed: int = 0):
        super().__init__(model, device, batch_size, seed)
        B = batch_size
        if self.device.type == "cuda" and B % 16:
            raise ValueError("--cell=gru on the GPU runs whole 16-row groups: batch size %d is not a multiple "
                             "of 16" % B)
        f = dict(device=self.device, dtype=torch.float32)
        self.xh = torch.zeros(T, B, I + H, **f)    # [x_t, h_{t-1}] rows
        self.xrh = torch.zeros(T, B, I + H, **f)   # [x_t, r_t * h_{t-1}] rows
        self.g = torch.empty(T, B, 2 * H, **f)     # r, u
        self.cand = torch.empty(T, B, H, **f)
        self.hT = torch.empty(B, H, **f)
        self.logits = torch.empty(B, NC, **f)
        self.y = torch.empty(B, NC, **f)
        self.dlogits = torch.empty(B, NC, **f)
        self.dgg = torch.empty(T, B, 2 * H, **f)
        self.dgc = torch.empty(T, B, H, **f)
        self.loss = torch.zeros(1, **f)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.device)
        m = model
        self.Wo, self.bo = self.P.view("Variable"), self.P.view("Variable_1")
        self.Wg, self.bg, self.Wc, self.bc = (self.P.view(n) for n in (m.gk, m.gb, m.ck, m.cb))
        self.gWo, self.gbo = self.P.gview("Variable"), self.P.gview("Variable_1")
        self.gWg, self.gbg, self.gWc, self.gbc = (self.P.gview(n) for n in (m.gk, m.gb, m.ck, m.cb))
        # each kernel gradient's own split-K workspace (two wgrad_tallk launches per step)
        self.k_splits = 32
        self.ws_g = self.ws_c = None
        if self.device.type == "cuda":
            self.ws_g = torch.empty(ops.tallk_ws_floats(I + H, 2 * H, self.k_splits), **f)
            self.ws_c = torch.empty(ops.tallk_ws_floats(I + H, H, self.k_splits), **f)

    def load_batch(self, batch):
        x, y = batch
        B = self.batch_size
        # image row t is step t; one launch stages x into xh, zeroes h_{-1}, copies the labels and clears the
        # step's accumulators.  The forward launch copies the x columns on into xrh.
        if x.dtype == torch.float32 and y.dtype == torch.float32 and x.numel() == B * T * I and y.numel() == B * NC:
            ops.seq_stage(x, self.xh, T, I, y, self.y, zero=(self.loss, self.correct))
            self._acc_cleared = True
            return
        self.xh[:, :, :I].copy_(x.reshape(B, T, I).transpose(0, 1))
        self.xh[0, :, I:].zero_()
        self.y.copy_(y.reshape(B, NC))

    def forward(self, head=False):
        """The recurrence, then the classifier head: with ``head`` (compute_grads) forward + backward of the head
        as one launch where it fits (ops.dense_head; returns whether it ran), else the logits GEMM alone."""
        B = self.batch_size
        if not ops.gru_seq_fwd(self.xh, self.xrh, self.Wg, self.bg, self.Wc, self.bc, self.g, self.cand, self.hT):
            raise RuntimeError("gru_seq_fwd declined the shape (B %d, I %d, H %d): no other GRU path" % (B, I, H))
        if head and ops.dense_head(self.hT, self.Wo, self.bo, self.y, self.logits, self.loss, self.correct,
                                   self.gWo, self.gbo, None, 1.0 / B, w_fmajor=True, store=True,
                                   dl_out=self.dlogits):
            return True
        ops.gemm(self.hT, self.Wo, self.logits, M=B, N=NC, K=H, bmode=ops.RMAJ, ldb=NC, bias=self.bo)
        return False

    def compute_grads(self):
        B = self.batch_size
        # every gradient element is stored (not accumulated) by this step's kernels
        if not getattr(self, "_acc_cleared", False):
            self.loss.zero_()
            self.correct.zero_()
        self._acc_cleared = False
        if not self.forward(head=True):  # a batch too large for the one-workgroup head
            ops.softmax_xent(self.logits, labels_oh=self.y, scale=1.0 / B, dlogits=self.dlogits, loss_sum=self.loss,
                             correct=self.correct)
            ops.gemm(self.hT, self.dlogits, self.gWo, M=H + 1, N=NC, K=B, amode=ops.RMAJ, lda=H, bmode=ops.RMAJ,
                     ldb=NC, a_ones_row=H, bias_out=self.gbo)
        # the BPTT launch forms dh_T = dlogits . W_out^T itself (hT stands in for the unused dhT)
        if not ops.gru_seq_bwd(self.xh, self.Wg, self.Wc, self.g, self.cand, self.hT, self.dgg, self.dgc,
                               dl=self.dlogits, wo=self.Wo):
            raise RuntimeError("gru_seq_bwd declined the shape (B %d, I %d, H %d)" % (B, I, H))
        # kernel + bias gradients over all T*B rows: gWg = [x | h]^T [dr | du], gWc = [x | r h]^T dc
        ops.wgrad_tallk(self.xh, I + H, self.dgg, 2 * H, I + H, 2 * H, T * B, self.gWg, bias=self.gbg,
                        splits=self.k_splits, workspace=self.ws_g)
        ops.wgrad_tallk(self.xrh, I + H, self.dgc, H, I + H, H, T * B, self.gWc, bias=self.gbc,
                        splits=self.k_splits, workspace=self.ws_c)
        return {"loss": ScaledScalar(self.loss, 1.0 / B)}

    evaluate = LstmProgram.evaluate  # program-batch chunks, padded: uses load_batch / forward / logits / y only


class LnLstmProgram(StepProgram):
    """The row-sequence model with tf.contrib.rnn.LayerNormBasicLSTMCell(128) (LstmModel.set_cell("lnlstm")).

    The ten gamma / beta variables are adjacent 128-float blocks of the flat parameter buffer, so the kernels take them
    (and their gradients) as ONE [10][128] view.  On the GPU the forward and the BPTT recurrence are one persistent launch
    each (csrc/kernels/lnlstm_seq.hip, a workgroup per 16 batch rows), the gamma / beta gradients one slab per workgroup
    summed in a fixed order, and the kernel gradient one wgrad_tallk launch; there is no per-step HIP path, so the
    batch must be a multiple of 16 there.  On the CPU the same ops run their step-by-step fp32 paths."""

    def __init__(self, model: LstmModel, device, batch_size: int, seed: int = 0):
        super().__init__(model, device, batch_size, seed)
        B = batch_size
        if self.device.type == "cuda" and B % 16:
            raise ValueError("--cell=lnlstm on the GPU runs whole 16-row groups: batch size %d is not a multiple "
                             "of 16" % B)
        f = dict(device=self.device, dtype=torch.float32)
        self.xh = torch.zeros(T, B, I + H, **f)     # [x_t, h_{t-1}] rows
        self.zhat = torch.empty(T, B, 4 * H, **f)   # normalised gate pre-activations
        self.chat = torch.empty(T, B, H, **f)       # normalised cell state
        self.rs = torch.empty(T, B, 5, **f)         # reciprocal standard deviations
        self.hT = torch.empty(B, H, **f)
        self.logits = torch.empty(B, NC, **f)
        self.y = torch.empty(B, NC, **f)
        self.dlogits = torch.empty(B, NC, **f)
        self.dg = torch.empty(T, B, 4 * H, **f)
        self.ws_ln = torch.empty(max(B // 16, 1), 10, H, **f)  # one gamma / beta gradient slab per workgroup
        self.loss = torch.zeros(1, **f)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.device)
        m, P = model, self.P
        self.Wo, self.bo, self.K = P.view("Variable"), P.view("Variable_1"), P.view(m.kname)
        self.gWo, self.gbo, self.gK = P.gview("Variable"), P.gview("Variable_1"), P.gview(m.kname)
        o = P.offsets[m.ln_names[0]]
        if [P.offsets[n] for n in m.ln_names] != [o + H * i for i in range(10)]:
            raise RuntimeError("lnlstm: the gamma / beta variables are not adjacent in the parameter buffer")
        self.ln, self.gln = P.master[o:o + 10 * H].view(10, H), P.grad[o:o + 10 * H].view(10, H)
        self.k_splits = 32
        self.ws_k = None  # the kernel gradient's own split-K workspace
        if self.device.type == "cuda":
            self.ws_k = torch.empty(ops.tallk_ws_floats(I + H, 4 * H, self.k_splits), **f)

    load_batch = GruProgram.load_batch  # stages x into xh, zeroes h_{-1}, copies the labels, clears the accumulators

    def forward(self, head=False):
        """The recurrence, then the classifier head (as GruProgram.forward)."""
        B = self.batch_size
        if not ops.lnlstm_seq_fwd(self.xh, self.K, self.ln, self.zhat, self.chat, self.rs, self.hT):
            raise RuntimeError("lnlstm_seq_fwd declined the shape (B %d, I %d, H %d): no other path" % (B, I, H))
        if head and ops.dense_head(self.hT, self.Wo, self.bo, self.y, self.logits, self.loss, self.correct,
                                   self.gWo, self.gbo, None, 1.0 / B, w_fmajor=True, store=True,
                                   dl_out=self.dlogits):
            return True
        ops.gemm(self.hT, self.Wo, self.logits, M=B, N=NC, K=H, bmode=ops.RMAJ, ldb=NC, bias=self.bo)
        return False

    def compute_grads(self):
        B = self.batch_size
        # every gradient element is stored (not accumulated) by this step's kernels
        if not getattr(self, "_acc_cleared", False):
            self.loss.zero_()
            self.correct.zero_()
        self._acc_cleared = False
        if not self.forward(head=True):  # a batch too large for the one-workgroup head
            ops.softmax_xent(self.logits, labels_oh=self.y, scale=1.0 / B, dlogits=self.dlogits, loss_sum=self.loss,
                             correct=self.correct)
            ops.gemm(self.hT, self.dlogits, self.gWo, M=H + 1, N=NC, K=B, amode=ops.RMAJ, lda=H, bmode=ops.RMAJ,
                     ldb=NC, a_ones_row=H, bias_out=self.gbo)
        # the BPTT launch forms dh_T = dlogits . W_out^T itself (hT stands in for the unused dhT)
        if not ops.lnlstm_seq_bwd(self.K, self.ln, self.zhat, self.chat, self.rs, self.hT, self.dg, self.gln,
                                  self.ws_ln, dl=self.dlogits, wo=self.Wo):
            raise RuntimeError("lnlstm_seq_bwd declined the shape (B %d, I %d, H %d)" % (B, I, H))
        # kernel gradient over all T*B rows (the cell has no bias)
        ops.wgrad_tallk(self.xh, I + H, self.dg, 4 * H, I + H, 4 * H, T * B, self.gK, splits=self.k_splits,
                        workspace=self.ws_k)
        return {"loss": ScaledScalar(self.loss, 1.0 / B)}

    evaluate = LstmProgram.evaluate  # uses load_batch / forward / logits / y only


class GruStackProgram(StepProgram):
    """L stacked GRUCell(128) (LstmModel.set_cell("gru", layers=L), L > 1).

    Layer 0 reads the image rows and runs on the single layer's kernel, which also writes every h_t into the x
    columns of layer 1's xh.  The input sequence of a layer above is complete before the layer starts, so the x part
    of both its GEMMs is hoisted out of the recurrence: two exact-fp32 GEMMs over all T * B rows project it (biases in
    their epilogue) and the persistent kernel gru_proj_fwd starts each step's accumulators from the projections.
    Backward, top layer first: gru_stack_bwd takes a gradient at every step (dhs), which for layer l is layer
    l + 1's input gradient dx = dgg . Wg[:I]^T + dgc . Wc[:I]^T - two more GEMMs over T * B rows; layer 0's dx is never
    formed.  Every buffer is per layer and every gradient is stored, so the step captures into one hipGraph."""

    def __init__(self, model: LstmModel, device, batch_size: int, seed: int = 0):
        super().__init__(model, device, batch_size, seed)
        B, L = batch_size, model.layers
        if self.device.type == "cuda" and B % 16:
            raise ValueError("--cell=gru on the GPU runs whole 16-row groups: batch size %d is not a multiple "
                             "of 16" % B)
        f = dict(device=self.device, dtype=torch.float32)
        self.In = [I] + [H] * (L - 1)                                        # input width of each layer
        self.xh = [torch.zeros(T, B, i + H, **f) for i in self.In]           # [x_t, h_{t-1}] rows (h_{-1} = 0)
        self.xrh = [torch.zeros(T, B, i + H, **f) for i in self.In]          # [x_t, r_t * h_{t-1}] rows
        self.g = [torch.empty(T, B, 2 * H, **f) for _ in range(L)]
        self.cand = [torch.empty(T, B, H, **f) for _ in range(L)]
        self.hT = [torch.empty(B, H, **f) for _ in range(L)]
        self.dgg = [torch.empty(T, B, 2 * H, **f) for _ in range(L)]
        self.dgc = [torch.empty(T, B, H, **f) for _ in range(L)]
        # layers 1..: the projected inputs and the input gradient (the dhs of the layer below)
        self.xpg = [None] + [torch.empty(T, B, 2 * H, **f) for _ in range(L - 1)]
        self.xpc = [None] + [torch.empty(T, B, H, **f) for _ in range(L - 1)]
        self.dx = [None] + [torch.empty(T, B, H, **f) for _ in range(L - 1)]
        self.logits = torch.empty(B, NC, **f)
        self.y = torch.empty(B, NC, **f)
        self.dlogits = torch.empty(B, NC, **f)
        self.loss = torch.zeros(1, **f)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.Wo, self.bo = self.P.view("Variable"), self.P.view("Variable_1")
        self.gWo, self.gbo = self.P.gview("Variable"), self.P.gview("Variable_1")
        self.W = [tuple(self.P.view(n) for n in names) for names in model.cells]    # (Wg, bg, Wc, bc) per layer
        self.gW = [tuple(self.P.gview(n) for n in names) for names in model.cells]
        self.k_splits = 32
        self.ws = [(None, None)] * L  # each kernel gradient's own split-K workspace
        if self.device.type == "cuda":
            self.ws = [(torch.empty(ops.tallk_ws_floats(i + H, 2 * H, self.k_splits), **f),
                        torch.empty(ops.tallk_ws_floats(i + H, H, self.k_splits), **f)) for i in self.In]

    def load_batch(self, batch):
        x, y = batch
        B = self.batch_size
        if x.dtype == torch.float32 and y.dtype == torch.float32 and x.numel() == B * T * I and y.numel() == B * NC:
            ops.seq_stage(x, self.xh[0], T, I, y, self.y, zero=(self.loss, self.correct))
            self._acc_cleared = True
            return
        self.xh[0][:, :, :I].copy_(x.reshape(B, T, I).transpose(0, 1))
        self.xh[0][0, :, I:].zero_()
        self.y.copy_(y.reshape(B, NC))

    def forward(self, head=False):
        """The L recurrences, then the classifier head on the top layer's h_T (as GruProgram.forward)."""
        B, L, TB = self.batch_size, len(self.In), T * self.batch_size
        Wg, bg, Wc, bc = self.W[0]
        if not ops.gru_seq_fwd(self.xh[0], self.xrh[0], Wg, bg, Wc, bc, self.g[0], self.cand[0], self.hT[0],
                               h2=self.xh[1]):
            raise RuntimeError("gru_seq_fwd declined the shape (B %d, I %d, H %d): no other GRU path" % (B, I, H))
        for l in range(1, L):
            Wg, bg, Wc, bc = self.W[l]
            # the x rows of both kernels over the whole sequence: xh's x columns (pitch 2H) . W[:H] + bias
            ops.gemm(self.xh[l], Wg, self.xpg[l], M=TB, N=2 * H, K=H, lda=2 * H, bmode=ops.RMAJ, ldb=2 * H, bias=bg)
            ops.gemm(self.xh[l], Wc, self.xpc[l], M=TB, N=H, K=H, lda=2 * H, bmode=ops.RMAJ, ldb=H, bias=bc)
            if not ops.gru_proj_fwd(self.xh[l], self.xrh[l], self.xpg[l], self.xpc[l], Wg, Wc, self.g[l], self.cand[l],
                                    self.hT[l], h2=self.xh[l + 1] if l + 1 < L else None):
                raise RuntimeError("gru_proj_fwd declined the shape (B %d, I %d, H %d)" % (B, H, H))
        hT = self.hT[-1]
        if head and ops.dense_head(hT, self.Wo, self.bo, self.y, self.logits, self.loss, self.correct,
                                   self.gWo, self.gbo, None, 1.0 / B, w_fmajor=True, store=True,
                                   dl_out=self.dlogits):
            return True
        ops.gemm(hT, self.Wo, self.logits, M=B, N=NC, K=H, bmode=ops.RMAJ, ldb=NC, bias=self.bo)
        return False

    def compute_grads(self):
        B, L, TB = self.batch_size, len(self.In), T * self.batch_size
        # every gradient element is stored (not accumulated) by this step's kernels
        if not getattr(self, "_acc_cleared", False):
            self.loss.zero_()
            self.correct.zero_()
        self._acc_cleared = False
        if not self.forward(head=True):  # a batch too large for the one-workgroup head
            ops.softmax_xent(self.logits, labels_oh=self.y, scale=1.0 / B, dlogits=self.dlogits, loss_sum=self.loss,
                             correct=self.correct)
            ops.gemm(self.hT[-1], self.dlogits, self.gWo, M=H + 1, N=NC, K=B, amode=ops.RMAJ, lda=H, bmode=ops.RMAJ,
                     ldb=NC, a_ones_row=H, bias_out=self.gbo)
        for l in range(L - 1, -1, -1):
            (Wg, _, Wc, _), (gWg, gbg, gWc, gbc), i = self.W[l], self.gW[l], self.In[l]
            # the top layer starts from dh_T = dlogits . W_out^T (formed in the launch), the others from zeros + dhs
            top = dict(dl=self.dlogits, wo=self.Wo) if l == L - 1 else dict(dhs=self.dx[l + 1])
            if not ops.gru_stack_bwd(self.xh[l], Wg, Wc, self.g[l], self.cand[l], self.dgg[l], self.dgc[l], **top):
                raise RuntimeError("gru_stack_bwd declined the shape (B %d, I %d, H %d)" % (B, i, H))
            if l > 0:  # dx = dgg . Wg[:I]^T + dgc . Wc[:I]^T: the gradient at every h_t of the layer below
                ops.gemm(self.dgg[l], Wg, self.dx[l], M=TB, N=i, K=2 * H, bmode=ops.KMAJ, ldb=2 * H)
                ops.gemm(self.dgc[l], Wc, self.dx[l], M=TB, N=i, K=H, bmode=ops.KMAJ, ldb=H, beta=1.0)
            ops.wgrad_tallk(self.xh[l], i + H, self.dgg[l], 2 * H, i + H, 2 * H, TB, gWg, bias=gbg,
                            splits=self.k_splits, workspace=self.ws[l][0])
            ops.wgrad_tallk(self.xrh[l], i + H, self.dgc[l], H, i + H, H, TB, gWc, bias=gbc,
                            splits=self.k_splits, workspace=self.ws[l][1])
        return {"loss": ScaledScalar(self.loss, 1.0 / B)}

    evaluate = LstmProgram.evaluate  # uses load_batch / forward / logits / y only


class GruBidirProgram(StepProgram):
    """A bidirectional GRU layer (LstmModel.set_cell("gru", bidirectional=True)): GRUCell(128) forward in time and
    GRUCell(128) backward in time over the same image rows, the classifier head on [h_fw(T-1) | h_bw(0)].

    Every recurrence buffer has a leading direction axis (ops.gru_bidir_fwd's contract): the batch is staged once, into
    xh[0], and the backward-in-time direction copies x_t into its own rows.  On the GPU both directions are ONE
    persistent launch forward and ONE for the BPTT, grid (B / 16, 2) (csrc/kernels/gru_bidir.hip): the directions are
    independent, so the second runs on CUs the first leaves idle.  The four kernel gradients read the contiguous
    slices xh[d] / dgg[d] and xrh[d] / dgc[d]; every gradient is stored, so the step captures into one hipGraph."""

    def __init__(self, model: LstmModel, device, batch_size: int, seed: int = 0):
        super().__init__(model, device, batch_size, seed)
        B = batch_size
        if self.device.type == "cuda" and B % 16:
            raise ValueError("--cell=gru on the GPU runs whole 16-row groups: batch size %d is not a multiple "
                             "of 16" % B)
        f = dict(device=self.device, dtype=torch.float32)
        self.xh = torch.zeros(2, T, B, I + H, **f)    # [x_t | the state step t starts from]; both initial states 0
        self.xrh = torch.zeros(2, T, B, I + H, **f)   # [x_t | r_t * state]
        self.g = torch.empty(2, T, B, 2 * H, **f)
        self.cand = torch.empty(2, T, B, H, **f)
        self.feat = torch.empty(B, 2 * H, **f)        # [h_fw after T-1 | h_bw after 0]
        self.logits = torch.empty(B, NC, **f)
        self.y = torch.empty(B, NC, **f)
        self.dlogits = torch.empty(B, NC, **f)
        self.dgg = torch.empty(2, T, B, 2 * H, **f)
        self.dgc = torch.empty(2, T, B, H, **f)
        self.loss = torch.zeros(1, **f)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.Wo, self.bo = self.P.view("Variable"), self.P.view("Variable_1")
        self.gWo, self.gbo = self.P.gview("Variable"), self.P.gview("Variable_1")
        self.W = [tuple(self.P.view(n) for n in names) for names in model.cells]    # (Wg, bg, Wc, bc) per direction
        self.gW = [tuple(self.P.gview(n) for n in names) for names in model.cells]
        self.k_splits = 32
        self.ws = [(None, None)] * 2  # each kernel gradient's own split-K workspace
        if self.device.type == "cuda":
            self.ws = [(torch.empty(ops.tallk_ws_floats(I + H, 2 * H, self.k_splits), **f),
                        torch.empty(ops.tallk_ws_floats(I + H, H, self.k_splits), **f)) for _ in range(2)]

    def load_batch(self, batch):
        x, y = batch
        B = self.batch_size
        # staged once, into direction 0's rows (h_{-1} zeroed); xh[1]'s initial state is never written: zeros
        if x.dtype == torch.float32 and y.dtype == torch.float32 and x.numel() == B * T * I and y.numel() == B * NC:
            ops.seq_stage(x, self.xh[0], T, I, y, self.y, zero=(self.loss, self.correct))
            self._acc_cleared = True
            return
        self.xh[0, :, :, :I].copy_(x.reshape(B, T, I).transpose(0, 1))
        self.xh[0, 0, :, I:].zero_()
        self.y.copy_(y.reshape(B, NC))

    def forward(self, head=False):
        """Both recurrences in one launch, then the classifier head on feat [B][2H] (as GruProgram.forward)."""
        B = self.batch_size
        (Wg0, bg0, Wc0, bc0), (Wg1, bg1, Wc1, bc1) = self.W
        if not ops.gru_bidir_fwd(self.xh, self.xrh, Wg0, bg0, Wc0, bc0, Wg1, bg1, Wc1, bc1, self.g, self.cand,
                                 self.feat):
            raise RuntimeError("gru_bidir_fwd declined the shape (B %d, I %d, H %d): no other GRU path" % (B, I, H))
        if head and ops.dense_head(self.feat, self.Wo, self.bo, self.y, self.logits, self.loss, self.correct,
                                   self.gWo, self.gbo, None, 1.0 / B, w_fmajor=True, store=True,
                                   dl_out=self.dlogits):
            return True
        ops.gemm(self.feat, self.Wo, self.logits, M=B, N=NC, K=2 * H, bmode=ops.RMAJ, ldb=NC, bias=self.bo)
        return False

    def compute_grads(self):
        B = self.batch_size
        # every gradient element is stored (not accumulated) by this step's kernels
        if not getattr(self, "_acc_cleared", False):
            self.loss.zero_()
            self.correct.zero_()
        self._acc_cleared = False
        if not self.forward(head=True):  # a batch too large for the one-workgroup head
            ops.softmax_xent(self.logits, labels_oh=self.y, scale=1.0 / B, dlogits=self.dlogits, loss_sum=self.loss,
                             correct=self.correct)
            ops.gemm(self.feat, self.dlogits, self.gWo, M=2 * H + 1, N=NC, K=B, amode=ops.RMAJ, lda=2 * H,
                     bmode=ops.RMAJ, ldb=NC, a_ones_row=2 * H, bias_out=self.gbo)
        # each direction starts from its half of dlogits . W_out^T, formed in the launch (feat stands in for dhT)
        if not ops.gru_bidir_bwd(self.xh, self.W[0][0], self.W[0][2], self.W[1][0], self.W[1][2], self.g, self.cand,
                                 self.feat, self.dgg, self.dgc, dl=self.dlogits, wo=self.Wo):
            raise RuntimeError("gru_bidir_bwd declined the shape (B %d, I %d, H %d)" % (B, I, H))
        for d in range(2):  # gWg = [x | state]^T [dr | du], gWc = [x | r state]^T dc, per direction
            gWg, gbg, gWc, gbc = self.gW[d]
            ops.wgrad_tallk(self.xh[d], I + H, self.dgg[d], 2 * H, I + H, 2 * H, T * B, gWg, bias=gbg,
                            splits=self.k_splits, workspace=self.ws[d][0])
            ops.wgrad_tallk(self.xrh[d], I + H, self.dgc[d], H, I + H, H, T * B, gWc, bias=gbc,
                            splits=self.k_splits, workspace=self.ws[d][1])
        return {"loss": ScaledScalar(self.loss, 1.0 / B)}

    evaluate = LstmProgram.evaluate  # uses load_batch / forward / logits / y only
