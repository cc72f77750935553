"""Evaluation on a held-out set during training, without leaving the device.

The test rows and labels are resident on the program's device.  A pass is ``ceil(n / B)`` runs of one
chunk function - gather the chunk's rows into the program's input buffer, inference forward up to the
logits, ``ops.eval_metrics`` - whose whole progress is device state: the evaluation counters, the chunk
cursor and the next chunk's row indices are written by ``eval_metrics`` itself.  So the chunk has no
per-chunk host tensor, runs the same eagerly, while it is captured and when it is replayed, and the
host reads the result once per pass.

A program takes part by offering ``forward_logits()``: the inference forward on the batch loaded in
``program.x`` up to fp32 logits [B][num_classes] (``models.resnet.ResNetProgram``).
"""
from __future__ import annotations

import torch

from .. import ops
from .graphs import StepGraph

PROTOCOL_ERROR = ("%s: periodic evaluation needs a program with an inference forward to fp32 logits "
                  "(forward_logits(): resnet20, resnet50), which %r does not offer")


def supports(program) -> bool:
    """Whether ``program`` offers the evaluation protocol."""
    return callable(getattr(program, "forward_logits", None))


class DeviceEvaluator:
    def __init__(self, prog, images_u8, labels_int, topk: int = 5, examples: int = 0, graph: bool = True):
        """``images_u8`` [n][H*W*C] uint8 and ``labels_int`` [n] (numpy arrays or tensors) are copied to
        ``prog``'s device once; ``examples`` > 0 evaluates the first that many rows only.  ``graph``:
        capture the chunk into a hipGraph (GPU) after an eager warm-up."""
        if not supports(prog):
            raise ValueError(PROTOCOL_ERROR % ("DeviceEvaluator", getattr(prog.model, "name", type(prog).__name__)))
        ncls = int(prog.model.num_classes)
        if not 1 <= int(topk) <= ncls:
            raise ValueError("DeviceEvaluator: topk (--eval_topk) = %d, but the model has %d classes" % (topk, ncls))
        images_u8, labels_int = torch.as_tensor(images_u8), torch.as_tensor(labels_int)
        n = images_u8.shape[0]
        if int(examples) < 0:
            raise ValueError("DeviceEvaluator: examples (--eval_examples) must be >= 0, got %d" % examples)
        if int(examples) > 0:
            n = min(n, int(examples))
        if n < 1 or labels_int.shape[0] < n:
            raise ValueError("DeviceEvaluator: %d images with %d labels" % (n, labels_int.shape[0]))
        if images_u8.dtype != torch.uint8 or images_u8[0].numel() != prog.x[0].numel():
            raise ValueError("DeviceEvaluator: images are uint8 rows of %d values" % prog.x[0].numel())
        self.prog, self.topk, self.n = prog, int(topk), n
        dev, B = prog.device, prog.batch_size
        self.images = images_u8[:n].reshape(n, -1).contiguous().to(dev)
        self.labels = labels_int[:n].reshape(n).to(torch.int32).contiguous().to(dev)
        self.chunks = -(-n // B)
        self.state = ops.eval_state(dev, n)
        self.idx = torch.zeros(B, dtype=torch.int32, device=dev)
        self.lab = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ws = torch.zeros(2 * B, dtype=torch.int32, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self._idx0 = torch.arange(B, dtype=torch.int32).clamp_max(n - 1).to(dev)
        self._graph = bool(graph)
        self._runner = self._norm = None

    @property
    def capture_error(self):
        """The exception that made the chunk fall back to eager launches (None: captured, or not tried)."""
        return self._runner.capture_error if self._runner is not None else None

    @property
    def graph(self):
        return self._runner.graph if self._runner is not None else None

    def _chunk(self):
        p = self.prog
        if p.input_norm is not None:  # the training batches are standardised: so are these (no crop, no flip)
            H, W, C = p.x.shape[1:]
            ops.augment_rows(self.images, p.x, H, W, C, mean=p.input_norm[0], inv_std=p.input_norm[1], idx=self.idx,
                             labels_src=self.labels, labels_dst=self.lab)
        else:
            ops.gather_rows(self.images, p.x, idx=self.idx, labels_src=self.labels, labels_dst=self.lab)
        ops.eval_metrics(p.forward_logits(), self.lab, self.topk, self.state, idx=self.idx, ws=self.ws,
                         ticket=self.ticket)

    def run(self) -> dict:
        """One pass over the set: dict(examples, accuracy, topk_accuracy, loss).  Parameters, moving
        averages, optimizer state and the batchers are left untouched; the step accumulators the forward
        touched are cleared."""
        p = self.prog
        if self._runner is None or p.input_norm is not self._norm:  # (a capture holds the gather it recorded)
            self._norm = p.input_norm
            self._runner = StepGraph(self._chunk, warmup=1, enabled=self._graph and p.device.type == "cuda")
        self.state.zero_()
        self.state[ops.EVAL_N:ops.EVAL_N + 1].fill_(self.n)
        self.idx.copy_(self._idx0)
        bns = p.batchnorms()
        was = [bn.infer for bn in bns], p.training
        for bn in bns:
            bn.infer = True
        p.training = False
        try:
            for _ in range(self.chunks):
                self._runner()
        finally:
            p.training = was[1]
            for bn, f in zip(bns, was[0]):
                bn.infer = f
            for t in p.step_accumulators()[1:]:
                t.zero_()
        st = ops.eval_state_dict(self.state)  # the pass's one host read
        if st["bad_labels"] > 0:
            raise ValueError("DeviceEvaluator: %d of %d labels lie outside [0, %d)"
                             % (st["bad_labels"], st["count"], p.model.num_classes))
        if st["count"] != self.n or st["cursor"] != self.chunks:
            raise RuntimeError("DeviceEvaluator: folded %d rows in %d chunks, expected %d in %d"
                               % (st["count"], st["cursor"], self.n, self.chunks))
        return {"examples": st["count"], "accuracy": st["hits1"] / self.n, "topk_accuracy": st["hitsk"] / self.n,
                "loss": st["loss_sum"] / self.n}
