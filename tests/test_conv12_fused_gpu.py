"""The fused conv1 + conv2 forward launch (ops.conv12_gather_fwd, csrc/kernels/imgconv12_fused.hip)
against the pair of launches it replaces (conv1_gather_fwd + conv2's imgconv): bit-identical outputs.

Batches: the fused kernel runs min(B, 256) workgroups, each persistent over images b, b + 256, ...
  * 256: one image per workgroup, no second iteration;
  * 259: three workgroups take a second image (the ragged prefetch guard, the reuse of aliased LDS);
  * 515: two and three images per workgroup.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

_OUTS = ("x", "labels", "p1", "a1", "p2", "a2")


def _trainer(B, fused, seed=11):
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    tr = MnistCnnTrainer(B, "cuda", seed=seed)
    assert tr.fused_conv12 is True  # the default schedule is the fused launch
    tr.fused_conv12 = fused
    return tr


def _forward_twice(B, fused):
    tr = _trainer(B, fused)
    snaps = []
    for _ in range(2):  # the second call: stale LDS / accumulators, the counter advanced once
        # outputs start from a pattern that differs between the arms: a value the launch leaves unwritten
        # cannot compare equal
        for k in _OUTS:
            getattr(tr, k).view(torch.uint8).fill_(0x55 if fused else 0x2A)
        for t in tr.accum:  # P.grad's head and conv ranges, loss_sum, correct
            t.fill_(3)
        tr.forward()
        torch.cuda.synchronize()
        for i, t in enumerate(tr.accum):
            assert int(torch.count_nonzero(t).item()) == 0, "accumulator range %d not cleared (fused=%s)" % (i, fused)
        snap = {k: getattr(tr, k).clone() for k in _OUTS}
        snap["data_ctr"] = tr.data_ctr.clone()
        snaps.append(snap)
    return snaps


@pytest.mark.parametrize("B", [256, 259, 515])
def test_fused_conv12_forward_matches_the_two_launches(B):
    on, off = _forward_twice(B, True), _forward_twice(B, False)
    for call, (a, b) in enumerate(zip(on, off)):
        assert int(a["data_ctr"].item()) == int(b["data_ctr"].item()) == call + 1  # the head advances it, once
        for k in _OUTS:
            assert torch.equal(a[k], b[k]), "%s differs after forward() call %d at B=%d" % (k, call + 1, B)
    # the two calls sampled different batches (the comparison above is not of one repeated image set)
    assert not torch.equal(on[0]["x"], on[1]["x"])


def test_fused_conv12_steps_match_the_two_launches():
    res = {}
    for fused in (True, False):
        tr = _trainer(320, fused)
        for _ in range(3):
            tr.step()
        torch.cuda.synchronize()
        res[fused] = (tr.P.master.clone(), tr.P.grad.clone(), tr.loss_sum.clone())
    for name, a, b in zip(("P.master", "P.grad", "loss_sum"), res[True], res[False]):
        assert torch.equal(a, b), name
