"""The pipelined fused conv1 + conv2 forward (csrc/kernels/imgconv12_fused.hip): while conv2's k loop of image i
runs, conv1's input of image i + 1 (row -> P, x, label, the shifted copies) is built and row i + 2 is fetched;
conv2's p2 / a2 staging lies in the border of the LDS image and is zeroed again after it has left.  Every output
stays bit-identical to the two launches (MnistCnnTrainer.fused_conv12 = False).

The kernel runs 256 workgroups, each persistent over images b, b + 256, ...:
  * 256: one image per workgroup - the prologue's staging and the epilogue only, nothing built ahead;
  * 257: exactly one workgroup has a next image (built ahead, nothing fetched behind it);
  * 259, 515: two to three images per workgroup with uneven tails (515: a row fetched two images ahead, the
    border staging reused after its re-zeroing, workgroups that stop one image earlier than others).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

_OUTS = ("x", "labels", "p1", "a1", "p2", "a2")


def _trainer(B, fused, seed=23):
    from dtfe.models.mnist_cnn import MnistCnnTrainer

    tr = MnistCnnTrainer(B, "cuda", seed=seed)
    assert tr.fused_conv12 is True  # the default schedule is the fused launch
    tr.fused_conv12 = fused
    return tr


def _forward_twice(B, fused):
    tr = _trainer(B, fused)
    snaps = []
    for _ in range(2):  # the second call: stale LDS and outputs, the counter advanced once
        for k in _OUTS:  # a pattern that differs between the arms: an unwritten value cannot compare equal
            getattr(tr, k).view(torch.uint8).fill_(0x5A if fused else 0x33)
        for t in tr.accum:
            t.fill_(7)
        tr.forward()
        torch.cuda.synchronize()
        for i, t in enumerate(tr.accum):
            assert int(torch.count_nonzero(t).item()) == 0, "accumulator range %d not cleared (fused=%s)" % (i, fused)
        snap = {k: getattr(tr, k).clone() for k in _OUTS}
        snap["data_ctr"] = tr.data_ctr.clone()
        snaps.append(snap)
    return snaps


@pytest.mark.parametrize("B", [256, 257, 259, 515])
def test_pipelined_conv12_forward_matches_the_two_launches(B):
    on, off = _forward_twice(B, True), _forward_twice(B, False)
    for call, (a, b) in enumerate(zip(on, off)):
        assert int(a["data_ctr"].item()) == int(b["data_ctr"].item()) == call + 1
        assert torch.equal(a["data_ctr"], b["data_ctr"])
        for k in _OUTS:
            assert torch.equal(a[k], b[k]), "%s differs after forward() call %d at B=%d" % (k, call + 1, B)
    assert not torch.equal(on[0]["x"], on[1]["x"])  # two different batches were compared


def test_pipelined_conv12_steps_match_the_two_launches():
    res = {}
    for fused in (True, False):
        tr = _trainer(320, fused)
        for _ in range(3):
            tr.step()
        torch.cuda.synchronize()
        res[fused] = (tr.P.master.clone(), tr.P.grad.clone(), tr.loss_sum.clone())
    for name, a, b in zip(("P.master", "P.grad", "loss_sum"), res[True], res[False]):
        assert torch.equal(a, b), name
