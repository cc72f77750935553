"""What ResNetProgram's backward reports to a bucket hook holds: a gradient reported final does not change."""
import pytest
import torch

from dtfe.models.resnet import ResNetModel


@pytest.mark.parametrize("arch,B", [("resnet20", 2)])
def test_reported_gradients_are_final(arch, B):
    torch.manual_seed(0)
    prog = ResNetModel(arch=arch).program("cpu", B, seed=0)
    seen = []
    prog.grad_ready = lambda lo, after=None: seen.append((lo, prog.P.grad.clone()))
    x = torch.rand(B, 32, 32, 3)
    y = torch.nn.functional.one_hot(torch.randint(0, 10, (B,)), 10).float()
    prog.load_batch((x, y))
    prog.compute_grads()
    final = prog.P.grad
    assert seen and seen[-1][0] == 0 and float(final.abs().sum()) > 0
    for lo, snap in seen:
        assert 0 <= lo <= prog.P.total
        assert torch.equal(snap[lo:], final[lo:]), "a gradient at or above offset %d changed after ready(%d)" % (lo, lo)
