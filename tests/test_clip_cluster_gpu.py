"""--clip_norm through the parameter-server path on the GPU: the worker clips its gradient on the
device (norm + in-place scale inside its captured step) and only then pushes over the native link."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "launch"))
import local_cluster  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.slow]


def test_ps_worker_clips_on_the_device_before_the_native_push(tmp_path):
    lr, clip, steps = 0.01, 1e-3, 4  # softmax: zero-initialised variables, GradientDescent(0.01)
    extra = ["--device=cuda", "--data_dir=/nonexistent", "--seed=1", "--workers=1", "--num_steps=%d" % steps,
             "--save_model_secs=0", "--check_pull", "--clip_norm=%r" % clip, "--model_dir=" + str(tmp_path)]
    codes, out, _ = local_cluster.launch("softmax", 1, 1, extra, timeout=300, stream=False, gpus=1)
    assert all(c == 0 for c in codes.values()), "%s\n%s" % (codes, "\n".join(
        "---- %s\n%s" % (k, "\n".join(v[-40:])) for k, v in out.items()))
    assert any(l.startswith("ps 0: native data plane:") for l in out[("ps", 0)]), out[("ps", 0)][-10:]
    norms = {int(m.group(1)): float(m.group(2)) for l in out[("worker", 0)]
             for m in [re.match(r"pull l2norm gs=(\d+): (\S+)$", l)] if m}
    assert sorted(norms) == list(range(1, steps + 1)), out[("worker", 0)]
    # every update has norm <= lr * C (plain SGD), so after k of them from zero |p| <= k * lr * C;
    # the first gradient's norm is far above C: the first update sits at the bound, not below it
    for k, n in norms.items():
        assert 0 < n <= k * lr * clip * (1 + 1e-5), (k, n)
    assert norms[1] >= lr * clip * (1 - 1e-5), norms
