"""DeviceEvaluator and the --eval_every CLI on the GPU: ResNet-20, B = 8, 20 test rows (chunks of 8, 8, 4).
The bodies are test_device_eval_cpu.py's, run on the device."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_device_eval_cpu import (agrees_with_evaluate, cli_local_mode, construction_errors,  # noqa: E402
                                  flags_restored_when_forward_raises, graph_and_eager_agree, nothing_else_moves)

pytestmark = pytest.mark.gpu
GPU = ("cuda:0", 8, 20)


def test_evaluator_agrees_with_evaluate_gpu():
    agrees_with_evaluate(*GPU)


def test_evaluator_graph_and_eager_bit_equal_gpu():
    graph_and_eager_agree(*GPU)


def test_evaluator_moves_nothing_else_gpu():
    nothing_else_moves(*GPU)


def test_evaluator_restores_flags_when_forward_raises_gpu(monkeypatch):
    flags_restored_when_forward_raises(*GPU, monkeypatch)


def test_evaluator_construction_errors_gpu():
    construction_errors(*GPU)


def test_cli_eval_every_gpu(tmp_path):
    cli_local_mode("cuda", 8, 20, tmp_path)
