"""Data-parallel fine-tuning over RCCL with two ranks — runs on any box that shows at least two GPUs and skips itself on a one-GPU
box, exactly as tests/test_gpu_rccl_multi.py does.  On such a box this is the first N > 1 hardware run of the training path: two
ranks of the training CLI, one GPU each, the gradient rows all-gathered on the device, against the one-process restatement, byte
for byte (tests/test_gpu_train_parallel.py runs the same case with gloo ranks sharing one GPU)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_gpu_train_parallel import _ranks_against_restatement, tiny_data  # noqa: E402,F401

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible GPUs (RCCL with N > 1)')]


def test_two_ranks_over_rccl_equal_the_one_process_restatement(tiny_data):  # noqa: F811
    _ranks_against_restatement(tiny_data, 2, (), backend='nccl')
