"""Soft depth masks in the fused loss and the captured training step: the kernel-level checks of tests/soft_loss_checks.py
once on the CPU kernel emulator and once on the MI355X, the harness-level ones (CUDA tensors, hipGraph) on the MI355X."""
import os

import pytest

from tests import soft_loss_checks as sl
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_soft_loss_op", "check_soft_kernels_on_onehot")
GPU_ONLY = ("check_soft_loss_large", "check_fused_dispatch", "check_trainer_soft_step", "check_graphed_trainer_soft")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(sl, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(sl, name)("cuda"))
