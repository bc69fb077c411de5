"""Soft depth masks up to 16 regions on the fp32-MFMA kernels: every check of tests/soft_mask_checks.py once on the CPU
kernel emulator and once on the MI355X."""
import os

import pytest

from tests import soft_mask_checks as sc
from tests.emu_fixture import emu  # noqa: F401

CHECKS = ("check_soft_op_vs_float64", "check_soft_dispatch", "check_soft_bf16_k16", "check_soft_dD_repeatable",
          "check_soft_whole_net_k16", "check_soft_whole_net_c32_resized", "check_mask_pack_k16")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", CHECKS)
def test_emu(emu, name):
    print(getattr(sc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHECKS)
def test_gpu(device_lib, name):
    print(getattr(sc, name)("cuda"))
