"""The small kernels (dynk, instnorm, weight norm, the 1- and 3-channel convolution, region pooling) at op level against
float64: every check of tests/small_kernel_checks.py once on the CPU kernel emulator and once on the MI355X."""
import os

import pytest

from tests import small_kernel_checks as sc
from tests.emu_fixture import emu  # noqa: F401

CHECKS = ("check_dynk_shapes", "check_instnorm_shapes", "check_weight_norm_shapes", "check_c1_conv_shapes",
          "check_region_pool_shapes")


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
