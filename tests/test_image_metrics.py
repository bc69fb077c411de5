"""The test script's metrics on the device - PSNR, SSIM, PSNR_Y, SSIM_Y of uint8 frames (csrc/metrics.hip,
ops.image_metrics_u8, validate.image_metrics, validate.test_u8): the checks of tests/image_metrics_checks.py once on the CPU
kernel emulator and once on the MI355X; test_u8's graph, self-ensemble and soft-mask options on the MI355X only."""
import os

import pytest

from tests import image_metrics_checks as ic
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_against_restatement", "check_flat_and_extreme", "check_identical", "check_gray", "check_batch_and_repeat",
        "check_refusals", "check_test_u8")
GPU_ONLY = ("check_test_u8_options",)


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(ic, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(ic, name)("cuda"))
