"""Range and per-plane tests of the fp16 x 2 split convolutions: every check of tests/split_range_checks.py once on the CPU
kernel emulator and once on the MI355X (the forms the emulator has no time for: there only)."""
import os

import pytest

from tests import split_range_checks as sr
from tests.emu_fixture import emu  # noqa: F401

CHECKS = ("check_conv3_range", "check_conv9_range", "check_exactness")
# the forms the emulator's minute has no room for (a 64 -> 64 launch takes it 2.4 s per sample, the whole net 30 s per pass)
GPU_ONLY = ("check_conv3_other_forms", "check_whole_net_dark_frame")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


def test_model_vs_float64():
    print(sr.check_model_vs_float64())


@pytest.mark.parametrize("name", CHECKS)
def test_emu(emu, name):
    print(getattr(sr, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHECKS + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(sr, name)("cuda"))
