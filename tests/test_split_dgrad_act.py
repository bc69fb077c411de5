"""The 32-produced-channel split dgrad with the fused activation / PixelShuffle backward: every check of
tests/split_dgrad_act_checks.py once on the CPU kernel emulator and once on the MI355X.  The whole-net check runs on the GPU
only: its emulator pass (training steps of the x8 net at 64 x 96 HR pixels, every convolution on the fp16 x 2 kernels) takes
minutes."""
import os

import pytest

from tests import split_dgrad_act_checks as sd
from tests.emu_fixture import emu  # noqa: F401


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("case", tuple(sd.CASES))
@pytest.mark.parametrize("name", sd.CHECKS)
def test_emu(emu, name, case):
    print(getattr(sd, name)("cpu", case))


def test_plain_unchanged_emu(emu):
    print(sd.check_plain_unchanged("cpu"))


def test_refused_emu(emu):
    assert sd.check_refused("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", tuple(sd.CASES))
@pytest.mark.parametrize("name", sd.CHECKS)
def test_gpu(device_lib, name, case):
    print(getattr(sd, name)("cuda", case))


@pytest.mark.gpu
def test_plain_unchanged_gpu(device_lib):
    print(sd.check_plain_unchanged("cuda"))


@pytest.mark.gpu
def test_refused_gpu(device_lib):
    assert sd.check_refused("cuda")


@pytest.mark.gpu
def test_net_gpu(device_lib, monkeypatch):
    print(sd.check_net("cuda", monkeypatch))
