"""The 9x9 split dgrad with the fused activation / PixelShuffle backward: every check of tests/conv9_dgrad_act_checks.py once
on the CPU kernel emulator and once on the MI355X.  The whole-net check runs on the GPU only: its emulator pass (a training
step of the x8 net at 64 x 96 HR pixels, every convolution on the fp16 x 2 kernels) takes minutes."""
import os

import pytest

from tests import conv9_dgrad_act_checks as cd
from tests.emu_fixture import emu  # noqa: F401


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("case", tuple(cd.CASES))
@pytest.mark.parametrize("name", cd.CHECKS)
def test_emu(emu, name, case):
    print(getattr(cd, name)("cpu", case))


@pytest.mark.parametrize("case", cd.PLAIN_CASES)
def test_plain_emu(emu, case):
    print(cd.check_plain("cpu", case))


def test_refused_emu(emu):
    assert cd.check_refused("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", tuple(cd.CASES))
@pytest.mark.parametrize("name", cd.CHECKS)
def test_gpu(device_lib, name, case):
    print(getattr(cd, name)("cuda", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cd.PLAIN_CASES)
def test_plain_gpu(device_lib, case):
    print(cd.check_plain("cuda", case))


@pytest.mark.gpu
def test_refused_gpu(device_lib):
    assert cd.check_refused("cuda")


@pytest.mark.gpu
def test_net_gpu(device_lib, monkeypatch):
    print(cd.check_net("cuda", monkeypatch))
