"""The 9x9 split weight gradient (dy split once, fixed-order slab reduction): every check of tests/conv9_wgrad_checks.py once
on the CPU kernel emulator and once on the MI355X."""
import os

import pytest

from tests import conv9_wgrad_checks as cw
from tests.emu_fixture import emu  # noqa: F401


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("case", tuple(cw.CASES))
def test_emu(emu, case):
    """(One test per case: its checks share the emulated launches.)"""
    for name in cw.CHECKS:
        print(name, getattr(cw, name)("cpu", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", tuple(cw.CASES))
@pytest.mark.parametrize("name", cw.CHECKS)
def test_gpu(device_lib, name, case):
    print(getattr(cw, name)("cuda", case))
