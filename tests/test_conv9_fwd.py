"""The 9x9 split forward on two workgroups per CU: every check of tests/conv9_fwd_checks.py once on the CPU kernel emulator
and once on the MI355X."""
import os

import pytest

from tests import conv9_fwd_checks as cf
from tests.emu_fixture import emu  # noqa: F401


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("case", tuple(cf.CASES))
def test_emu(emu, case):
    """(One test per case: its checks share the emulated launches, which take seconds - and minutes in case f, whose point
    is more tiles than the 512 workgroups of the persistent grid.)"""
    for name in cf.CHECKS + (("check_exact",) if case in cf.EXACT_CASES else ()):
        print(name, getattr(cf, name)("cpu", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", tuple(cf.CASES))
@pytest.mark.parametrize("name", cf.CHECKS)
def test_gpu(device_lib, name, case):
    print(getattr(cf, name)("cuda", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cf.EXACT_CASES)
def test_exact_gpu(device_lib, case):
    print(cf.check_exact("cuda", case))
