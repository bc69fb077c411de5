"""The SEAN kernels at op level, every kernel form (tests/sean_exact_checks.py): every check once on the CPU kernel
emulator and once on the MI355X."""
import os

import pytest

from tests import sean_exact_checks as sc
from tests.emu_fixture import emu  # noqa: F401

CHECKS = tuple(n for n in dir(sc) if n.startswith("check_"))


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
