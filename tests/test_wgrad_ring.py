"""Tile-order and row-ring tests of the fp16 x 2 weight-gradient kernel: every check of tests/wgrad_ring_checks.py once on the
CPU kernel emulator (the two shapes it has time for) and once on the MI355X (those and the other instantiations)."""
import os

import pytest

from tests import wgrad_ring_checks as wr
from tests.emu_fixture import emu  # noqa: F401


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("case", wr.EMU_CASES, ids=wr.case_id)
@pytest.mark.parametrize("name", wr.CHECKS)
def test_emu(emu, name, case):
    print(getattr(wr, name)("cpu", case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", wr.EMU_CASES + wr.GPU_ONLY_CASES, ids=wr.case_id)
@pytest.mark.parametrize("name", wr.CHECKS)
def test_gpu(device_lib, name, case):
    print(getattr(wr, name)("cuda", case))
