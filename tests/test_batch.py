"""Training batches from uint8 HR frames: the LR / GT / plane kernels of csrc/batch.hip, data.resize_tables / draw_augment /
BatchMaker - the checks of tests/batch_checks.py once on the CPU kernel emulator and once on the MI355X; BatchMaker feeding
the captured training step on the MI355X only; draw_augment (host code) once."""
import os

import pytest

from tests import batch_checks as bc
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_lr_value", "check_lr_invariants", "check_gt", "check_plane", "check_masks", "check_refusals",
        "check_end_to_end")
GPU_ONLY = ("check_graphed_trainer",)


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


def test_draw_augment():
    print(bc.check_draw_augment())


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(bc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(bc, name)("cuda"))
