"""Soft depth masks from the depth map: dasr_depth_to_masks_soft, prep.depth_to_soft_masks and the ``soft_masks=`` argument
of FrameUpscaler / validate_u8 / BatchMaker - the checks of tests/soft_prep_checks.py once on the CPU kernel emulator and
once on the MI355X; the captured upscaler and the trainer on soft batches on the MI355X only."""
import os

import pytest

from tests import soft_prep_checks as sc
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_soft_rule_bits", "check_soft_rule_properties", "check_soft_continuity", "check_soft_refusals",
        "check_prep_stamp", "check_whole_net_forward", "check_batch_maker_soft", "check_defaults_unchanged")
GPU_ONLY = ("check_upscaler_soft", "check_upscaler_soft_graph", "check_trainer_takes_soft_batches")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(sc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(sc, name)("cuda"))
