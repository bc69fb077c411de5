"""The pair encoding of two-plane soft depth masks: dasr_depth_to_masks_soft_pair, dasr_sean_fwd_pair[_bf16], the pair
MaskPack and the ``soft_pair=`` switch - the checks of tests/soft_pair_checks.py once on the CPU kernel emulator and once on
the MI355X; the persistent-workgroup case and the captured upscaler on the MI355X only."""
import os

import pytest

from tests import soft_pair_checks as pc
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_producer", "check_producer_refusals", "check_forward_exact", "check_forward_bound", "check_forward_amax",
        "check_forward_refusals", "check_resize", "check_whole_net_forward", "check_training_step", "check_switches",
        "check_stamp")
GPU_ONLY = ("check_upscaler_pair", "check_graphed_trainer_pair")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(pc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(pc, name)("cuda"))
