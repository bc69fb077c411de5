"""Geometric self-ensemble inference (the reference's test_x8): the expand / ingest / merge kernels of csrc/ensemble.hip,
validate.test_x8, video.FrameUpscaler(self_ensemble=True) and validate.validate_u8(self_ensemble=True) - the checks of
tests/ensemble_checks.py once on the CPU kernel emulator and once on the MI355X; the larger networks, the captured graph and
validate_u8 on the MI355X only."""
import os

import pytest

from tests import ensemble_checks as ec
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_expand", "check_ingest", "check_merge", "check_masks_commute", "check_conditioning_stamps",
        "check_test_x8_members", "check_upscaler_ensemble")
GPU_ONLY = ("check_test_x8_members_x8", "check_ensemble_graph", "check_validate_u8_ensemble")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(ec, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(ec, name)("cuda"))
