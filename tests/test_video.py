"""Video inference: uint8 frame ingest / emit / SSD kernels, the NHWC inference entry, video.FrameUpscaler (eager, captured,
pipelined) and validate.validate_u8 - the checks of tests/video_checks.py once on the CPU kernel emulator and once on the
MI355X; the captured graph (replay, validate_u8 over it, fixed-range masks), the oracle comparison and the 64-bit SSD case on the
MI355X only."""
import os

import pytest

from tests import video_checks as vc
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_ingest_u8", "check_emit_u8", "check_ssd_u8", "check_upscaler_matches_validate", "check_pipeline_order",
        "check_validate_u8")
GPU_ONLY = ("check_ssd_u8_large", "check_upscaler_vs_oracle", "check_graph_replay", "check_validate_u8_graph",
            "check_upscaler_fixed_range")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(vc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(vc, name)("cuda"))
