"""The one-hot SEAN kernels at op level against float64, unclaimed pixels inside the image, forward workgroups whose tile
chunk crosses a sample boundary: every check of tests/onehot_sean_checks.py once on the CPU kernel emulator and once on the
MI355X."""
import os

import pytest

from tests import onehot_sean_checks as oc
from tests.emu_fixture import emu  # noqa: F401

CHECKS = ("check_onehot_op_vs_float64", "check_onehot_bf16", "check_onehot_fwd_crosses_samples",
          "check_onehot_whole_net_unclaimed", "check_scalar_region_limit", "check_dynk_odd_latent")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


def test_fwd_plan():
    """fwd_plan against hand-worked splits: the benchmark shape and a launch with fewer tiles than workgroups."""
    tps, chunks = oc.fwd_plan(16, 128, 160, 64, True)           # 80 tiles per sample, 1280 tiles over 512 workgroups
    assert tps == 80 and len(chunks) == 512 and chunks[0] == (0, 3) and chunks[255] == (765, 768)
    assert chunks[256] == (768, 770) and chunks[-1] == (1278, 1280)
    assert oc.crossing_workgroups(16, 128, 160, 64, True)
    tps, chunks = oc.fwd_plan(2, 9, 33, 96, False)              # two slices: 384 slots, 8 tiles
    assert tps == 4 and chunks == [(i, i + 1) for i in range(8)]
    assert oc.crossing_workgroups(2, 9, 33, 96, False) == []


@pytest.mark.parametrize("name", CHECKS)
def test_emu(emu, name):
    print(getattr(oc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHECKS)
def test_gpu(device_lib, name):
    print(getattr(oc, name)("cuda"))
