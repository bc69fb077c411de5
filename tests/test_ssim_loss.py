"""The SSIM training criterion (csrc/ssim_bwd.hip, harness.SSIMLoss, harness.Trainer(ssim_weight=...)): the kernel-level
checks of tests/ssim_loss_checks.py once on the CPU kernel emulator and once on the MI355X, the harness-level ones (CUDA
tensors, hipGraph) on the MI355X; the float64 truth they share is pinned to the reference's own module on the CPU."""
import os

import pytest

from tests import ssim_loss_checks as sc
from tests.emu_fixture import emu  # noqa: F401

BOTH = ("check_ssim_bwd_op", "check_ssim_bwd_flags")
GPU_ONLY = ("check_ssim_loss_module", "check_trainer_ssim_step", "check_trainer_ssim_off", "check_graphed_trainer_ssim",
            "check_fused_ssim_collective")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


def test_truth_matches_reference():
    print(sc.check_truth_pinned())


def test_yml_keys_to_ssim_weight():
    from dasr_amd import networks
    on = {"train": {"ssim_loss": {"use_ssim_criterion": True, "ssim_weight": -0.25}}}
    off = {"train": {"ssim_loss": {"use_ssim_criterion": False, "ssim_weight": 1.0}}}
    assert networks.ssim_weight(on) == -0.25 and networks.ssim_weight(off) is None and networks.ssim_weight({}) is None


def test_cpu_trainer_ssim_fallback():
    """CPU tensors: the PyTorch formulation, l_ssim = w * S logged and part of l_all; None leaves the log as it was."""
    import torch
    from dasr_amd import harness

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor(0.9))

        def forward(self, lq, depth, masks):
            return torch.nn.functional.interpolate(lq, scale_factor=2, mode="nearest") * self.w

    torch.manual_seed(0)
    lq, depth = torch.rand(2, 3, 8, 10), torch.rand(2, 1, 8, 10)
    gt = torch.nn.functional.interpolate(lq, scale_factor=2, mode="nearest")
    region = torch.arange(80).reshape(8, 10) % 10                                   # every region non-empty
    masks = torch.nn.functional.one_hot(region, 10).permute(2, 0, 1).float().expand(2, 10, 8, 10).contiguous()
    net = Net()
    log = harness.Trainer(net, ssim_weight=-0.5).optimize_parameters(lq, gt, depth, masks)
    want = -0.5 * float(harness.ssim_torch(0.9 * gt, gt))
    assert abs(float(log["l_ssim"]) - want) <= 1e-6, (float(log["l_ssim"]), want)
    assert abs(float(log["l_all"]) - float(log["l_pix"] + log["l_dynamic"] + log["l_ssim"])) <= 1e-6
    assert net.w.grad is not None
    log0 = harness.Trainer(Net()).optimize_parameters(lq, gt, depth, masks)
    assert sorted(log0) == ["l_all", "l_dynamic", "l_pix"]


def _dp_worker(rank, world, port, B, H, W, q):
    import torch
    import torch.distributed as dist
    from dasr_amd import harness, synth
    from tests.test_dp_gloo import _TinyNet
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    net = _TinyNet()
    tr = harness.Trainer(net, 10, ssim_weight=-0.5)
    assert tr.world == world
    per = B // world
    log = tr.optimize_parameters(*synth.seeded_batch(rank * per, per, H, W, 8))
    if rank == 0:
        torch.save(({k: v.detach().clone() for k, v in net.state_dict().items()}, {k: float(v) for k, v in log.items()}), q)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_ssim_step_equals_single_process_step(tmp_path):
    """2 gloo ranks with the criterion on: the logged l_ssim is the global value (it rides in the dynamic loss's
    collective), and the averaged gradients give the single-process Adam step on the concatenated batch."""
    import torch
    import torch.multiprocessing as mp
    from dasr_amd import harness, synth
    from tests.test_dp_gloo import _TinyNet, _free_port
    B, H, W = 4, 8, 10
    torch.manual_seed(0)
    net = _TinyNet()
    ref_log = harness.Trainer(net, 10, ssim_weight=-0.5).optimize_parameters(*synth.seeded_batch(0, B, H, W, 8))
    ctx = mp.get_context("spawn")
    q = str(tmp_path / "rank0.pt")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, B, H, W, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    sd, log = torch.load(q)
    for k in ("l_ssim", "l_pix", "l_dynamic", "l_all"):
        assert abs(log[k] - float(ref_log[k])) <= 1e-5 * max(1.0, abs(float(ref_log[k]))), (k, log[k], float(ref_log[k]))
    for k, v in net.state_dict().items():
        assert torch.allclose(sd[k], v, rtol=1e-4, atol=1e-6), k


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(sc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(sc, name)("cuda"))
