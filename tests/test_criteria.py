"""The reference's other training criteria (csrc/loss.hip: the ``_crit`` family; harness.criterion_losses;
harness.Trainer(pixel_criterion=, dynamic_criterion=, mask_criterion=, mask_weight=, dynamic_weight=None); networks.criteria):
the kernel-level checks of tests/criteria_checks.py once on the CPU kernel emulator and once on the MI355X, the harness-level
ones (CUDA tensors, hipGraph) on the MI355X; the float64 truth they share is pinned to the reference's own modules on the
CPU."""
import os

import pytest

from tests import criteria_checks as cc
from tests.emu_fixture import emu  # noqa: F401

KERNEL_CASES = [(s, False) for s in cc.SCALES] + [(4, True)]
KERNEL_IDS = ["scale%d%s" % (s, "_unaligned" if u else "") for s, u in KERNEL_CASES]
BOTH = ("check_crit_golden_case", "check_default_bits", "check_refusals")
GPU_ONLY = ("check_default_unchanged", "check_graphed_static_mask", "check_trainer_ssim_l2", "check_crit_collective")


@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


def test_truth_matches_reference():
    print(cc.check_truth_pinned())


def test_abi_declares_and_exports_the_family():
    import ctypes
    from dasr_amd import _lib, build
    fns = _lib.declared_functions()
    lib = ctypes.CDLL(build.build_hip(verbose=False))
    for name in ("dasr_loss_sums_crit", "dasr_loss_bwd_crit", "dasr_loss_sums_soft_crit", "dasr_loss_bwd_soft_crit"):
        assert name in fns and fns[name][1][-4:] == ["int", "int", "int", "void*"], name
        assert hasattr(lib, name), name


def test_yml_keys_to_criteria():
    """The ``train:`` keys of a shipped yml (train_depthNet_SEAN_depthMask_x8.yml:85-115, typed in), and the switches."""
    from dasr_amd import networks
    train = {"lr_G": 1e-3, "pixel_criterion": "l1", "pixel_weight": 1.0,
             "depth_loss": {"depth_criterion": "l1", "depth_weight": [0.1, 0, 0, 0], "use_depth_criterion": False},
             "vgg_loss": {"use_vgg_criterion": False, "vgg_type": "vgg19"},
             "ssim_loss": {"use_ssim_criterion": False, "ssim_weight": 1.0},
             "mask_loss": {"use_mask_criterion": False, "mask_criterion": "smoothl1", "mask_weight": 1.0},
             "dynamic_loss": {"use_dynamic_criterion": True, "dynamic_criterion": "smoothl1", "dynamic_weight": 10.0}}
    default = dict(pixel_criterion="l1", pixel_weight=1.0, dynamic_criterion="smoothl1", dynamic_weight=10.0,
                   mask_criterion=None, mask_weight=1.0)
    assert networks.criteria({"train": train}) == default
    assert networks.criteria({}) == default and networks.criteria({"train": None}) == default
    train["pixel_criterion"] = "cb"
    train["mask_loss"] = {"use_mask_criterion": True, "mask_criterion": "l2", "mask_weight": 0.5}
    train["dynamic_loss"] = {"use_dynamic_criterion": False, "dynamic_criterion": "l1", "dynamic_weight": 3.0}
    assert networks.criteria({"train": train}) == dict(pixel_criterion="cb", pixel_weight=1.0, dynamic_criterion="l1",
                                                       dynamic_weight=None, mask_criterion="l2", mask_weight=0.5)
    train["dynamic_loss"]["use_dynamic_criterion"] = True
    assert networks.criteria({"train": train})["dynamic_weight"] == 3.0


def test_region_criterion_cb_is_refused():
    import torch
    from dasr_amd import harness
    net = cc.SrNet(torch.zeros(1, 3, 2, 2))
    for kw in (dict(dynamic_criterion="cb"), dict(mask_criterion="cb")):
        with pytest.raises(NotImplementedError, match="CharbonnierLoss"):
            harness.Trainer(net, **kw)
    with pytest.raises(NotImplementedError):
        harness.Trainer(net, pixel_criterion="smoothl1")
    with pytest.raises(NotImplementedError):
        harness.Trainer(net, dynamic_criterion="huber")


def test_cpu_trainer_matches_reference_every_combination():
    print(cc.check_cpu_trainer_vs_golden())


def test_cpu_default_trainer_unchanged():
    print(cc.check_default_unchanged("cpu"))


def test_cpu_packed_collective_pretended_world():
    print(cc.check_crit_collective("cpu"))


def test_training_state_without_dynamic_term(tmp_path):
    """dynamic_weight=None: no loss weights in the optimizer, none in the saved state, no l_dynamic; resume works."""
    import numpy as np
    import torch
    from dasr_amd import harness
    sr, hr, masks = cc.make_inputs(2, 10, "onehot")
    tr = harness.Trainer(cc.SrNet(sr), 10, dynamic_weight=None, mask_criterion="l2")
    np.random.seed(1)
    log = tr.optimize_parameters(None, hr, None, masks)
    assert sorted(log) == ["l_all", "l_mask", "l_pix"] and tr.dynamic_loss is None
    assert sum(len(g["params"]) for g in tr.optimizer.param_groups) == 1
    path = str(tmp_path / "1.state")
    tr.save_training_state(path)
    state = torch.load(path)
    assert "loss_weights" not in state
    tr2 = harness.Trainer(cc.SrNet(sr), 10, dynamic_weight=None, mask_criterion="l2")
    tr2.resume_training(path)
    assert tr2.step_count == 1
    assert "loss_weights" in _default_state(tmp_path)


def _default_state(tmp_path):
    import torch
    from dasr_amd import harness
    sr, hr, masks = cc.make_inputs(2, 10, "onehot")
    tr = harness.Trainer(cc.SrNet(sr), 10)
    tr.optimize_parameters(None, hr, None, masks)
    path = str(tmp_path / "d.state")
    tr.save_training_state(path)
    return torch.load(path)


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
    tr = harness.Trainer(net, 10, dynamic_criterion="l2", pixel_criterion="l2")
    assert tr.world == world
    per = B // world
    log = tr.optimize_parameters(*synth.seeded_batch(rank * per, per, H, W, 8))
    if rank == 0:
        torch.save(({k: v.detach().clone() for k, v in net.state_dict().items()}, {k: float(v) for k, v in log.items()},
                    tr.dynamic_loss.trainable_weight.detach().clone()), q)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_l2_step_equals_single_process_step(tmp_path):
    """2 gloo ranks with dynamic_criterion='l2' (and pixel l2): the logged terms are the global batch's - the region means
    need no denominators - and the averaged gradients give the single-process Adam step on the concatenated batch."""
    import torch
    import torch.multiprocessing as mp
    from dasr_amd import harness, synth
    from tests.test_dp_gloo import _TinyNet, _free_port
    B, H, W = 4, 8, 10
    torch.manual_seed(0)
    net = _TinyNet()
    ref = harness.Trainer(net, 10, dynamic_criterion="l2", pixel_criterion="l2")
    ref_log = ref.optimize_parameters(*synth.seeded_batch(0, B, H, W, 8))
    ctx = mp.get_context("spawn")
    q = str(tmp_path / "rank0.pt")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, B, H, W, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    sd, log, w = torch.load(q)
    assert sorted(log) == ["l_all", "l_dynamic", "l_pix"]
    for k in log:
        assert abs(log[k] - float(ref_log[k])) <= 1e-5 * max(1.0, abs(float(ref_log[k]))), (k, log[k], float(ref_log[k]))
    for k, v in net.state_dict().items():
        assert torch.allclose(sd[k], v, rtol=1e-4, atol=1e-6), k
    assert torch.allclose(w, ref.dynamic_loss.trainable_weight.detach(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("s,unaligned", KERNEL_CASES, ids=KERNEL_IDS)
def test_emu_kernels(emu, s, unaligned):
    print(cc.check_crit_kernels("cpu", s, unaligned))


@pytest.mark.parametrize("name", BOTH)
def test_emu(emu, name):
    print(getattr(cc, name)("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("s,unaligned", KERNEL_CASES, ids=KERNEL_IDS)
def test_gpu_kernels(device_lib, s, unaligned):
    print(cc.check_crit_kernels("cuda", s, unaligned))


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOTH + GPU_ONLY)
def test_gpu(device_lib, name):
    print(getattr(cc, name)("cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", cc.PIXEL)
@pytest.mark.parametrize("net_name", ("tiny", "x4_nb4"))
def test_gpu_trainer_combinations(device_lib, net_name, pixel):
    print(cc.check_trainer_combos("cuda", net_name, pixel))
