"""The SSIM training criterion: csrc/ssim_bwd.hip (dasr_ssim_bwd), ops.ssim / ops.ssim_bwd, harness.SSIMLoss and
harness.Trainer(ssim_weight=...).  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_ssim_loss.py runs them.

Truth is float64 autograd through oracle.ssim_ref, pinned to the reference's own ``ssim_loss.SSIM`` by
tests/golden/ssim_loss.npz (tools/make_ssim_loss_golden.py).  The kernel's bound is not a chosen number: it is 4 x the error
of fp32 PyTorch autograd through ssim_ref against the same truth (max abs over max |truth|), the worst over SHAPES,
measured where the test runs; the factor covers the different summation order of a separable, tiled filter."""
import contextlib
import functools
import math
import os

import numpy as np
import torch

from dasr_amd import ops, synth
from oracle import depthnet_oracle as O
from tests.golden_cases import _wave, ssim_inputs
from tests.parity_checks import GOLDEN, build_net
from tests.soft_loss_checks import TRAINER_CASE

T = 32                                       # the kernel's tile (SB_T)
SHAPES = {"small": (2, 3, 24, 31),           # one partial tile
          "edge": (1, 3, T + 1, 2 * T + 1),  # 1-pixel tiles whose halos span a whole neighbour
          "tiny": (1, 1, 7, 5),              # image smaller than the window
          "pixel": (1, 1, 1, 1),             # single pixel
          "hr": (1, 3, 96, 120)}             # interior tiles
MODULE_SHAPE = (2, 3, 128, 160)


def make_pair(name, shape):
    """The recipe of golden_cases.ssim_inputs() (smooth field + hashed texture, the second image a perturbed copy) for any
    [B,C,H,W]; "small" and "hr" ARE its pairs."""
    known = ssim_inputs()
    if name in known:
        assert tuple(known[name][0].shape) == tuple(shape)
        return known[name]
    n = int(np.prod(shape))
    base = 0.5 + 0.35 * _wave(shape, 0.0131, 0.3, torch.float32) * _wave(shape, 0.00071, 1.1, torch.float32)
    tex = synth.hash_uniform(n, "ssim." + name).reshape(shape).to(torch.float32)
    a = (base + 0.1 * (tex - 0.5)).clamp(0, 1)
    b = (a + 0.08 * (synth.hash_uniform(n, "ssim.noise." + name).reshape(shape).to(torch.float32) - 0.5)).clamp(0, 1)
    return a, b


@functools.lru_cache(maxsize=None)
def pairs():
    """name -> (img1, img2), fp32 on the CPU: SHAPES and the identical pair.  Built once, never modified."""
    out = {name: make_pair(name, shape) for name, shape in SHAPES.items()}
    out["identical"] = (out["small"][0], out["small"][0].clone())
    return out


def _autograd(a, b, dtype):
    x = a.to(dtype).clone().requires_grad_(True)           # (a copy: the shared inputs stay as they are)
    v = O.ssim_ref(x, b.to(dtype))
    v.backward()
    return v.item(), x.grad.double()


@functools.lru_cache(maxsize=None)
def truth(name):
    """(S, dS/dimg1) by float64 autograd through oracle.ssim_ref.  Computed once per case, shared, never modified."""
    return _autograd(*pairs()[name], torch.float64)


@functools.lru_cache(maxsize=None)
def fp32_error(name):
    """Error of fp32 PyTorch autograd through ssim_ref against the float64 truth: max abs over max |truth|."""
    want = truth(name)[1]
    return (_autograd(*pairs()[name], torch.float32)[1] - want).abs().max().item() / want.abs().max().item()


@functools.lru_cache(maxsize=None)
def bound():
    figs = {name: fp32_error(name) for name in SHAPES}
    print("fp32 autograd through ssim_ref vs float64:", figs)
    return 4.0 * max(figs.values())


def check_truth_pinned(device=None):
    """The float64 truth against the reference's own module (value of its fp32 run, gradient of its float64 run)."""
    g = np.load(os.path.join(GOLDEN, "ssim_loss.npz"))
    worst = 0.0
    scale = truth("small")[1].abs().max().item()
    for name in pairs():
        v, grad = truth(name)
        assert abs(v - g[name + ".value"].item()) <= 2e-6, (name, v, g[name + ".value"].item())       # check_ssim_kernel's gate
        assert abs(v - g[name + ".value64"].item()) <= 1e-12, (name, v, g[name + ".value64"].item())
        want = torch.from_numpy(g[name + ".grad64"])
        ref = scale if name == "identical" else want.abs().max().item()
        err = (grad - want).abs().max().item() / ref
        worst = max(worst, err)
        assert err <= 1e-10, (name, err)                    # the same float64 formula: only the summation order differs
    return dict(worst=worst)


def _rel(got, want, ref=None):
    want = want.double()
    return (got.double().cpu() - want).abs().max().item() / (want.abs().max().item() if ref is None else ref)


def _one(device, v=1.0):
    return torch.tensor([v], dtype=torch.float32, device=device)


def check_ssim_bwd_op(device):
    """dasr_ssim_bwd against the float64 truth on every shape, and the identical pair gated absolutely."""
    tol = bound()
    figs = {}
    for name in SHAPES:
        a, b = (t.to(device) for t in pairs()[name])
        v = float(ops.ssim(a, b).mean())
        assert abs(v - truth(name)[0]) <= 2e-6, (name, v, truth(name)[0])
        figs[name] = _rel(ops.ssim_bwd(a, b, _one(device)), truth(name)[1])
        print("ssim_bwd", name, SHAPES[name], "kernel", figs[name], "fp32 autograd", fp32_error(name), "bound", tol)
    a, b = (t.to(device) for t in pairs()["identical"])
    figs["identical"] = _rel(ops.ssim_bwd(a, b, _one(device)), truth("identical")[1], truth("small")[1].abs().max().item())
    print("ssim_bwd identical pair (absolute, over max |grad| of 'small')", figs["identical"], "bound", tol)
    for name, f in figs.items():
        assert f <= tol, (name, f, tol)
    return dict(figs, bound=tol)


def check_ssim_bwd_flags(device):
    """accumulate adds the very value accumulate=0 writes; two runs are bit-identical; dscale is read from the device."""
    tol = bound()
    for name in ("small", "edge", "hr"):
        a, b = (t.to(device) for t in pairs()[name])
        base = ops.ssim_bwd(a, b, _one(device))
        assert torch.equal(base, ops.ssim_bwd(a, b, _one(device))), name
        prefill = torch.from_numpy(np.linspace(-1.0, 1.0, a.numel(), dtype=np.float32)).reshape(a.shape).to(device)
        acc = ops.ssim_bwd(a, b, _one(device), out=prefill.clone(), accumulate=True)
        assert torch.equal(acc, prefill + base), name
        over = ops.ssim_bwd(a, b, _one(device), out=prefill.clone())
        assert torch.equal(over, base), name
        m = _rel(ops.ssim_bwd(a, b, _one(device, -0.37)), -0.37 * truth(name)[1])
        assert m <= tol, (name, m, tol)
        zero = ops.ssim_bwd(a, b, _one(device, 0.0))
        assert torch.equal(zero, torch.zeros_like(zero)), name
        assert torch.equal(ops.ssim_bwd(a, b, _one(device, 0.0), out=prefill.clone(), accumulate=True), prefill), name
    return dict(ok=True)


# ---- harness level (GPU) ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _counting(obj, name):
    real, calls = getattr(obj, name), [0]

    def wrapper(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    setattr(obj, name, wrapper)
    try:
        yield calls
    finally:
        setattr(obj, name, real)


@contextlib.contextmanager
def _torch_ssim():
    """SSIMLoss forced to its PyTorch formulation."""
    from dasr_amd import harness
    harness.SSIMLoss.force_torch = True
    try:
        yield
    finally:
        harness.SSIMLoss.force_torch = False


def check_ssim_loss_module(device):
    """SSIMLoss on a leaf sr: the kernels against the PyTorch formulation on the same tensors, value and gradient."""
    from dasr_amd import harness
    tol = bound()
    a, b = (t.to(device) for t in make_pair("module", MODULE_SHAPE))
    crit = harness.SSIMLoss()
    runs = []
    for forced in (False, True):
        sr = a.clone().requires_grad_(True)
        with contextlib.ExitStack() as st, _counting(ops, "ssim") as nf, _counting(ops, "ssim_bwd") as nb:
            if forced:
                st.enter_context(_torch_ssim())
            v = crit(sr, b)
            (-0.5 * v).backward()
            assert (nf[0], nb[0]) == ((0, 0) if forced else (1, 1)), (forced, nf, nb)
        runs.append((float(v), sr.grad))
    (v_hip, g_hip), (v_ref, g_ref) = runs
    dv, dg = abs(v_hip - v_ref) / max(1.0, abs(v_ref)), _rel(g_hip, g_ref.cpu())
    print("SSIMLoss", MODULE_SHAPE, "value", v_hip, v_ref, "grad max-rel", dg, "bound", tol)
    assert dv <= tol and dg <= tol, (dv, dg, tol)
    try:
        crit(a, b.clone().requires_grad_(True))
        raised = False
    except ValueError:
        raised = True
    assert raised, "a second image that requires a gradient must be refused"
    # tensors the kernels do not take: the PyTorch formulation (here: CPU tensors), no kernel call
    with _counting(ops, "ssim") as nf:
        sr = a.cpu().requires_grad_(True)
        v_cpu = crit(sr, b.cpu())
        v_cpu.backward()
        assert nf[0] == 0 and sr.grad is not None and abs(float(v_cpu) - v_ref) <= tol
    return dict(value=dv, grad=dg, bound=tol)


def _batch(first_idx, device):
    return tuple(t.to(device) for t in synth.seeded_batch(first_idx, 2, 16, 20, 8))


GATED = ("conv_output.", "upscale3.")        # behind the loss on the main stream (the depth-branch stream's
#                                              gradients carry an open run-to-run fault this criterion does not touch)


def check_trainer_ssim_step(device):
    """One Trainer(ssim_weight=-0.5) step: the HIP criterion (one node with the fused losses) against the same step with
    SSIMLoss forced to its PyTorch formulation, from identical parameters."""
    from dasr_amd import harness
    runs = []
    for forced in (False, True):
        net, _ = build_net(TRAINER_CASE, device)
        tr = harness.Trainer(net, ssim_weight=-0.5)
        with contextlib.ExitStack() as st, _counting(ops, "ssim") as nf, _counting(ops, "ssim_bwd") as nb:
            if forced:
                st.enter_context(_torch_ssim())
            log = tr.optimize_parameters(*_batch(0, device))
            assert (nf[0], nb[0]) == ((0, 0) if forced else (1, 1)), (forced, nf, nb)
        grads = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()
                 if p.grad is not None and k.startswith(GATED)}
        runs.append(({k: float(log[k]) for k in ("l_ssim", "l_pix", "l_dynamic", "l_all")}, grads))
    (la, ga), (lb, gb) = runs
    print("trainer ssim step:", la, lb)
    for k in ("l_ssim", "l_pix", "l_dynamic"):
        assert abs(la[k] - lb[k]) <= 2e-5 * max(1, abs(lb[k])), (k, la[k], lb[k])
    assert abs(la["l_all"] - (la["l_pix"] + la["l_dynamic"] + la["l_ssim"])) <= 1e-5 * max(1, abs(la["l_all"])), la
    assert -0.5 <= la["l_ssim"] < 0.0, la                  # w * S with w = -0.5 and 0 < S <= 1
    assert set(ga) == set(gb) and any(k.startswith("conv_output.") for k in ga) and any(k.startswith("upscale3.") for k in ga)
    num = sum((ga[k] - gb[k]).pow(2).sum().item() for k in gb)
    den = sum(gb[k].pow(2).sum().item() for k in gb)
    rel = math.sqrt(num / max(den, 1e-300))
    print("trainer ssim step: grad rel L2 over", sorted(gb), rel)
    assert rel <= 2e-5, rel
    return dict(rel=rel)


def check_trainer_ssim_off(device):
    """ssim_weight=None: no l_ssim in the log, and not one call of ops.ssim / ops.ssim_bwd during the step."""
    from dasr_amd import harness
    net, _ = build_net(TRAINER_CASE, device)
    tr = harness.Trainer(net)
    assert tr.ssim_loss is None
    with _counting(ops, "ssim") as nf, _counting(ops, "ssim_bwd") as nb:
        log = tr.optimize_parameters(*_batch(0, device))
        assert (nf[0], nb[0]) == (0, 0), (nf, nb)
    assert sorted(log) == ["l_all", "l_dynamic", "l_pix"], sorted(log)
    return dict(ok=True)


def check_graphed_trainer_ssim(device):
    """Three eager steps, the capture and one replay with the criterion on, against the eager trainer step by step."""
    from dasr_amd import harness
    runs = {}
    for use_graph in (False, True):
        net, _ = build_net(TRAINER_CASE, device)
        tr = harness.Trainer(net, use_graph=use_graph, ssim_weight=-0.5)
        runs[use_graph] = [float(tr.optimize_parameters(*_batch(10 * step, device))["l_ssim"]) for step in range(5)]
        assert (tr._graph is not None) == use_graph
    le, lg = runs[False], runs[True]
    print("graphed vs eager l_ssim:", le, lg)
    assert all(math.isfinite(b) and abs(a - b) <= 3e-3 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    return dict(eager=le, graph=lg)


def check_fused_ssim_collective(device):
    """The multi-rank HIP path on real device memory (the pattern of test_rccl_bucketed_allreduce_single_rank): a one-rank
    RCCL group cannot show a sum, so the harness is told the world is 2.  The all-reduce then returns this rank's vector, and
    every GLOBAL value must come out as exactly that vector's entry over 2 - S from entry 2K + 1, the L1 sum from entry 2K -
    while S itself and its gradient are those of the single-rank call; then the same through one Trainer step."""
    import torch.distributed as dist
    from dasr_amd import harness
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29573")
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    real_world = harness._world
    try:
        K = 10
        lq, gt, dm, mk = _batch(0, device)
        noise = synth.hash_uniform(gt.numel(), "ssim.dp").reshape(gt.shape).float().to(device)
        w = (1.0 + 0.1 * torch.arange(K, dtype=torch.float32)).to(device)
        res = {}
        for world in (1, 2):
            harness._world = (lambda group=None: 2) if world == 2 else real_world
            sr = (gt + 0.1 * (noise - 0.5)).clamp(0, 1).requires_grad_(True)
            out = harness.fused_losses(sr, gt, mk.clone(), w, 1.0, 10.0, dist.group.WORLD if world == 2 else None,
                                       with_ssim=True)
            assert out is not None and len(out) == 7
            l_pix, l_dyn, _, _, l_pix_glob, S, S_glob = out
            dS, = torch.autograd.grad(S, sr, retain_graph=True)
            res[world] = (float(l_pix), float(l_dyn), float(l_pix_glob), S.detach().clone(), S_glob.clone(), dS)
        harness._world = real_world
        (pix1, dyn1, pixg1, S1, Sg1, dS1), (pix2, dyn2, pixg2, S2, Sg2, dS2) = res[1], res[2]
        assert torch.equal(S1, S2) and torch.equal(dS1, dS2) and torch.equal(Sg1, S1)
        assert torch.equal(Sg2, S1 / 2), (float(Sg2), float(S1))             # entry 2K + 1 of the collective, over the world
        assert 0.5 < float(S1) < 1.0 and abs(pix1 - float(S1)) > 0.1          # (S and the L1 value cannot be mistaken for each other)
        # (the loss sums are added with float atomics: two launches differ in the last bits)
        assert abs(pix2 - pix1) <= 1e-6 * pix1 and abs(pixg2 - pix1 / 2) <= 1e-6 * pix1 and pixg1 == pix1, (pix1, pix2, pixg1, pixg2)
        assert abs(dyn2 - dyn1) <= 2e-5 * max(1, abs(dyn1)), (dyn1, dyn2)
        # one Trainer step: the logged terms are the global ones
        logs = {}
        for world in (1, 2):
            net, _ = build_net(TRAINER_CASE, device)
            tr = harness.Trainer(net, group=dist.group.WORLD, ssim_weight=-0.5)
            if world == 2:
                tr._enable_dp(2)
                harness._world = lambda group=None: 2
            with _counting(ops, "ssim") as nf, _counting(ops, "ssim_bwd") as nb:
                log = tr.optimize_parameters(*_batch(0, device))
                assert (nf[0], nb[0]) == (1, 1), (nf, nb)
            harness._world = real_world
            logs[world] = {k: float(v) for k, v in log.items()}
        print("pretended world 2:", logs)
        for k in ("l_ssim", "l_pix"):
            assert abs(logs[2][k] - logs[1][k] / 2) <= 2e-5 * max(1, abs(logs[1][k])), (k, logs)
        assert abs(logs[2]["l_all"] - (logs[2]["l_pix"] + logs[2]["l_dynamic"] + logs[2]["l_ssim"])) <= 1e-5, logs
        return dict(S=float(S1), S_global=float(Sg2))
    finally:
        harness._world = real_world
        if own:
            dist.destroy_process_group()
