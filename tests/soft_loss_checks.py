"""Soft (non one-hot) depth masks in the fused loss and the captured training step (csrc/loss.hip: k_loss_sums_soft /
k_loss_bwd_soft; harness._LossSums, harness.fused_losses, harness.Trainer; prep.mark_soft).  Each check takes the
device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_soft_loss.py runs them.

Gates of the loss values and gradients are the project's own for these quantities (parity_checks.check_fused_loss):
l_pix 2e-6, l_dyn 2e-5 (both times max(1, |.|)), d/dsr and d/dw 2e-5 of the largest reference entry - against the oracle
run in FLOAT64 on the same masks.  The oracle's own fp32 run sits within 3e-7 (dsr) and 2.3e-6 (dw) of its float64 run on
these inputs, so the gates leave about 8x."""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

from dasr_amd import ops, synth
from oracle import depthnet_oracle as O
from tests.parity_checks import ZERO_GRAD_KEYS, build_net, rel_max

SHAPES = [(2, 6, 7, 8), (1, 5, 9, 2), (2, 4, 5, 3)]          # (B, h, w, scale): the shapes of check_fused_loss
KS = (1, 7, 10, 16)
TRAINER_CASE = dict(scale=8, which=[0, 1, 2], L=32, nb=5, B=2, H=16, W=20)


def soft_masks(mk, kind, gen):
    """(a) 0.7*onehot + 0.3*rand; (b) 2*rand - 0.5 with exact zeros where a second rand < 0.3: negatives, zeros, values > 1."""
    if kind == "a":
        return 0.7 * mk + 0.3 * torch.rand(mk.shape, generator=gen)
    assert kind == "b"
    m = 2.0 * torch.rand(mk.shape, generator=gen) - 0.5
    m[torch.rand(mk.shape, generator=gen) < 0.3] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def make_inputs(B, h, w, s, K, kind):
    """(sr, gt, masks, loss weights) on the CPU; masks drawn first, then sr.  ``kind`` None: the one-hot masks themselves."""
    lq, gt, dm, mk = synth.seeded_batch(7, B, h, w, s, K)
    gen = torch.Generator().manual_seed(3)
    masks = mk.float() if kind is None else soft_masks(mk.float(), kind, gen)
    sr = (gt + 0.6 * torch.randn(gt.shape, generator=gen)).clamp(-1, 2)
    sr[0, 0, 0, :3] += 3.0                                    # |d| > 1: the linear branch of smooth-L1
    if kind is not None:                                      # a region of tiny area would turn the gates into rounding noise
        assert masks.mean(dim=(0, 2, 3)).min().item() >= 0.05, (B, h, w, s, K, kind)
    return sr, gt, masks.contiguous(), 1.0 + 0.1 * torch.arange(K, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def oracle_f64(B, h, w, s, K, kind):
    """O.total_loss in float64 on the CPU: (l_pix, l_dyn, dsr, dw).  Computed once per case, shared, never modified."""
    sr, gt, masks, wts = make_inputs(B, h, w, s, K, kind)
    sr_o = sr.double().requires_grad_(True)
    w_o = wts.double().requires_grad_(True)
    total, l_pix, l_dyn, _ = O.total_loss(sr_o, gt.double(), masks.double(), w_o)
    total.backward()
    return l_pix.item(), l_dyn.item(), sr_o.grad, w_o.grad


def _gate(got, want, K, what):
    l_pix, l_dyn, dsr, dw = got
    l_pix_o, l_dyn_o, dsr_o, dw_o = want
    figs = dict(l_pix=abs(l_pix - l_pix_o) / max(1, abs(l_pix_o)), l_dyn=abs(l_dyn - l_dyn_o) / max(1, abs(l_dyn_o)),
                dsr=rel_max(dsr, dsr_o), dw=(dw.double().cpu() - dw_o).abs().max().item() if K == 1 else rel_max(dw, dw_o))
    print(what, figs)
    assert figs["l_pix"] <= 2e-6, (what, figs)
    assert figs["l_dyn"] <= 2e-5, (what, figs)
    assert figs["dsr"] <= 2e-5, (what, figs)
    assert figs["dw"] <= (1e-7 if K == 1 else 2e-5), (what, figs)      # K = 1: dw is identically zero in both runs
    return figs


def _soft_loss_on(device, B, h, w, s, K, kind):
    """harness._LossSums -> num / den, softmax, x 10, exactly as check_fused_loss does for the one-hot op."""
    from dasr_amd import harness
    sr, gt, masks, wts = make_inputs(B, h, w, s, K, kind)
    sr_d = sr.clone().to(device).requires_grad_(True)
    w_d = wts.clone().to(device).requires_grad_(True)
    sums = harness._LossSums.apply(sr_d, gt.to(device), masks.to(device), K, None, False)
    num, den, l1 = sums[:K], sums[K:2 * K].detach(), sums[2 * K]
    l_pix = l1 / sr.numel()
    l_dyn = (F.softmax(w_d, 0) * (num / den)).sum() * 10.0
    (l_pix + l_dyn).backward()
    return l_pix.item(), l_dyn.item(), sr_d.grad, w_d.grad


def check_soft_loss_op(device):
    worst = {}
    for (B, h, w, s) in SHAPES:
        for K in KS:
            for kind in ("a", "b"):
                figs = _gate(_soft_loss_on(device, B, h, w, s, K, kind), oracle_f64(B, h, w, s, K, kind), K,
                             (B, h, w, s, K, kind))
                for k, v in figs.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    return worst


def check_soft_kernels_on_onehot(device):
    """On one-hot masks (one pixel in no bin at all) the soft kernels give what the region-byte kernels give."""
    worst = 0.0
    for (B, h, w, s) in SHAPES:
        for K in KS:
            sr, gt, mk, _ = make_inputs(B, h, w, s, K, None)
            mk = mk.clone()
            mk[0, :, 1, 2] = 0.0                              # a no-bin pixel: all planes zero
            sr_d, gt_d, mk_d = sr.to(device), gt.to(device), mk.to(device)
            region, flag = ops.mask_compress(mk_d)
            assert int(flag.item()) == 0 and int(region[0, 1, 2]) == K
            dsums = (0.5 + torch.rand(2 * K + 1, generator=torch.Generator().manual_seed(5))).to(device)
            a = rel_max(ops.loss_sums_soft(sr_d, gt_d, mk_d, K), ops.loss_sums(sr_d, gt_d, region, K))
            b = rel_max(ops.loss_bwd_soft(sr_d, gt_d, mk_d, dsums, K), ops.loss_bwd(sr_d, gt_d, region, dsums, K))
            assert a <= 2e-5 and b <= 2e-5, (B, h, w, s, K, a, b)
            worst = max(worst, a, b)
    return dict(worst=worst)


# One thread of the soft kernels takes one run in ALL channels, so the launch has B*H*w threads; the grid cap is
# dasr_ew_grid's 2048 workgroups of 256.  B = 2, h = 192, w = 172, s = 8 gives 528 384 runs = 2064 workgroups' worth: just past
# the cap (the grid-stride loop runs a second, partial round) and 2048 workgroups add into each sum.
LARGE = (2, 192, 172, 8, 10, "a")


def check_soft_loss_large(device):
    """Past the grid cap of the soft kernels (the issue's B = 2, h = 96, w = 120 would be 720 workgroups here, since a
    thread takes all three channels of its run: the case is sized just past the 2048-workgroup cap instead, see LARGE)."""
    B, h, w, s, K, kind = LARGE
    assert 2048 * 256 < B * h * s * w < 2 * 2048 * 256
    want = oracle_f64.__wrapped__(*LARGE)                     # 100 MB of float64 gradient: not kept in the cache
    try:
        return _gate(_soft_loss_on(device, *LARGE), want, K, LARGE)
    finally:
        make_inputs.cache_clear()


@contextlib.contextmanager
def _counting(obj, name):
    """Count the calls of ``obj.name`` while the block runs."""
    real, calls = getattr(obj, name), [0]

    def wrapper(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    setattr(obj, name, wrapper)
    try:
        yield calls
    finally:
        setattr(obj, name, real)


def check_fused_dispatch(device):
    from dasr_amd import harness, prep
    B, h, w, s, K = 2, 6, 7, 8, 10
    sr, gt, soft, wts = make_inputs(B, h, w, s, K, "a")

    def run(masks, sr=sr, gt=gt, wts=wts):
        sr_d = sr.clone().to(device).requires_grad_(True)
        w_d = wts.clone().to(device).requires_grad_(True)
        return harness.fused_losses(sr_d, gt.to(device), masks, w_d, 1.0, 10.0), sr_d, w_d

    # soft masks: the fused path, at the oracle's values
    with _counting(ops, "loss_sums") as n_hot, _counting(ops, "loss_sums_soft") as n_soft:
        fused, sr_d, w_d = run(soft.to(device))
        assert fused is not None and (n_hot[0], n_soft[0]) == (0, 1)
    l_pix, l_dyn = fused[0], fused[1]
    (l_pix + l_dyn).backward()
    _gate((l_pix.item(), l_dyn.item(), sr_d.grad, w_d.grad), oracle_f64(B, h, w, s, K, "a"), K, "fused_losses")
    # 17 regions, and a non-integer H/h ratio: the PyTorch formulation
    sr17, gt17, soft17, w17 = make_inputs(B, h, w, s, 17, "a")
    assert run(soft17.to(device), sr17, gt17, w17)[0] is None
    assert run(soft[:, :, :5].contiguous().to(device))[0] is None            # H / h = 48 / 5
    assert run(soft[:, :, :, :6].contiguous().to(device))[0] is None         # H / h = 8, W / w = 56 / 6
    # one-hot masks still take the region-byte kernels
    onehot = make_inputs(B, h, w, s, K, None)[2].to(device)
    with _counting(ops, "loss_sums") as n_hot, _counting(ops, "loss_sums_soft") as n_soft:
        assert run(onehot)[0] is not None and (n_hot[0], n_soft[0]) == (1, 0)
    # the classification costs one compression per tensor, none at all after mark_soft, and one again after an edit
    with _counting(ops, "mask_compress") as n:
        t = soft.to(device)
        assert prep.attach_region(t) is False
        assert run(t)[0] is not None
        assert prep.attach_region(t) is False
        assert n[0] <= 1, n
        t2 = prep.mark_soft(soft.to(device))
        before = n[0]
        assert prep.attach_region(t2) is False and run(t2)[0] is not None and prep.attach_region(t2) is False
        assert n[0] == before, n
        t2.mul_(1.0)                                          # an in-place edit drops the stamp
        assert not prep.marked_soft(t2)
        assert prep.attach_region(t2) is False and n[0] == before + 1, n
        t.add_(0.0)
        assert prep.attach_region(t) is False and n[0] == before + 2, n
        # edited into one-hot masks: the soft stamp must not survive
        t.copy_(onehot)
        assert prep.attach_region(t) is True and not prep.marked_soft(t)
    return dict(ok=True)


def _soft_batch(first_idx, seed, device):
    lq, gt, dm, mk = synth.seeded_batch(first_idx, 2, 16, 20, 8)
    soft = soft_masks(mk.float(), "a", torch.Generator().manual_seed(seed))
    return lq.to(device), gt.to(device), dm.to(device), soft.contiguous().to(device)


def check_trainer_soft_step(device):
    """One Trainer step on soft masks: the fused soft path against the PyTorch formulation, from identical parameters."""
    from dasr_amd import harness
    runs = []
    for fused in (True, False):
        net, _ = build_net(TRAINER_CASE, device)
        tr = harness.Trainer(net)
        lq, gt, dm, soft = _soft_batch(0, 3, device)
        real = harness.fused_losses
        if not fused:
            harness.fused_losses = lambda *a, **k: None
        try:
            with _counting(ops, "loss_sums_soft") as n:
                log = tr.optimize_parameters(lq, gt, dm, soft)
            assert n[0] == (1 if fused else 0), n
        finally:
            harness.fused_losses = real
        grads = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters() if p.grad is not None}
        grads["loss.trainable_weight"] = tr.dynamic_loss.trainable_weight.grad.detach().double().cpu()
        runs.append((float(log["l_pix"]), float(log["l_dynamic"]), grads))
    (pix_a, dyn_a, ga), (pix_b, dyn_b, gb) = runs
    assert abs(pix_a - pix_b) <= 2e-5 * max(1, abs(pix_b)), (pix_a, pix_b)
    assert abs(dyn_a - dyn_b) <= 2e-5 * max(1, abs(dyn_b)), (dyn_a, dyn_b)
    assert set(ga) == set(gb)
    num = den = 0.0
    for k in gb:
        if any(z in k for z in ZERO_GRAD_KEYS):
            continue
        num += (ga[k] - gb[k]).pow(2).sum().item()
        den += gb[k].pow(2).sum().item()
    rel = math.sqrt(num / max(den, 1e-300))
    print("trainer soft step: l_pix", pix_a, pix_b, "l_dynamic", dyn_a, dyn_b, "grad rel L2", rel)
    assert rel <= 2e-5, rel
    return dict(rel=rel)


def check_graphed_trainer_soft(device):
    """The protocol of test_graphed_trainer_matches_eager on soft masks (0.7 * the step's one-hot masks + 0.3 * rand), then
    a one-hot batch through the soft-captured step, and the one-hot-captured step's refusal of soft masks."""
    from dasr_amd import harness, prep
    runs, trainers = {}, {}
    net0, _ = build_net(TRAINER_CASE, device)
    init = {k: v.detach().clone() for k, v in net0.state_dict().items()}
    for use_graph in (False, True):
        net, _ = build_net(TRAINER_CASE, device)
        tr = harness.Trainer(net, use_graph=use_graph)
        losses = []
        for step in range(7):
            log = tr.optimize_parameters(*_soft_batch(10 * step, 100 + step, device))
            losses.append(float(log["l_all"]))
        assert (tr._graph is not None) == use_graph
        runs[use_graph] = (losses, {k: v.detach().clone() for k, v in net.state_dict().items()})
        trainers[use_graph] = tr
    le, lg = runs[False][0], runs[True][0]
    assert all(abs(a - b) <= 3e-3 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    dot = na = nb = 0.0
    for k, v0 in init.items():
        if any(z in k for z in ZERO_GRAD_KEYS):
            continue
        ua, ub = (runs[False][1][k] - v0).double().flatten(), (runs[True][1][k] - v0).double().flatten()
        dot += float(ua @ ub); na += float(ua @ ua); nb += float(ub @ ub)
    cosine = dot / (na * nb) ** 0.5
    assert cosine >= 0.98, cosine
    # a one-hot batch through the step captured on soft masks, against an eager step from the same parameters
    tr = trainers[True]
    lq, gt, dm, _ = _soft_batch(70, 0, device)
    net2, _ = build_net(TRAINER_CASE, device)
    net2.load_state_dict(tr.net.state_dict())
    tr2 = harness.Trainer(net2)
    with torch.no_grad():
        tr2.dynamic_loss.trainable_weight.copy_(tr.dynamic_loss.trainable_weight)
    got = float(tr.optimize_parameters(lq, gt, dm, prep.depth_to_masks(dm, 10))["l_all"])
    want = float(tr2.optimize_parameters(lq, gt, dm, prep.depth_to_masks(dm, 10))["l_all"])
    assert math.isfinite(got) and abs(got - want) <= 3e-3 * max(1.0, abs(want)), (got, want)
    # captured on one-hot masks: soft masks are refused as before
    net3, _ = build_net(TRAINER_CASE, device)
    tr3 = harness.Trainer(net3, use_graph=True)
    for step in range(4):
        lq, gt, dm, _ = _soft_batch(10 * step, 0, device)
        tr3.optimize_parameters(lq, gt, dm, prep.depth_to_masks(dm, 10))
    assert tr3._graph is not None
    try:
        tr3.optimize_parameters(*_soft_batch(40, 104, device))
        raised = False
    except ValueError as e:
        raised = "one-hot" in str(e)
    assert raised, "a step captured on one-hot masks must refuse soft masks"
    print("graphed vs eager on soft masks: losses", le, lg, "update cosine", cosine, "one-hot batch", got, want)
    return dict(cosine=cosine)
