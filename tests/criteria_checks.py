"""The criterion-parametrised losses: csrc/loss.hip (dasr_loss_{sums,bwd}[_soft]_crit), ops.loss_sums_crit / loss_bwd_crit,
harness.criterion_losses, harness.Trainer(pixel_criterion=, dynamic_criterion=, mask_criterion=, mask_weight=,
dynamic_weight=None) and networks.criteria.  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_criteria.py runs them.

Truth is the FLOAT64 run of a restatement of the reference's formulas (``ref_*`` below: the criterion of the MASKED images,
mask_loss.py:22-41,64-90; loss.py:37-47; F_model_depthCond.py:164), pinned to the reference's own modules by
tests/golden/criteria.npz (tools/make_criteria_golden.py).  The same restatement run in fp32 is "the reference's fp32 error"
of a case.  A kernel result is gated at the smaller of

  * 10 x that fp32 error on the same case (never below 10 x 2^-24: the results are fp32 numbers, so no comparison can ask
    for more than their own representation error), and
  * CAP_SUMS / CAP_DSR: 10 x the worst figure measured on the MI355X over all cases.

Figures: sums - the largest relative error of an entry (an entry whose truth is 0, an empty region, must be 0); dsr - the
largest absolute error over the largest |truth|."""
import contextlib
import functools
import itertools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from dasr_amd import ops, synth
from tests.parity_checks import GOLDEN, ZERO_GRAD_KEYS, build_net

PIXEL = ("l1", "l2", "cb")
REGION = ("l1", "l2", "smoothl1")
B_, C_, LR_H, LR_W = 2, 3, 5, 7
SCALES = (2, 3, 4, 8)                           # 2, 3: the scalar path; 4, 8: the vector path
KS = (1, 7, 10, 16)
EPS32 = 2.0 ** -24
CAP_SUMS = 4.5e-6                               # 10 x 4.5e-7: worst sums figure on the MI355X (emulator: 2.6e-7)
CAP_DSR = 3.8e-6                                # 10 x 3.8e-7: worst dsr figure, the emulator's (MI355X: 3.0e-7)
CAP_STEP = 7e-6                                 # fused step against the PyTorch formulation, 10 x the worst on the MI355X:
#                                                 logged term 2.9e-7, update rel-L2 6.2e-7, gradient rel-L2 7.2e-7
GOLDEN_SHAPE = dict(s=2, K=10)
WEIGHTS = dict(pixel_weight=1.0, dynamic_weight=10.0, mask_weight=0.7)
MASK_SEED = 5                                   # np.random.seed before the static mask loss draws its region


# ---- inputs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_inputs(s, K, kind, dyadic=False):
    """(sr, hr, masks) fp32 on the CPU, built once and never modified.  B = 2, C = 3, LR 5 x 7: no HR element count is a
    multiple of 256.  d = sr - hr is drawn in [-3, 3] (both smooth-L1 branches), four elements sit at +-(1 +- 1e-3), and the
    block [:, :, :s, :2s] has sr == hr exactly (sign(0), the cb gradient at 0).  ``kind``: 'onehot' (every region non-empty,
    one LR pixel in no region), 'soft' (negative values, zeros, values above 1), and '*_empty': region K - 1 is empty.
    ``dyadic``: every value a multiple of 1/16, so that every partial sum is exact in fp32 whatever the order of the adds."""
    gen = torch.Generator().manual_seed(1000 * s + 10 * K + (1 if dyadic else 0))
    shape = (B_, C_, LR_H * s, LR_W * s)
    hr = torch.rand(shape, generator=gen)
    d = 6.0 * torch.rand(shape, generator=gen) - 3.0
    if dyadic:
        hr, d = torch.round(hr * 16) / 16, torch.round(d * 16) / 16
    else:
        d.view(-1)[5:9] = torch.tensor([1 - 1e-3, 1 + 1e-3, -(1 - 1e-3), -(1 + 1e-3)])
    sr = hr + d
    sr[:, :, :s, :2 * s] = hr[:, :, :s, :2 * s]
    region = (torch.randperm(B_ * LR_H * LR_W, generator=gen) % K).reshape(B_, LR_H, LR_W)
    if kind.endswith("_empty"):
        assert K >= 2
        region[region == K - 1] = 0
    if kind.startswith("onehot"):
        masks = F.one_hot(region, K).permute(0, 3, 1, 2).float()
        masks[0, :, 1, 2] = 0.0
    else:
        masks = 2.0 * torch.rand((B_, K, LR_H, LR_W), generator=gen) - 0.5
        masks[torch.rand(masks.shape, generator=gen) < 0.3] = 0.0
        if kind.endswith("_empty"):
            masks[:, K - 1] = 0.0
        if dyadic:
            # multiples of 1/2: u = M d is a multiple of 1/32 and every smooth-L1 term one of 2^-11, so a region's
            # numerator (terms >= 0: no partial sum exceeds it) is exact in fp32 in any order while it stays below 2^13
            masks = torch.round(masks * 2) / 2
            u = F.interpolate(masks, scale_factor=s, mode="nearest").double().unsqueeze(2) * (sr - hr).double().unsqueeze(1)
            assert F.smooth_l1_loss(u, torch.zeros_like(u), reduction="none").sum(dim=(0, 2, 3, 4)).max().item() < 2 ** 13
    if not kind.endswith("_empty"):
        assert masks.sum(dim=(0, 2, 3)).min().item() > 0.5, (s, K, kind)
    return sr, hr, masks.contiguous()


# ---- the reference's formulas, restated (any dtype) ----------------------------------------------------------------------
def _masked(sr, hr, masks, k):
    m = F.interpolate(masks[:, k:k + 1], size=sr.shape[2:], mode="nearest")
    m3 = torch.cat([m, m, m], dim=1)
    return m3 * sr, m3 * hr, m3


def ref_pixel(sr, hr, crit, weight):
    if crit == "l1":
        return weight * F.l1_loss(sr, hr)
    if crit == "l2":
        return weight * F.mse_loss(sr, hr)
    diff = sr - hr
    return weight * torch.sum(torch.sqrt(diff * diff + 1e-6))


def ref_region(sr, hr, masks, k, crit):
    a, b, m3 = _masked(sr, hr, masks, k)
    if crit == "smoothl1":
        return torch.sum(F.smooth_l1_loss(a, b, reduction="none")) / torch.sum(m3)
    return F.l1_loss(a, b) if crit == "l1" else F.mse_loss(a, b)


def ref_dynamic(sr, hr, masks, crit, weight, tw=None):
    K = masks.shape[1]
    sm = F.softmax(torch.ones(K, dtype=sr.dtype) if tw is None else tw, dim=0)
    return sum(sm[k] * ref_region(sr, hr, masks, k, crit) for k in range(K)) * weight


def ref_mask(sr, hr, masks, crit, weight, index):
    return weight * ref_region(sr, hr, masks, index, crit)


def ref_sums(sr, hr, masks):
    """The raw sums of the ``_crit`` kernels by the same masked-image formulas: px[crit], num[crit] [K], area [K]."""
    K = masks.shape[1]
    diff = sr - hr
    px = {"l1": diff.abs().sum(), "l2": (diff * diff).sum(), "cb": torch.sqrt(diff * diff + 1e-6).sum()}
    num = {c: [] for c in REGION}
    area = []
    for k in range(K):
        a, b, m3 = _masked(sr, hr, masks, k)
        num["l1"].append((a - b).abs().sum())
        num["l2"].append(((a - b) ** 2).sum())
        num["smoothl1"].append(F.smooth_l1_loss(a, b, reduction="sum"))
        area.append(m3.sum())
    return px, {c: torch.stack(v) for c, v in num.items()}, torch.stack(area)


def combos(with_b=True):
    """(pixel, A, B): every pixel x region pair without a second region criterion, and with each other one."""
    out = []
    for p, a in itertools.product(PIXEL, REGION):
        out.append((p, a, None))
        if with_b:
            out += [(p, a, b) for b in REGION if b != a]
    return out


def _dsums(n, seed):
    return 0.5 + torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _run_ref(s, K, kind, dtype):
    sr, hr, masks = make_inputs(s, K, kind)
    x = sr.to(dtype).clone().requires_grad_(True)
    px, num, area = ref_sums(x, hr.to(dtype), masks.to(dtype))
    out = {}
    for i, (p, a, b) in enumerate(combos()):
        sums = torch.cat([num[a], area, px[p].reshape(1)] + ([num[b]] if b else []))
        w = _dsums(sums.numel(), i).to(dtype)
        w[K:2 * K] = 0                                      # the areas carry no gradient
        dsr, = torch.autograd.grad((w * sums).sum(), x, retain_graph=True)
        out[(p, a, b)] = (sums.detach().double(), dsr.double())
    return out


def sums_error(got, want):
    got, want = got.double().cpu(), want.double()
    if bool(((want == 0) & (got != 0)).any()):
        return math.inf
    nz = want != 0
    return ((got - want).abs()[nz] / want.abs()[nz]).max().item() if bool(nz.any()) else 0.0


def dsr_error(got, want):
    want = want.double()
    return (got.double().cpu() - want).abs().max().item() / want.abs().max().item()


@functools.lru_cache(maxsize=None)
def truth(s, K, kind):
    """combo -> (sums64, dsr64, the fp32 run's sums error, its dsr error).  Computed once per case, shared, never modified."""
    t64, t32 = _run_ref(s, K, kind, torch.float64), _run_ref(s, K, kind, torch.float32)
    return {c: (t64[c][0], t64[c][1], sums_error(t32[c][0], t64[c][0]), dsr_error(t32[c][1], t64[c][1])) for c in t64}


def kinds_for(K, a, b):
    """Empty regions only where the reference gives 0 and not 0/0: under l1 / l2."""
    ks = ["onehot", "soft"]
    if K >= 2 and "smoothl1" not in (a, b):
        ks += ["onehot_empty", "soft_empty"]
    return ks


# ---- golden --------------------------------------------------------------------------------------------------------------
GOLDEN_KINDS = ("onehot", "soft", "onehot_empty", "soft_empty")


def golden_terms():
    """name -> (function of (sr, hr) in any dtype giving the term, with the reference's weights); the terms of criteria.npz.
    The total loss of any combination is a sum of these (F_model_depthCond.py:163-190), and so is its gradient."""
    s, K = GOLDEN_SHAPE["s"], GOLDEN_SHAPE["K"]
    terms = {}
    for c in PIXEL:
        terms["pix." + c] = (None, lambda sr, hr, m, c=c: ref_pixel(sr, hr, c, WEIGHTS["pixel_weight"]))
    for kind in GOLDEN_KINDS:
        for c in REGION:
            if kind.endswith("_empty") and c == "smoothl1":
                continue
            terms["dyn.%s.%s" % (kind, c)] = (kind, lambda sr, hr, m, c=c: ref_dynamic(sr, hr, m, c, WEIGHTS["dynamic_weight"]))
            if not kind.endswith("_empty"):
                terms["mask.%s.%s" % (kind, c)] = (kind, lambda sr, hr, m, c=c: ref_mask(sr, hr, m, c, WEIGHTS["mask_weight"],
                                                                                      mask_index(K)))
    return s, K, terms


def mask_index(K, seed=MASK_SEED):
    """The region mask_loss.py:24 draws first after np.random.seed(seed) (the global state is left as it was)."""
    return int(np.random.RandomState(seed).randint(0, K, 1)[0])


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "criteria.npz"))


def check_truth_pinned(device=None):
    """The float64 restatement against the reference's own modules: every term's value and gradient on the golden inputs
    (which must be the ones make_inputs builds), and the drawn region."""
    g = golden()
    s, K, terms = golden_terms()
    assert int(g["mask_index"].item()) == mask_index(K)
    worst = 0.0
    for name, (kind, fn) in terms.items():
        sr, hr, masks = make_inputs(s, K, kind or "onehot")
        assert np.array_equal(g["sr"], sr.numpy()) and np.array_equal(g["hr"], hr.numpy())
        if kind:
            assert np.array_equal(g["masks." + kind], masks.numpy()), kind
        x = sr.double().requires_grad_(True)
        v = fn(x, hr.double(), masks.double())
        dsr, = torch.autograd.grad(v, x)
        want_v, want_g = g[name + ".value64"].item(), torch.from_numpy(g[name + ".grad64"])
        ev = abs(v.item() - want_v) / max(1.0, abs(want_v))
        eg = (dsr - want_g).abs().max().item() / max(1e-300, want_g.abs().max().item())
        worst = max(worst, ev, eg)
        assert ev <= 1e-12 and eg <= 1e-12, (name, ev, eg)
    return dict(worst=worst)


def golden_fp32_errors():
    """The reference's OWN fp32 run against its float64 run, per term: (value, gradient) errors as the kernels' are figured."""
    g = golden()
    out = {}
    for name in golden_terms()[2]:
        v64, g64 = g[name + ".value64"].item(), torch.from_numpy(g[name + ".grad64"])
        out[name] = (abs(g[name + ".value32"].item() - v64) / abs(v64) if v64 else abs(g[name + ".value32"].item()),
                     dsr_error(torch.from_numpy(g[name + ".grad32"]), g64))
    return out


# ---- kernel level --------------------------------------------------------------------------------------------------------
def _aux(masks, kind, device):
    m = masks.to(device)
    if kind.startswith("soft"):
        return m
    region, flag = ops.mask_compress(m)
    assert int(flag.item()) == 0
    return region


def _offset_by_one_float(t, device):
    """A copy of ``t`` on the device that starts 4 bytes after a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def check_crit_kernels(device, s, unaligned=False):
    """Every (pixel, A[, B]) at scale ``s`` for K in KS, region bytes and soft masks, against the float64 truth."""
    worst = dict(sums=0.0, dsr=0.0, ref_sums=0.0, ref_dsr=0.0)
    for K in KS:
        for combo in combos():
            p, a, b = combo
            for kind in kinds_for(K, a, b):
                sr, hr, masks = make_inputs(s, K, kind)
                want_sums, want_dsr, ref_es, ref_ed = truth(s, K, kind)[combo]
                sr_d = _offset_by_one_float(sr, device) if unaligned else sr.to(device)
                hr_d, aux = hr.to(device), _aux(masks, kind, device)
                i = combos().index(combo)
                dsums = _dsums(want_sums.numel(), i).float().to(device)
                es = sums_error(ops.loss_sums_crit(sr_d, hr_d, aux, K, p, a, b), want_sums)
                ed = dsr_error(ops.loss_bwd_crit(sr_d, hr_d, aux, dsums, K, p, a, b), want_dsr)
                gs, gd = min(CAP_SUMS, 10 * max(ref_es, EPS32)), min(CAP_DSR, 10 * max(ref_ed, EPS32))
                if es > gs or ed > gd:
                    print("MISS", (s, K, kind, combo), "sums", es, "ref", ref_es, "dsr", ed, "ref", ref_ed)
                worst = dict(sums=max(worst["sums"], es), dsr=max(worst["dsr"], ed), ref_sums=max(worst["ref_sums"], ref_es),
                             ref_dsr=max(worst["ref_dsr"], ref_ed))
                assert es <= gs, ("sums", s, K, kind, combo, es, gs, ref_es)
                assert ed <= gd, ("dsr", s, K, kind, combo, ed, gd, ref_ed)
    print("crit kernels scale", s, "unaligned" if unaligned else "", worst)
    return worst


def check_crit_golden_case(device):
    """The golden case itself (scale 2, K = 10): each term's raw sums through the kernels, composed as the harness composes
    them, against the reference's float64 run - no looser than 10 x the reference's own fp32 run on that term."""
    from dasr_amd import harness
    g = golden()
    s, K, terms = golden_terms()
    ref32 = golden_fp32_errors()
    figs = {}
    for name, (kind, _) in terms.items():
        what, _, crit = name.partition(".")
        crit = crit.split(".")[-1]
        sr, hr, masks = make_inputs(s, K, kind or "onehot")
        sr_d = sr.to(device).requires_grad_(True)
        kw = dict(pixel_weight=0.0, dynamic_weight=None, pixel_criterion="l1", mask_criterion=None)
        if what == "pix":
            kw.update(pixel_weight=WEIGHTS["pixel_weight"], pixel_criterion=crit, dynamic_weight=1.0, dynamic_criterion="l1")
        elif what == "dyn":
            kw.update(dynamic_weight=WEIGHTS["dynamic_weight"], dynamic_criterion=crit)
        else:
            kw.update(mask_criterion=crit, mask_weight=WEIGHTS["mask_weight"],
                      mask_index=torch.tensor([mask_index(K)], device=device))
        m_d = masks.to(device)
        real_aux = harness._criterion_aux
        if device == "cpu":                                  # the emulator's tensors are CPU tensors: hand the kernels' input over
            harness._criterion_aux = lambda sr_, m_, kind=kind: _aux(m_, kind or "onehot", device)
        try:
            t = harness.criterion_losses(sr_d, hr.to(device), m_d, torch.ones(K, device=device), **kw)
        finally:
            harness._criterion_aux = real_aux
        assert t["fused"], name
        v = {"pix": t["l_pix"], "dyn": t["l_dyn"], "mask": t["l_mask"]}[what]
        dsr, = torch.autograd.grad(v, sr_d)
        v64 = g[name + ".value64"].item()
        ev = abs(float(v.detach()) - v64) / abs(v64) if v64 else abs(float(v.detach()))
        ed = dsr_error(dsr, torch.from_numpy(g[name + ".grad64"]))
        gv, gd = 10 * max(ref32[name][0], EPS32), 10 * max(ref32[name][1], EPS32)
        figs[name] = (ev, ed, ref32[name])
        print("golden case", name, "value", ev, "dsr", ed, "reference fp32", ref32[name])
        assert ev <= min(CAP_SUMS, gv) and ed <= min(CAP_DSR, gd), (name, ev, ed, ref32[name])
    return dict(value=max(f[0] for f in figs.values()), dsr=max(f[1] for f in figs.values()))


def check_default_bits(device):
    """(pixel l1, A smoothl1, no B), on region bytes and on soft masks: the argument-policy kernels' sums and dsr equal the
    fixed-policy kernels' bit for bit.  dsr on the general inputs; the sums on the dyadic ones, where the order in which the
    float atomics land cannot matter (two launches of the SAME kernel differ in the last bits otherwise)."""
    for s in SCALES:
        for K in KS:
            for dyadic in (False, True):
                for kind, sums_fn, bwd_fn in (("onehot", ops.loss_sums, ops.loss_bwd),
                                              ("soft", ops.loss_sums_soft, ops.loss_bwd_soft)):
                    sr, hr, masks = make_inputs(s, K, kind, dyadic)
                    sr_d, hr_d, aux = sr.to(device), hr.to(device), _aux(masks, kind, device)
                    if dyadic:
                        new, old = ops.loss_sums_crit(sr_d, hr_d, aux, K, "l1", "smoothl1"), sums_fn(sr_d, hr_d, aux, K)
                        assert torch.equal(new, old), (s, K, kind, new, old)
                        assert float(old[2 * K]) > 0 and float(old[0]) > 0
                    dsums = _dsums(2 * K + 1, 3).float().to(device)
                    new, old = ops.loss_bwd_crit(sr_d, hr_d, aux, dsums, K, "l1", "smoothl1"), bwd_fn(sr_d, hr_d, aux, dsums, K)
                    assert torch.equal(new, old), (s, K, kind, dyadic)
    return dict(ok=True)


def check_refusals(device):
    """K = 17, 'cb' as a region criterion and 'smoothl1' as the pixel criterion: DASR_E_UNSUPPORTED, for both mask forms."""
    sr, hr, _ = make_inputs(4, 16, "soft")
    sr_d, hr_d = sr.to(device), hr.to(device)
    soft17 = torch.rand(B_, 17, LR_H, LR_W).to(device)
    region = torch.zeros(B_, LR_H, LR_W, dtype=torch.uint8, device=device)
    soft16 = torch.rand(B_, 16, LR_H, LR_W).to(device)
    cases = [(soft17, 17, "l1", "l2", None), (region, 17, "l1", "l2", None), (soft16, 16, "l1", "cb", None),
             (region, 16, "l1", "l1", "cb"), (soft16, 16, "smoothl1", "l1", None), (region, 16, "smoothl1", "l1", None)]
    for aux, K, p, a, b in cases:
        for fn in (lambda: ops.loss_sums_crit(sr_d, hr_d, aux, K, p, a, b),
                   lambda: ops.loss_bwd_crit(sr_d, hr_d, aux, torch.ones((3 if b else 2) * K + 1, device=device), K, p, a, b)):
            try:
                fn()
                raised = False
            except RuntimeError as e:
                raised = "code -3" in str(e)
            assert raised, (K, p, a, b)
    return dict(ok=True)


# ---- harness level -------------------------------------------------------------------------------------------------------
def trainer_combos():
    """(pixel, dynamic or None, mask or None): all 48, the default among them."""
    return list(itertools.product(PIXEL, REGION + (None,), (None,) + REGION))


def trainer_kwargs(pixel, dyn, mask):
    kw = dict(pixel_criterion=pixel, mask_criterion=mask, mask_weight=WEIGHTS["mask_weight"])
    if dyn is None:
        kw["dynamic_weight"] = None
    else:
        kw["dynamic_criterion"] = dyn
    return kw


class SrNet(torch.nn.Module):
    """A 'generator' whose output IS its parameter: after a step ``sr.grad`` is d total / d sr."""

    def __init__(self, sr):
        super().__init__()
        self.sr = torch.nn.Parameter(sr.clone())

    def forward(self, lq, depth, masks):
        return self.sr


def check_cpu_trainer_vs_golden(device="cpu"):
    """The PyTorch-formulation Trainer on CPU tensors against criteria.npz, every combination, one-hot and soft masks: each
    logged term against the reference's float64 value and d l_all / d sr against the sum of its gradients.  The bound is
    10 x the reference's own fp32 error on the same terms (not below 10 x 2^-24)."""
    from dasr_amd import harness
    g = golden()
    s, K, _ = golden_terms()
    ref32 = golden_fp32_errors()
    worst = 0.0
    for kind in ("onehot", "soft"):
        sr, hr, masks = make_inputs(s, K, kind)
        for pixel, dyn, mask in trainer_combos():
            names = {"l_pix": "pix." + pixel}
            if dyn:
                names["l_dynamic"] = "dyn.%s.%s" % (kind, dyn)
            if mask:
                names["l_mask"] = "mask.%s.%s" % (kind, mask)
            net = SrNet(sr)
            tr = harness.Trainer(net, K, **trainer_kwargs(pixel, dyn, mask))
            np.random.seed(MASK_SEED)
            log = tr.optimize_parameters(None, hr, None, masks)
            assert sorted(log) == sorted(list(names) + ["l_all"]), (sorted(log), names)
            assert (tr.mask_region == mask_index(K)) if mask else tr.mask_region is None
            total = 0.0
            for key, name in names.items():
                v64 = g[name + ".value64"].item()
                total += v64
                e = abs(float(log[key]) - v64) / abs(v64)
                worst = max(worst, e)
                assert e <= 10 * max(ref32[name][0], EPS32), (kind, pixel, dyn, mask, key, e, ref32[name])
            assert abs(float(log["l_all"]) - total) <= 1e-5 * abs(total)
            want = sum(torch.from_numpy(g[name + ".grad64"]) for name in names.values())
            bound = 10 * max(max(ref32[name][1] for name in names.values()), EPS32)
            e = dsr_error(net.sr.grad, want)
            worst = max(worst, e)
            assert e <= bound, (kind, pixel, dyn, mask, "dsr", e, bound)
            assert (tr.dynamic_loss is None) == (dyn is None)
            assert len(tr.params) == (1 if dyn is None else 2)
    return dict(worst=worst)


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
def _torch_criteria(on=True):
    from dasr_amd import harness
    harness.Trainer.force_torch_criteria = on
    try:
        yield
    finally:
        harness.Trainer.force_torch_criteria = False


X4_CASE = dict(name="x4_nb4", scale=4, which=[0, 1], L=32, nb=4, B=1, H=12, W=16)       # golden_cases.CASES
GATED = ("conv_output.", "upscale")          # the HR tail, behind the loss on the main stream (as ssim_loss_checks gates)


def _tiny_net(device):
    from tests.test_dp_gloo import _TinyNet
    return _TinyNet().to(device)


def _step_pair(device, make_net, batch, kw, keys):
    """One step through the fused path and one through the forced PyTorch formulation, from identical parameters and the
    same drawn region: the largest relative difference of a logged term, and the relative L2 differences of the UPDATE and
    of the gradients of the parameters under ``keys`` (the first Adam update alone does not see a gradient's scale)."""
    from dasr_amd import harness
    runs = []
    for forced in (False, True):
        net = make_net()
        init = {k: v.detach().clone() for k, v in net.state_dict().items()}
        tr = harness.Trainer(net, **kw)
        fused_expected = not forced and (tr.dynamic_loss is not None or tr.mask_criterion is not None)
        np.random.seed(MASK_SEED)
        with _torch_criteria(forced), _counting(ops, "loss_sums_crit") as nf, _counting(ops, "loss_bwd_crit") as nb, \
                _counting(ops, "loss_sums") as n_old:
            log = tr.optimize_parameters(*batch)
        assert (nf[0], nb[0], n_old[0]) == ((1, 1, 0) if fused_expected else (0, 0, 0)), (kw, forced, nf, nb, n_old)
        mine = lambda k: k.startswith(keys) and not any(z in k for z in ZERO_GRAD_KEYS)
        grads = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters() if mine(k) and p.grad is not None}
        upd = {k: (v.detach() - init[k]).double().cpu() for k, v in net.state_dict().items() if k in grads}
        runs.append(({k: float(v) for k, v in log.items()}, upd, grads))
    (la, ua, ga), (lb, ub, gb) = runs
    assert sorted(la) == sorted(lb) and all(math.isfinite(v) for v in la.values()), (la, lb)
    assert sorted(ga) == sorted(gb) == sorted(ub) and gb
    e_log = max(abs(la[k] - lb[k]) / max(1.0, abs(lb[k])) for k in lb)
    return e_log, _rel_l2(ua, ub, _well_conditioned(gb)), _rel_l2(ga, gb), la


ADAM_FLOOR = 1e-3


def _well_conditioned(grads):
    """The entries on which a first Adam update can be compared at all.  The update is lr * g / (|g| + 1e-8): an entry whose
    gradient is rounding noise around 0 takes +lr or -lr at random in ANY two fp32 evaluations of the same step (measured on
    the MI355X: update rel-L2 of 0.14 between the fused path and the PyTorch formulation whose gradients agree to 7e-8).  So
    the updates are compared where |g| >= ADAM_FLOOR x the tensor's largest |g| (and >= 1e-5, far above Adam's eps); the
    gradients themselves are compared on every entry."""
    return {k: (g.abs() >= max(ADAM_FLOOR * g.abs().max().item(), 1e-5)) for k, g in grads.items()}


def _rel_l2(a, b, where=None):
    pick = (lambda k, t: t[where[k]]) if where is not None else (lambda k, t: t)
    num = sum(pick(k, a[k] - b[k]).pow(2).sum().item() for k in b)
    den = sum(pick(k, b[k]).pow(2).sum().item() for k in b)
    assert den > 0
    return math.sqrt(num / den)


def check_trainer_combos(device, net_name, pixel):
    """Every non-default combination with this pixel criterion, fused against the forced PyTorch formulation."""
    if net_name == "tiny":                       # soft masks (the float-mask kernels); the HIP DepthNet below: region bytes
        lq, gt, dm, mk = synth.seeded_batch(0, 2, 8, 10, 8)
        mk = (0.7 * mk + 0.3 * torch.rand(mk.shape, generator=torch.Generator().manual_seed(3))).contiguous()
        batch = tuple(t.to(device) for t in (lq, gt, dm, mk))
        make_net, keys = (lambda: _tiny_net(device)), ("conv.",)
    else:
        c = X4_CASE
        batch = tuple(t.to(device) for t in synth.seeded_batch(0, c["B"], c["H"], c["W"], c["scale"]))
        net0, _ = build_net(c, device)
        state = {k: v.detach().clone() for k, v in net0.state_dict().items()}

        def make_net():
            net0.load_state_dict(state)
            return net0
        keys = GATED
    worst = [0.0, 0.0, 0.0]
    for _, dyn, mask in [c for c in trainer_combos() if c[0] == pixel]:
        if (pixel, dyn, mask) == ("l1", "smoothl1", None):
            continue
        kw = trainer_kwargs(pixel, dyn, mask)
        e_log, e_upd, e_grad, log = _step_pair(device, make_net, batch, kw, keys)
        print("trainer", net_name, (pixel, dyn, mask), "log", e_log, "update rel L2", e_upd, "grad rel L2", e_grad, log)
        worst = [max(worst[0], e_log), max(worst[1], e_upd), max(worst[2], e_grad)]
        assert max(e_log, e_upd, e_grad) <= CAP_STEP, (net_name, pixel, dyn, mask, e_log, e_upd, e_grad)
    return dict(log=worst[0], update=worst[1], grad=worst[2])


def check_default_unchanged(device):
    """Trainer(net) and Trainer(net, **networks.criteria({})): the same launches (the existing loss kernels, never the new
    family), the same log keys and optimizer layout, and after two steps bit-identical parameters and loss weights on the
    CPU.  On the GPU the existing step is not bit-reproducible against ITSELF: dasr_loss_sums adds with float atomics, their
    order reaches the loss weights' gradient through num / den, and the second step reads those weights (two default
    Trainers, and a default one against the criteria({}) one - the same code - each came out with differing last bits on
    the MI355X).  An Adam step moves a value by at most lr, and a relative gradient noise of 1e-6 moves that by 1e-9, far
    below a unit in the last place, so all the noise can do is tip a rounding: at most one unit per step.  There the gate
    is therefore 2 units in the last place of each tensor's largest magnitude."""
    from dasr_amd import harness, networks
    assert networks.criteria({}) == dict(pixel_criterion="l1", pixel_weight=1.0, dynamic_criterion="smoothl1",
                                         dynamic_weight=10.0, mask_criterion=None, mask_weight=1.0)
    outs = []
    for kw in ({}, networks.criteria({})):
        net = _tiny_net(device)
        tr = harness.Trainer(net, 10, **kw)
        assert tr._default_criteria and tr._mask_idx is None
        with _counting(ops, "loss_sums_crit") as n_new, _counting(ops, "loss_sums") as n_old:
            logs = [tr.optimize_parameters(*(t.to(device) for t in synth.seeded_batch(4 * i, 2, 8, 10, 8))) for i in range(2)]
        assert n_new[0] == 0 and n_old[0] == (2 if device == "cuda" else 0), (n_new, n_old)
        assert sorted(logs[-1]) == ["l_all", "l_dynamic", "l_pix"]
        assert sorted(tr.optimizer.state_dict()["param_groups"][0]["params"]) == list(range(len(tr.params)))
        tensors = dict(net.state_dict(), loss_w=tr.dynamic_loss.trainable_weight)
        outs.append(({k: v.detach().clone() for k, v in tensors.items()}, sorted(tr.optimizer.state_dict()["state"])))
    (a, sa), (b, sb) = outs
    assert sa == sb and sorted(a) == sorted(b)
    differ = {}
    for k in a:
        if not torch.equal(a[k], b[k]):
            differ[k] = (a[k] - b[k]).abs().max().item() / a[k].abs().max().item()
    print("default Trainer against Trainer(**criteria({})): tensors with differing bits", differ)
    assert all(v <= 2 * 2.0 ** -23 for v in differ.values()) and (device == "cuda" or not differ), differ
    return dict(differ=differ)


def check_graphed_static_mask(device):
    """use_graph with the static mask loss on: three eager steps, the capture and two replays whose drawn regions DIFFER; each
    graphed step's log must equal an eager step from the same parameters with that region - the device-side index is live."""
    from dasr_amd import harness
    from tests.soft_loss_checks import TRAINER_CASE
    K = 10
    seed = next(sd for sd in range(100) if len(set(_draws(sd, 6, K)[3:])) == 3)      # capture and both replays: 3 regions
    draws = _draws(seed, 6, K)
    kw = dict(mask_criterion="l1", mask_weight=50.0, dynamic_criterion="l2")
    net, _ = build_net(TRAINER_CASE, device)
    tr = harness.Trainer(net, use_graph=True, **kw)
    net2, _ = build_net(TRAINER_CASE, device)
    np.random.seed(seed)
    figs = []
    for step in range(6):
        batch = tuple(t.to(device) for t in synth.seeded_batch(10 * step, 2, 16, 20, 8))
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        w_before = tr.dynamic_loss.trainable_weight.detach().clone()
        log = {k: float(v) for k, v in tr.optimize_parameters(*batch).items()}
        assert tr.mask_region == draws[step], (step, tr.mask_region, draws)
        if step < 3:
            continue
        assert tr._graph is not None
        # the eager step from the same parameters with the same region (the generator state is kept out of its draw)
        net2.load_state_dict(before)
        tr2 = harness.Trainer(net2, **kw)
        with torch.no_grad():
            tr2.dynamic_loss.trainable_weight.copy_(w_before)
        state = np.random.get_state()
        np.random.seed(seed)
        for _ in range(step):
            np.random.randint(0, K, 1)
        want = {k: float(v) for k, v in tr2.optimize_parameters(*batch).items()}
        np.random.set_state(state)
        assert tr2.mask_region == draws[step]
        e = max(abs(log[k] - want[k]) / max(1.0, abs(want[k])) for k in want)
        figs.append((draws[step], log["l_mask"], want["l_mask"], e))
        assert sorted(log) == ["l_all", "l_dynamic", "l_mask", "l_pix"] and e <= CAP_STEP, (step, log, want)
    print("graphed static mask: (region, l_mask graphed, l_mask eager, worst log difference)", figs)
    assert figs[1][0] != figs[2][0] and abs(figs[1][1] - figs[2][1]) > 100 * CAP_STEP * max(1.0, abs(figs[1][1])), figs
    return dict(figs=figs)


def _draws(seed, n, K):
    rs = np.random.RandomState(seed)
    return [int(rs.randint(0, K, 1)[0]) for _ in range(n)]


def check_trainer_ssim_l2(device):
    """The SSIM criterion stays on alongside pixel l2 / dynamic l2: one node (its backward adds into the criteria's dsr),
    against the same step with both forced to their PyTorch formulations."""
    from dasr_amd import harness
    from tests.soft_loss_checks import TRAINER_CASE
    runs = []
    for forced in (False, True):
        net, _ = build_net(TRAINER_CASE, device)
        init = {k: v.detach().clone() for k, v in net.state_dict().items()}
        tr = harness.Trainer(net, ssim_weight=-0.5, pixel_criterion="l2", dynamic_criterion="l2")
        harness.SSIMLoss.force_torch = forced
        try:
            with _torch_criteria(forced), _counting(ops, "ssim_bwd") as ns, _counting(ops, "loss_bwd_crit") as nb:
                log = tr.optimize_parameters(*(t.to(device) for t in synth.seeded_batch(0, 2, 16, 20, 8)))
            assert (ns[0], nb[0]) == ((0, 0) if forced else (1, 1)), (forced, ns, nb)
        finally:
            harness.SSIMLoss.force_torch = False
        mine = lambda k: k.startswith(GATED) and not any(z in k for z in ZERO_GRAD_KEYS)
        grads = {k: p.grad.detach().double().cpu() for k, p in net.named_parameters() if mine(k) and p.grad is not None}
        upd = {k: (v.detach() - init[k]).double().cpu() for k, v in net.state_dict().items() if k in grads}
        runs.append(({k: float(v) for k, v in log.items()}, upd, grads))
    (la, ua, ga), (lb, ub, gb) = runs
    assert sorted(la) == ["l_all", "l_dynamic", "l_pix", "l_ssim"] and -0.5 <= la["l_ssim"] < 0, la
    assert sorted(ga) == sorted(gb) == sorted(ub)
    e_log = max(abs(la[k] - lb[k]) / max(1.0, abs(lb[k])) for k in lb)
    e_upd, e_grad = _rel_l2(ua, ub, _well_conditioned(gb)), _rel_l2(ga, gb)
    print("trainer ssim + l2 / l2:", la, lb, "log", e_log, "update rel L2", e_upd, "grad rel L2", e_grad)
    assert max(e_log, e_upd, e_grad) <= CAP_STEP, (e_log, e_upd, e_grad)
    return dict(log=e_log, update=e_upd, grad=e_grad)


def check_crit_collective(device):
    """The packed collective with a pretended world of 2 (the pattern of ssim_loss_checks.check_fused_ssim_collective): the
    one-rank all-reduce returns this rank's vector, so every GLOBAL value must be that vector's entry over 2 - the l2 dynamic
    term's mean, the pixel value, S - while the gradient carriers and the rank-local static mask term stay the single-rank
    ones ('cb': world x the local sum)."""
    import torch.distributed as dist
    from dasr_amd import harness
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29574")
    own = not dist.is_initialized()
    if own and device == "cuda":
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    elif own:
        dist.init_process_group("gloo", rank=0, world_size=1)
    real_world = harness._world
    try:
        K = 10
        h, w = (16, 20) if device == "cuda" else (8, 10)      # (the CPU run goes through the PyTorch formulations)
        lq, gt, dm, mk = (t.to(device) for t in synth.seeded_batch(0, 2, h, w, 8))
        noise = synth.hash_uniform(gt.numel(), "crit.dp").reshape(gt.shape).float().to(device)
        w = (1.0 + 0.1 * torch.arange(K, dtype=torch.float32)).to(device)
        idx = torch.tensor([3], device=device)
        res = {}
        for pixel in ("l2", "cb"):
            for world in (1, 2):
                harness._world = (lambda group=None: 2) if world == 2 else real_world
                sr = (gt + 0.1 * (noise - 0.5)).clamp(0, 1).requires_grad_(True)
                t = harness.criterion_losses(sr, gt, mk.clone(), w, 1.0, 10.0, pixel, "l2", "smoothl1", 0.7, idx,
                                             dist.group.WORLD if world == 2 else None, harness.SSIMLoss())
                harness._world = real_world
                assert t["fused"] == (device == "cuda")
                d_dyn, = torch.autograd.grad(t["l_dyn"], sr, retain_graph=True)
                d_pix, = torch.autograd.grad(t["l_pix"], sr, retain_graph=True)
                res[world] = dict(t, d_dyn=d_dyn, d_pix=d_pix)
            a, b = res[1], res[2]
            rel = lambda x, y: abs(float(x.detach()) - float(y.detach())) / max(1e-30, abs(float(y.detach())))
            assert rel(b["l_pix_log"], a["l_pix_log"] if pixel == "cb" else a["l_pix_log"] / 2) <= 2e-6, pixel
            assert rel(b["l_pix"], 2 * a["l_pix"] if pixel == "cb" else a["l_pix"]) <= 2e-6, pixel
            assert rel(b["l_dyn"], a["l_dyn"] / 2) <= 2e-6 and rel(b["S_log"], a["S_log"] / 2) <= 2e-6
            assert rel(b["l_mask"], a["l_mask"]) <= 2e-6 and float(a["l_mask"]) > 0
            assert torch.equal(a["d_dyn"], b["d_dyn"])               # the local mean's gradient, whatever the world
            assert dsr_error(b["d_pix"], (2 if pixel == "cb" else 1) * a["d_pix"].cpu()) <= 1e-6
        return dict(ok=True)
    finally:
        harness._world = real_world
        if own:
            dist.destroy_process_group()
