"""Training / test harness around DepthNet — the counterpart of the reference's model wrapper.

Reproduces what ``F_Model_depthCond`` does for the shipped ymls
(codes/models/F_model_depthCond.py:87-122,146-192,228-234; codes/train.py:179-199):
L1 pixel loss (weight 1) + dynamic depth-aware smooth-L1 loss (weight 10, 10 trainable region
weights, codes/models/modules/mask_loss.py:44-90), Adam(lr 1e-3, betas (0.9, 0.99), wd 0) over the
generator's parameters plus the loss weights, CosineAnnealingLR_Restart stepped BEFORE the optimiser
(codes/models/lr_scheduler.py:34-62).  Losses and optimiser stay PyTorch (north_star); the generator
forward/backward is the HIP path, and so are the sums every loss term needs: ONE autograd node (``_LossSums``: one pass over
sr / hr forward, one backward, for one-hot masks and for soft masks alike), ONE rule for when the kernels take the tensors
(``_criterion_aux``) and ONE piece of arithmetic after the sums (``_compose_losses``: the division, the softmax weighting and
the collective stay in PyTorch).  The criteria a reference yml can name - ``pixel_criterion`` l1 / l2 / cb,
``dynamic_criterion`` l1 / l2 / smoothl1, the dynamic term off, the static ``mask_loss`` - are ``Trainer`` arguments
(``networks.criteria(opt)``).  The default combination (pixel l1, dynamic smooth-L1, no static mask) runs the kernels that
have it compiled in (``dasr_loss_{sums,bwd}[_soft]``, through ``fused_losses``), any other the same kernels with the criteria
as arguments (``dasr_loss_{sums,bwd}[_soft]_crit``, through ``criterion_losses``).  The reference's optional SSIM criterion
(``Trainer(ssim_weight=...)``, off by default as in the shipped ymls) is ``SSIMLoss``: ``dasr_ssim`` forward, ``dasr_ssim_bwd``
backward, in the same autograd node and collective when its kernels take the tensors.

Data parallel: one process per GPU (torchrun), ``torch.distributed`` backend ``nccl`` (= RCCL over
xGMI) on the GPU box, ``gloo`` in CPU tests.  The net itself is communication-free (instance norm is
per-sample).  Per step: ONE small all-reduce of the packed loss scalars (K numerators | K denominators |
sum|sr-hr|: the dynamic loss is then the GLOBAL ratio the reference's default nn.DataParallel path computes
on GPU0, SURVEY.md §8e, and the logged L1 is the global-batch value), and the gradient all-reduce (14.8 M
fp32 = 59 MB for the x8 net, plus the 10 loss weights) in FOUR flat buckets issued asynchronously from the
backward tape as each bucket's gradients complete (HR tail, later LR blocks, earlier LR blocks, then encoder /
head / depth branch / loss weights), waited for once before ``optimizer.step()``.
"""
import math

import torch
import torch.nn.functional as F


def cosine_restart_lr(step, base_lr=1e-3, T_period=(20000, 20000, 20000, 20000),
                      restarts=(20000, 40000, 60000), weights=(1, 1, 1), eta_min=1e-7):
    """Learning rate after ``step`` calls of CosineAnnealingLR_Restart.step()
    (closed form of the recursion in codes/models/lr_scheduler.py:46-62)."""
    last_restart, T, w = 0, T_period[0], 1.0
    for j, r in enumerate(restarts):
        if step >= r:
            last_restart, T, w = r, T_period[j + 1], weights[j]
    return eta_min + (base_lr * w - eta_min) * (1 + math.cos(math.pi * (step - last_restart) / T)) / 2


def _world(group=None):
    """Number of data-parallel ranks: derived from torch.distributed itself, so that a caller who passes no group
    while a process group is initialised still gets the GLOBAL dynamic-loss ratio (group None == the WORLD group)."""
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_world_size(group)
    return 1


def ssim_torch(img1, img2):
    """The PyTorch formulation of the reference's ``SSIM()`` criterion (models/modules/ssim_loss.py:7-37, size_average=True):
    the 2-D window g g^T formed in fp32, five grouped convolutions, the SSIM map and its mean.  What ``SSIMLoss`` computes
    for tensors the HIP kernels do not take (CPU, other dtypes, other layouts)."""
    from .validate import _window_1d
    g = _window_1d().unsqueeze(1)
    ch = img1.shape[1]
    window = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(ch, 1, 11, 11).contiguous().to(img1.device).type_as(img1)
    mu1 = F.conv2d(img1, window, padding=5, groups=ch)
    mu2 = F.conv2d(img2, window, padding=5, groups=ch)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=5, groups=ch) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=5, groups=ch) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=5, groups=ch) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))).mean()


def _dscale(dS):
    """dL/dS as the one-element device tensor dasr_ssim_bwd reads (no host read-back)."""
    return dS.reshape(1).to(torch.float32).contiguous()


class _SSIM(torch.autograd.Function):
    """S = mean of the SSIM map (dasr_ssim; nothing saved but the two images); backward: dasr_ssim_bwd, one launch.
    Gradient to the first image only."""

    @staticmethod
    def forward(ctx, img1, img2):
        from . import ops
        ctx.save_for_backward(img1, img2)
        return ops.ssim(img1, img2).mean()

    @staticmethod
    def backward(ctx, dS):
        from . import ops
        img1, img2 = ctx.saved_tensors
        return ops.ssim_bwd(img1, img2, _dscale(dS)), None


class _LossSums(torch.autograd.Function):
    """sums = (K numerators of criterion A | K areas | pixel-criterion sum [| K numerators of criterion B]) in ONE pass over
    sr, hr, and one elementwise backward.  ``aux``: region bytes (uint8, from dasr_mask_compress) or float masks [B,K,h,w] -
    the mask then sits inside the criterion, so every pixel feeds all K numerators; K <= 16; no gradient to the masks.
    ``crits``: None - the default criteria (pixel l1, region smooth-L1, no B) through the kernels that have them compiled in
    (ops.loss_sums / loss_bwd, ops.loss_sums_soft / loss_bwd_soft); a tuple (pixel, A, B or None) - the criteria as kernel
    arguments (ops.loss_sums_crit / loss_bwd_crit), the default ones included.
    ``with_ssim``: a second output, the SSIM criterion of (sr, hr) - the 9x9 dgrad takes dL/dsr as one tensor, so the SSIM
    backward adds into the dsr the loss backward has just written (dasr_ssim_bwd, accumulate) instead of autograd adding two
    HR-sized tensors in a pass of its own."""

    @staticmethod
    def _ops(aux, crits):
        """(sums op, backward op, trailing arguments), looked up on ``ops`` at call time."""
        from . import ops
        if crits is not None:
            return ops.loss_sums_crit, ops.loss_bwd_crit, crits
        if aux.dtype == torch.uint8:
            return ops.loss_sums, ops.loss_bwd, ()
        return ops.loss_sums_soft, ops.loss_bwd_soft, ()

    @staticmethod
    def forward(ctx, sr, hr, aux, K, crits, with_ssim):
        from . import ops
        sr_c, hr_c = sr.contiguous(), hr.contiguous()
        if aux.dtype != torch.uint8:
            aux = aux.detach().contiguous()
        ctx.save_for_backward(sr_c, hr_c, aux)
        ctx.K, ctx.crits, ctx.with_ssim = K, crits, with_ssim
        sums_op, _, tail = _LossSums._ops(aux, crits)
        sums = sums_op(sr_c, hr_c, aux, K, *tail)
        if with_ssim:
            return sums, ops.ssim(sr_c, hr_c).mean()
        return sums

    @staticmethod
    def backward(ctx, dsums, dS=None):
        from . import ops
        sr, hr, aux = ctx.saved_tensors
        _, bwd_op, tail = _LossSums._ops(aux, ctx.crits)
        dsr = bwd_op(sr, hr, aux, dsums.contiguous(), ctx.K, *tail)
        if ctx.with_ssim:
            ops.ssim_bwd(sr, hr, _dscale(dS), out=dsr, accumulate=True)
        return dsr, None, None, None, None, None


class SSIMLoss(torch.nn.Module):
    """The reference's ``SSIM()`` criterion (models/modules/ssim_loss.py:39-63, ``size_average=True``): the mean of the SSIM
    map of two [B,C,H,W] images, 11 x 11 Gaussian windows.  fp32 contiguous CUDA tensors go through the HIP kernels
    (dasr_ssim forward, dasr_ssim_bwd backward: one launch each, nothing saved between them); anything else through the
    PyTorch formulation (``ssim_torch``).  The gradient goes to the FIRST image only: a second image that requires a
    gradient is refused."""

    force_torch = False          # tests: compare the kernels against the PyTorch formulation on the same tensors

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        if window_size != 11 or not size_average:
            raise NotImplementedError("SSIMLoss: the reference's configuration only (11 x 11 window, size_average=True)")

    @classmethod
    def hip_ok(cls, img1, img2):
        if cls.force_torch or img1.dim() != 4 or img1.shape != img2.shape or img1.shape[0] * img1.shape[1] > 65535:
            return False
        return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (img1, img2))

    def forward(self, img1, img2):
        if img2.requires_grad:
            raise ValueError("SSIMLoss: the second image must not require a gradient (the criterion differentiates "
                             "with respect to the first image only)")
        if self.hip_ok(img1, img2):
            return _SSIM.apply(img1, img2)
        return ssim_torch(img1, img2)


PIXEL_CRITERIA = ("l1", "l2", "cb")               # train.pixel_criterion (F_model_depthCond.py:50-58)
REGION_CRITERIA = ("l1", "l2", "smoothl1")        # dynamic_loss.dynamic_criterion / mask_loss.mask_criterion (mask_loss.py)
CB_EPS = 1e-6                                     # CharbonnierLoss(eps) (loss.py:40)


def check_criteria(pixel_criterion, dynamic_criterion, mask_criterion):
    """The reference's own refusals: an unknown name is NotImplementedError there too, and 'cb' as a REGION criterion dies
    with a NameError (mask_loss.py never imports CharbonnierLoss), so it is refused here with the reason."""
    if pixel_criterion not in PIXEL_CRITERIA:
        raise NotImplementedError("Loss type [%s] is not recognized." % (pixel_criterion,))
    for what, c in (("dynamic_criterion", dynamic_criterion), ("mask_criterion", mask_criterion)):
        if c == "cb":
            raise NotImplementedError("%s='cb': the reference's mask_loss.py names CharbonnierLoss without importing it "
                                      "(a NameError there), so there is no behaviour to reproduce; use l1, l2 or smoothl1"
                                      % what)
        if c is not None and c not in REGION_CRITERIA:
            raise NotImplementedError("Loss type [%s] for depth loss is not recognized." % (c,))


def _pixel_sum(d, pixel_criterion):
    if pixel_criterion == "l1":
        return d.abs().sum()
    if pixel_criterion == "l2":
        return (d * d).sum()
    return torch.sqrt(d * d + CB_EPS).sum()


def _region_sum(u, criterion):
    if criterion == "l1":
        return u.abs().sum()
    if criterion == "l2":
        return (u * u).sum()
    return F.smooth_l1_loss(u, torch.zeros_like(u), reduction="sum")


def criterion_sums_torch(sr, hr, mask_list, pixel_criterion, crit_a, crit_b=None):
    """The PyTorch formulation of what the ``_crit`` kernels sum, in their layout (K numerators of A | K areas | pixel sum
    [| K numerators of B]) and differentiable by autograd (the masks included): one masked pass per region, as the reference
    makes them.  ``crit_a`` None: the pixel sum alone."""
    d = sr - hr
    px = _pixel_sum(d, pixel_criterion).reshape(1)
    if crit_a is None:
        return px
    na, area, nb = [], [], []
    for k in range(mask_list.shape[1]):
        m = F.interpolate(mask_list[:, k:k + 1], size=sr.shape[2:], mode="nearest")
        u = m * d
        na.append(_region_sum(u, crit_a))
        area.append(float(sr.shape[1]) * m.sum())
        if crit_b is not None:
            nb.append(_region_sum(u, crit_b))
    return torch.cat([torch.stack(na), torch.stack(area), px] + ([torch.stack(nb)] if crit_b is not None else []))


def _criterion_aux(sr, mask_list):
    """THE rule for when the loss kernels take a step's tensors.  What they read beside sr / hr - region bytes for one-hot
    masks, the masks themselves when they are soft (contiguous fp32 CUDA masks that need no gradient) - or None: CPU
    tensors, other dtypes, HR / LR sizes that are no integer scale, masks that need a gradient, and every mask tensor of more
    than 16 regions, one-hot or not (checked before the masks are classified: dasr_mask_compress takes no more either).  On
    None the caller uses the PyTorch formulation."""
    from . import graph, ops, prep
    if not sr.is_cuda or sr.dtype != torch.float32 or mask_list.shape[2] == 0:
        return None
    H, W = sr.shape[2:]
    h, w = mask_list.shape[2:]
    if H % h or W % w or H // h != W // w or mask_list.shape[1] > ops.LOSS_MAX_REGIONS:
        return None
    if prep.attach_region(mask_list):         # no-op for masks from prep.depth_to_masks / already classified
        return graph.attached_region(mask_list)
    if mask_list.is_cuda and mask_list.dtype == torch.float32 and mask_list.is_contiguous() and not mask_list.requires_grad:
        return mask_list
    return None


def _compose_losses(sums, S, N, K, crits, trainable_weight, pixel_weight, dynamic_weight, mask_criterion, mask_weight,
                    mask_index, group):
    """Everything after the sums, for every combination of criteria: ``sums`` in the kernels' layout for ``crits`` = (pixel,
    A, B or None) with its gradient, ``S`` the SSIM value or None, ``N = sr.numel()``.  ``dynamic_weight`` None: no dynamic
    term (A is then the static mask term's criterion); ``mask_criterion`` None: no static mask term.  More than one rank:
    ONE collective carries every sum (and S); see ``criterion_losses`` for what is global and what stays local.  Returns the
    dict of ``criterion_losses`` without 'fused', and the softmax of the trainable weights (None without a dynamic term)."""
    pixel_criterion, crit_a, crit_b = crits
    world = _world(group)
    g = sums.detach()
    S_log = None if S is None else S.detach()
    if world > 1:
        g = torch.cat([g, S_log.reshape(1)]) if S is not None else g.clone()
        torch.distributed.all_reduce(g, group=group)
        if S is not None:
            S_log = g[-1] / world
    px = sums[2 * K]
    l_pix = pixel_weight * px * world if pixel_criterion == "cb" else pixel_weight * px / N
    if world > 1:
        l_pix_log = pixel_weight * g[2 * K] if pixel_criterion == "cb" else pixel_weight * g[2 * K] / (N * world)
    else:
        l_pix_log = l_pix.detach()
    den, gden = sums[K:2 * K].detach(), g[K:2 * K]

    def per_region(num, gnum, criterion, local_only):
        if criterion == "smoothl1":
            if world > 1 and not local_only:
                # value = global ratio; gradient: this rank's numerator over the global denominator, times world so that
                # the later gradient AVERAGE over ranks equals the gradient of the global loss
                local = num / gden * world
                return gnum / gden + (local - local.detach())
            return num / den
        if world > 1 and not local_only:
            local = num / N
            return gnum / (N * world) + (local - local.detach())
        return num / N

    out = dict(l_pix=l_pix, l_pix_log=l_pix_log, l_dyn=None, l_mask=None, per=None, S=S, S_log=S_log)
    sm = None
    if dynamic_weight is not None:
        assert K == trainable_weight.numel(), "dynamic loss: %d trainable region weights but %d mask channels" % (trainable_weight.numel(), K)
        out["per"] = per = per_region(sums[:K], g[:K], crit_a, False)
        sm = F.softmax(trainable_weight, dim=0)
        out["l_dyn"] = (sm * per).sum() * dynamic_weight
    if mask_criterion is not None:
        lo = 2 * K + 1 if crit_b is not None else 0
        per_m = per_region(sums[lo:lo + K], None, mask_criterion, True)
        out["l_mask"] = mask_weight * per_m.index_select(0, mask_index).squeeze(0)
    return out, sm


def fused_losses(sr, hr, mask_list, trainable_weight, pixel_weight, dynamic_weight, group=None, with_ssim=False):
    """The default combination's l_pix and l_dynamic from one pass over (sr, hr) on the GPU, through the kernels that have
    its criteria compiled in: the region-byte kernels when the masks are one-hot, the soft-mask kernels when they are not,
    or None where ``_criterion_aux`` gives None (the caller then uses the PyTorch formulation).  Same values and gradients
    as nn.L1Loss + dynamic_weight_mask_loss('smoothl1'); with a process group the region sums are made global first.
    ``with_ssim`` (the caller has checked ``SSIMLoss.hip_ok(sr, hr)``): the SSIM criterion of (sr, hr) rides along - in
    the same autograd node, and its value in the same collective - and the result has two more entries: S with its
    gradient, and its detached global value (the mean of the ranks' means: every rank's batch has the same size).
    Returns ``(l_pix, l_dyn, per, softmax(trainable_weight), global l_pix[, S, global S])``."""
    aux = _criterion_aux(sr, mask_list)
    if aux is None:
        return None
    K = mask_list.shape[1]
    sums = _LossSums.apply(sr, hr, aux, K, None, with_ssim)
    sums, S = sums if with_ssim else (sums, None)
    t, sm = _compose_losses(sums, S, sr.numel(), K, ("l1", "smoothl1", None), trainable_weight, pixel_weight,
                            dynamic_weight, None, None, None, group)
    out = (t["l_pix"], t["l_dyn"], t["per"], sm, t["l_pix_log"])
    return out + (S, t["S_log"]) if with_ssim else out


def criterion_losses(sr, hr, mask_list, trainable_weight, pixel_weight=1.0, dynamic_weight=10.0, pixel_criterion="l1",
                     dynamic_criterion="smoothl1", mask_criterion=None, mask_weight=1.0, mask_index=None, group=None,
                     ssim=None, force_torch=False):
    """The loss terms of a step for ANY combination of the reference's criteria, through the kernels that take the criteria
    as arguments (the default combination's own step goes through ``fused_losses``: the same loops with its criteria compiled
    in, the same arithmetic after them).  Values follow the reference, oddities included:

    * pixel: 'l1' / 'l2' are means over all elements, 'cb' is the SUM of sqrt(d^2 + 1e-6) (loss.py:46), each times
      ``pixel_weight``;
    * a region criterion 'smoothl1' is the ratio sum smooth_l1(M_k d) / (C sum M_k); 'l1' / 'l2' are nn.L1Loss / nn.MSELoss
      of the masked images, i.e. the mean over ALL B*C*H*W elements of |M_k d| or (M_k d)^2 - not a ratio to the area;
    * dynamic term (``dynamic_weight`` None: off): ``dynamic_weight * sum_k softmax(trainable_weight)_k per_k``;
    * static mask term (``mask_criterion`` None: off): ``mask_weight * per_k`` of the ONE region ``mask_index`` names (a
      device int64 tensor of one element, picked on the device: no host read-back), taken from the K sums the pass produced
      anyway; a second set of sums is computed only when ``mask_criterion != dynamic_criterion``.

    Fused path (one ``_crit`` pass forward, one backward; the SSIM criterion ``ssim`` rides in the node when its kernels take
    the tensors) under the rule of ``_criterion_aux``; otherwise - and with ``force_torch`` - ``criterion_sums_torch``.  With
    both region terms off the pixel criterion is one PyTorch expression and no kernel runs.

    More than one rank: ONE collective carries every sum (and S).  The logged pixel value is the global batch's; 'smoothl1'
    in the dynamic term is the global ratio as in ``fused_losses``; 'l1' / 'l2' there need no denominators - the value is the
    global mean, the gradient the local mean, which the gradient average over ranks makes global.  'cb' being a sum, its
    gradient carrier is ``world *`` the local sum for the same reason.  The static mask term stays RANK-LOCAL: the
    reference's ranks each draw their own region, so there is no global quantity to form.

    Returns a dict: ``l_pix`` (with gradient), ``l_pix_log`` (global value), ``l_dyn`` / ``l_mask`` (None when off),
    ``S`` / ``S_log`` (None without ``ssim``), ``per`` (the dynamic term's K values or None), ``fused`` (bool)."""
    check_criteria(pixel_criterion, dynamic_criterion, mask_criterion)
    dyn_on, mask_on = dynamic_weight is not None, mask_criterion is not None
    crit_a = dynamic_criterion if dyn_on else mask_criterion
    crit_b = mask_criterion if dyn_on and mask_on and mask_criterion != dynamic_criterion else None
    crits = (pixel_criterion, crit_a, crit_b)
    K = mask_list.shape[1] if crit_a is not None else 0
    S = None
    aux = None if force_torch or crit_a is None else _criterion_aux(sr, mask_list)
    if aux is not None:
        with_ssim = ssim is not None and ssim.hip_ok(sr, hr)
        sums = _LossSums.apply(sr, hr, aux, K, crits, with_ssim)
        sums, S = sums if with_ssim else (sums, None)
    else:
        sums = criterion_sums_torch(sr, hr, mask_list, *crits)
    if ssim is not None and S is None:
        S = ssim(sr, hr)
    out, _ = _compose_losses(sums, S, sr.numel(), K, crits, trainable_weight, pixel_weight, dynamic_weight, mask_criterion,
                             mask_weight, mask_index, group)
    out["fused"] = aux is not None
    return out


class DynamicMaskLoss(torch.nn.Module):
    """dynamic_weight_mask_loss with the 'smoothl1' criterion (mask_loss.py:44-90).

    ``smooth_l1(m*sr, m*hr)`` only sees the difference ``m*(sr-hr)``, so each region costs one masked
    pass over ``sr-hr``.  With a process group the region sums are made global before the division.
    """

    def __init__(self, num_regions=10, weight=10.0):
        super().__init__()
        self.l_mask_w = weight
        self.trainable_weight = torch.nn.Parameter(torch.ones(num_regions))

    def forward(self, sr, hr, mask_list, group=None, piggyback=None):
        """``piggyback``: a detached scalar (or small vector) summed over the ranks in the same collective as the region
        sums (the harness passes its local L1 value, and the SSIM value beside it when that criterion is on); its global
        sum is left in ``self.piggyback_sum``, in the same shape."""
        K = mask_list.shape[1]
        assert K == self.trainable_weight.numel(), "dynamic loss: %d trainable region weights but %d mask channels" % (self.trainable_weight.numel(), K)
        sm = F.softmax(self.trainable_weight, dim=0)
        diff = sr - hr
        nums, dens = [], []
        for i in range(K):
            m = F.interpolate(mask_list[:, i:i + 1], size=sr.shape[2:], mode="nearest")
            nums.append(F.smooth_l1_loss(m * diff, torch.zeros_like(diff), reduction="none").sum())
            dens.append(3.0 * m.sum())
        num, den = torch.stack(nums), torch.stack(dens)
        world = _world(group)
        self.piggyback_sum = piggyback
        if world > 1:
            parts = [num.detach(), den.detach()] + ([piggyback.detach().reshape(-1)] if piggyback is not None else [])
            g = torch.cat(parts)
            torch.distributed.all_reduce(g, group=group)          # one collective: numerators | denominators | piggyback
            gnum, gden = g[:K], g[K:2 * K]
            if piggyback is not None:
                self.piggyback_sum = g[2 * K] if piggyback.dim() == 0 else g[2 * K:]
            # value = global ratio; gradient: this rank's numerator over the global denominator, times world so
            # that the later gradient AVERAGE over ranks equals the gradient of the global loss
            local = num / gden * world
            per = gnum / gden
            per = per + (local - local.detach())
        else:
            per = num / den
        weighted = sm * per
        return list(per.unbind(0)), list(weighted.unbind(0)), weighted.sum() * self.l_mask_w, sm


class Trainer:
    """feed_data / optimize_parameters / test of the reference wrapper, for one DepthNet."""

    def __init__(self, net, num_regions=10, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0, pixel_weight=1.0,
                 dynamic_weight=10.0, group=None, T_period=(20000,) * 4, restarts=(20000, 40000, 60000),
                 restart_weights=(1, 1, 1), eta_min=1e-7, use_graph=False, ssim_weight=None, pixel_criterion="l1",
                 dynamic_criterion="smoothl1", mask_criterion=None, mask_weight=1.0):
        """``pixel_criterion`` ('l1' | 'l2' | 'cb'), ``dynamic_criterion`` ('l1' | 'l2' | 'smoothl1'), ``mask_criterion``
        (None: off | 'l1' | 'l2' | 'smoothl1') with ``mask_weight``, and ``dynamic_weight=None`` (dynamic term off): the
        ``train:`` switches of a reference yml (``networks.criteria(opt)`` maps one to these arguments;
        F_model_depthCond.py:50-58,78-84,164,183-190, mask_loss.py).  With the defaults nothing about a step changes: its
        launches, log keys, ``state_dict`` and captured graph are those of a Trainer without the arguments.  Any other
        combination goes through ``criterion_losses`` (see there for the values, which follow the reference, oddities
        included: 'cb' is a sum, 'l1' / 'l2' region losses are means over all elements): one ``_crit`` pass forward and one
        backward on the GPU.  'cb' as a region criterion raises NotImplementedError.
        The static mask loss draws ONE region per step as the reference does - ``np.random.randint(0, K, 1)[0]``
        (mask_loss.py:24), so seeding ``np.random`` reproduces its sequence - and adds ``mask_weight *`` that region's value,
        logged as ``l_mask`` and part of ``l_all``.  The drawn index lives in a device tensor that is refreshed before every
        step (under ``use_graph`` before every replay, the way the learning rate is); ``self.mask_region`` keeps the host
        copy.  With a process group the term stays RANK-LOCAL (value and log): the reference's ranks each draw their own
        region.  With ``dynamic_weight=None`` there are no trainable loss weights - none in the optimizer, none in the saved
        training state - and no ``l_dynamic`` in the log.

        ``ssim_weight``: None (the default) leaves the SSIM criterion off - the step, its launches and its log are those
        of a Trainer without the argument.  A number w switches it on as the reference does
        (``train.ssim_loss.use_ssim_criterion`` / ``ssim_weight``; F_model_depthCond.py:71-75,177-180):
        ``total += w * SSIM(sr, gt)`` - the SIMILARITY itself is added, so it takes a NEGATIVE weight to maximise it - and
        the log gains ``l_ssim`` (the weighted term, which ``l_all`` includes; with a process group the global value).  On
        the GPU the term is ``dasr_ssim`` forward and ``dasr_ssim_bwd`` backward, adding into the loss kernels' dL/dsr;
        under ``use_graph`` it is captured with the rest of the step.

        ``use_graph``: capture the whole step (zero_grad, forward, losses, backward, Adam) into ONE hipGraph after three
        eager steps and replay it afterwards - for steps whose ~2000 launches cost the host more than the GPU needs to run
        them (x8 / 16 frames / bf16: 22-30 ms of enqueue for a 35 ms step).  Single-rank only (the gradient exchange stays
        eager); same-shaped inputs (the loader's tensors are copied into the captured ones); Adam runs in its
        ``capturable`` form with the learning rate in a device tensor that the scheduler refreshes before every replay.
        The capture takes the kind of masks of the first captured batch: a step captured on soft masks accepts any later
        masks of that shape (one-hot included: the general kernels are correct for them), one captured on one-hot masks
        takes one-hot masks only."""
        self.net = net
        if group is None and torch.distributed.is_available() and torch.distributed.is_initialized():
            group = torch.distributed.group.WORLD
        self.group = group
        self.world = _world(group)
        device = next(net.parameters()).device
        check_criteria(pixel_criterion, dynamic_criterion, mask_criterion)
        self.pixel_criterion, self.dynamic_criterion, self.mask_criterion = pixel_criterion, dynamic_criterion, mask_criterion
        self.l_mask_w = float(mask_weight)
        # the default combination keeps the terms it always had (_losses: fused_losses / DynamicMaskLoss) and the order in
        # which its step adds them; any other adds in the reference's order (F_model_depthCond.py:163-190)
        self._default_criteria = (pixel_criterion == "l1" and dynamic_criterion == "smoothl1" and mask_criterion is None
                                  and dynamic_weight is not None)
        self._term_order = (("l_pix", "l_dynamic", "l_ssim") if self._default_criteria
                            else ("l_pix", "l_ssim", "l_mask", "l_dynamic"))
        self.dynamic_loss = None if dynamic_weight is None else DynamicMaskLoss(num_regions, dynamic_weight).to(device)
        self.mask_region = None
        self._mask_idx = None if mask_criterion is None else torch.zeros(1, dtype=torch.int64, device=device)
        self.l_pix_w = pixel_weight
        self.l_ssim_w = None if ssim_weight is None else float(ssim_weight)
        self.ssim_loss = None if ssim_weight is None else SSIMLoss()
        self.params = [p for p in net.parameters() if p.requires_grad]
        if self.dynamic_loss is not None:
            self.params += list(self.dynamic_loss.parameters())
        self.base_lr = lr
        self.use_graph = bool(use_graph) and device.type == "cuda" and self.world == 1
        self._graph = None
        self._static = None
        self._eager_steps = 0
        if self.use_graph:
            self._lr_t = torch.tensor(float(lr), device=device)
            self.optimizer = torch.optim.Adam(self.params, lr=self._lr_t, weight_decay=weight_decay, betas=betas,
                                              capturable=True)
        else:
            # on the GPU the multi-tensor "fused" form: one pass over the ~250 parameter tensors in a few launches instead
            # of the default's ~75 (1.3 ms of GPU time per step at x8; 64.3 -> 63.8 ms/step); same update rule, same state_dict
            self.optimizer = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay, betas=betas,
                                              fused=device.type == "cuda")
        self.sched = dict(T_period=T_period, restarts=restarts, weights=restart_weights, eta_min=eta_min)
        self.step_count = 0
        self.log = {}
        self._buckets = []           # [(flat tensor, [parameter indices], async work)] of the step in flight
        self._submitted = set()
        self._pindex = {}
        if self.world > 1:
            self._enable_dp(self.world)

    def _enable_dp(self, world):
        """Switch the gradient exchange on for ``world`` ranks (the constructor does this when the group has more than one
        rank; the single-GPU RCCL test calls it with a pretended world of 2 to exercise the bucketed path)."""
        self.world = world
        net = self.net
        names = getattr(net, "_param_names", None)
        if names is not None:        # the HIP DepthNet: its backward hands over completed gradients per tape bucket
            byname = dict(net.named_parameters())
            slot = {id(p): i for i, p in enumerate(self.params)}
            self._pindex = {n: slot[id(byname[n])] for n in names if id(byname[n]) in slot}
            object.__setattr__(net, "_grad_bucket_hook", self._on_grad_bucket)

    def update_learning_rate(self):
        self.step_count += 1                       # scheduler.step() comes first (codes/train.py:194)
        lr = cosine_restart_lr(self.step_count, self.base_lr, **self.sched)
        if self.use_graph:
            self._lr_t.fill_(lr)                   # the captured Adam reads the tensor
        else:
            for g in self.optimizer.param_groups:
                g["lr"] = lr
        return lr

    def _submit_bucket(self, idx, grads):
        """Pack ``grads`` (of parameters ``idx``) with one concatenation and start their all-reduce asynchronously."""
        if not grads:
            return
        flat = torch.cat([g.reshape(-1) for g in grads])
        work = torch.distributed.all_reduce(flat, group=self.group, async_op=True)
        self._buckets.append((flat, idx, work))
        self._submitted.update(idx)

    def _on_grad_bucket(self, pvars):
        """Called from the backward tape at each bucket boundary (tape.mark) with the net's parameter Vars: whatever has a
        gradient by now and has not been sent yet is complete (every parameter is packed exactly once) and goes out.
        Parameters that never receive a gradient (the constructed-but-unused block ``depth-residual{nb-2}``,
        SURVEY.md §8a row 1) never show up, on every rank alike, so the bucket layouts are identical everywhere."""
        idx, grads = [], []
        cur = torch.cuda.current_stream() if pvars and pvars[0].data.is_cuda else None
        for v in pvars:
            i = self._pindex.get(v.name)
            if i is None or v.grad is None or i in self._submitted:
                continue
            if cur is not None and v.grad_event is not None:   # produced on a side stream: order the pack after it
                cur.wait_event(v.grad_event)
            idx.append(i)
            grads.append(v.grad)
        self._submit_bucket(idx, grads)

    def _finish_allreduce(self):
        """The last bucket (everything the tape buckets did not cover, incl. the loss weights), then wait for all of them
        and write the averaged gradients back with one multi-tensor copy per bucket."""
        if self.world <= 1:
            return
        idx = [i for i, p in enumerate(self.params) if p.grad is not None and i not in self._submitted]
        self._submit_bucket(idx, [self.params[i].grad for i in idx])
        for flat, idx, work in self._buckets:
            work.wait()
            flat.div_(self.world)
            grads = [self.params[i].grad for i in idx]
            views, off = [], 0
            for g in grads:
                k = g.numel()
                views.append(flat[off:off + k].view_as(g))
                off += k
            torch._foreach_copy_(grads, views)
        self._buckets = []
        self._submitted = set()

    def optimize_parameters(self, lq, gt, depth, masks):
        if self.use_graph:
            return self._graphed_step(lq, gt, depth, masks)
        return self._eager_step(lq, gt, depth, masks)

    def _graphed_step(self, lq, gt, depth, masks):
        """Three eager steps (allocator pools, Adam state, side streams come into being), then capture, then replays."""
        if self._graph is None and self._eager_steps < 3:
            self._eager_steps += 1
            return self._eager_step(lq, gt, depth, masks)
        self.update_learning_rate()
        self._draw_mask_region(masks)              # the captured step reads the tensor
        if self._graph is None:
            from . import prep
            # any host read-back happens before the capture, not inside it: the answer (region bytes, or the soft stamp)
            # stays on the tensor and _step_body / fused_losses ask again for free
            self._static_soft = not prep.attach_region(masks)
            self._static = (lq, gt, depth, masks)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step_body(lq, gt, depth, masks)
            self._graph = g
            self._static_log = self.log
        else:
            from . import graph as _g, ops as _ops, prep as _prep
            if self._static[3] is not masks and not self._static_soft:   # region bytes travel with their mask tensor
                _prep.attach_region(masks)
                r_new, r_old = _g.attached_region(masks), getattr(self._static[3], "_dasr_region", None)
                if r_new is None or r_old is None:
                    raise ValueError("Trainer(use_graph=True): masks must be one-hot (prep.depth_to_masks / attach_region)")
                r_old.copy_(r_new)
            if self._static[3] is not masks and _g.attached_pair(self._static[3]) is not None:
                # the captured forward reads the captured masks' pair side-cars: they travel with their mask tensor too
                new = _g.attached_pair(masks)
                if new is None:
                    raise ValueError("Trainer(use_graph=True): the captured step reads a pair encoding; masks must come from "
                                     "prep.depth_to_soft_masks(pair=True)")
                for dst, src in zip(self._static[3]._dasr_pair, new):
                    dst.copy_(src)
            for dst, src in zip(self._static, (lq, gt, depth, masks)):
                if dst is not src:
                    if dst.shape != src.shape:
                        raise ValueError("Trainer(use_graph=True): the captured step has inputs of shape %s, got %s"
                                         % (tuple(dst.shape), tuple(src.shape)))
                    dst.copy_(src)
            if self._static[3] is not masks:       # the copy bumped the captured mask tensor's version: re-stamp it
                self._static[3]._dasr_version = _ops.tensor_version(self._static[3])
                if getattr(self._static[3], "_dasr_pair", None) is not None:
                    self._static[3]._dasr_pair_version = self._static[3]._dasr_version
        self._graph.replay()
        self.log = self._static_log
        return self.log

    def _eager_step(self, lq, gt, depth, masks):
        self.update_learning_rate()
        self._draw_mask_region(masks)
        return self._step_body(lq, gt, depth, masks)

    def _draw_mask_region(self, masks):
        """The static mask loss's region of this step, drawn as mask_loss.py:24 draws it, into the device tensor."""
        if self._mask_idx is not None:
            import numpy as np
            self.mask_region = int(np.random.randint(0, masks.shape[1], 1)[0])
            self._mask_idx.fill_(self.mask_region)

    def _step_body(self, lq, gt, depth, masks):
        self.optimizer.zero_grad(set_to_none=True)
        if masks.is_cuda:
            from . import prep
            prep.attach_region(masks)          # before the step's work is queued; free for prep.depth_to_masks output
        sr = self.net(lq, depth, masks)
        return self._finish_step(self._losses(sr, gt, masks, self.group if self.world > 1 else None))

    force_torch_criteria = False  # tests: a non-default combination through the PyTorch formulation on the same tensors

    def _finish_step(self, t):
        """Backward, gradient exchange, Adam and the log of a step whose terms ``_losses`` computed, added in
        ``self._term_order``."""
        terms = {"l_pix": ("l_pix", "l_pix_log"), "l_ssim": ("S", "S_log"), "l_mask": ("l_mask", "l_mask"),
                 "l_dynamic": ("l_dyn", "l_dyn")}
        total, log = None, {}
        for key in self._term_order:
            term, value = (t[k] for k in terms[key])
            if term is None:
                continue
            if key == "l_ssim":
                term, value = self.l_ssim_w * term, self.l_ssim_w * value
            total = term if total is None else total + term
            log[key] = value.detach()
        self._buckets, self._submitted = [], set()
        total.backward()
        self._finish_allreduce()
        self.optimizer.step()
        l_all = None
        for value in log.values():
            l_all = value if l_all is None else l_all + value
        log["l_all"] = l_all
        self.log = log
        return self.log

    def _losses(self, sr, gt, masks, grp):
        """The terms of a step, as the dict of ``criterion_losses``: ``l_pix`` / ``l_dyn`` / ``l_mask`` / ``S`` with their
        gradients (None for a term that is off), ``l_pix_log`` / ``S_log`` the global-batch values for the log.  Any
        combination but the default is ``criterion_losses``.  The default one is ``fused_losses`` - on the HIP path S
        shares the fused losses' autograd node and collective - and where that returns None, ``F.l1_loss`` +
        ``DynamicMaskLoss``, with S a term of its own (``SSIMLoss``) whose value rides with the L1 value in the dynamic
        loss's collective."""
        dyn = self.dynamic_loss
        if not self._default_criteria:
            return criterion_losses(sr, gt, masks, None if dyn is None else dyn.trainable_weight, self.l_pix_w,
                                    None if dyn is None else dyn.l_mask_w, self.pixel_criterion, self.dynamic_criterion,
                                    self.mask_criterion, self.l_mask_w, self._mask_idx, grp, self.ssim_loss,
                                    self.force_torch_criteria)
        on = self.ssim_loss is not None
        hip = on and self.ssim_loss.hip_ok(sr, gt)
        fused = fused_losses(sr, gt, masks, dyn.trainable_weight, self.l_pix_w, dyn.l_mask_w, grp,
                             **({"with_ssim": True} if hip else {}))
        S = S_log = None
        if fused is not None:
            l_pix, l_dyn, l_pix_log = fused[0], fused[1], fused[4]
            if hip:
                S, S_log = fused[5], fused[6]
            elif on:                                # (sr the kernels do not take, masks they do: a collective of its own)
                S = self.ssim_loss(sr, gt)
                S_log = S.detach()
                if self.world > 1:
                    S_log = S_log.clone()
                    torch.distributed.all_reduce(S_log, group=grp)
                    S_log = S_log / self.world
        else:
            l_pix = self.l_pix_w * F.l1_loss(sr, gt)
            if on:
                S = self.ssim_loss(sr, gt)
            piggyback = l_pix.detach() if S is None else torch.stack([l_pix.detach(), S.detach()])
            per, weighted, l_dyn, sm = dyn(sr, gt, masks, grp, piggyback=piggyback)
            glob = dyn.piggyback_sum / self.world                        # the global-batch values
            l_pix_log, S_log = (glob, None) if S is None else glob.unbind(0)
        return dict(l_pix=l_pix, l_pix_log=l_pix_log, l_dyn=l_dyn, l_mask=None, S=S, S_log=S_log)

    @torch.no_grad()
    def test(self, lq, depth, masks):
        self.net.eval()
        sr = self.net(lq, depth, masks)
        self.net.train()
        return sr


# ---- checkpoint interop (codes/models/base_model.py:77-119) --------------------------------
def save_network(net, path):
    """base_model.save_network: the module's state_dict (reference key names) with CPU tensors."""
    net = getattr(net, "module", net)
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, path)


def load_network(path, net, strict=True):
    """base_model.load_network: accepts the authors' `*_G.pth` files (a leading 'module.' from DataParallel
    checkpoints is stripped); strict key matching as in the reference."""
    net = getattr(net, "module", net)
    loaded = torch.load(path, map_location="cpu")
    clean = {(k[7:] if k.startswith("module.") else k): v for k, v in loaded.items()}
    return net.load_state_dict(clean, strict=strict)


def _save_training_state(trainer, path, epoch=0):
    """base_model.save_training_state: {'epoch','iter','schedulers','optimizers'}; the scheduler here is stateless
    given the step, so its entry holds the step and its constants.  'loss_weights' is an addition: the reference keeps
    the 10 dynamic-loss weights outside netG and does not checkpoint them at all."""
    state = {"epoch": epoch, "iter": trainer.step_count,
             "schedulers": [dict(last_epoch=trainer.step_count, base_lr=trainer.base_lr, **trainer.sched)],
             "optimizers": [trainer.optimizer.state_dict()]}
    if trainer.dynamic_loss is not None:           # (dynamic_weight=None: no trainable loss weights to keep)
        state["loss_weights"] = trainer.dynamic_loss.trainable_weight.detach().cpu()
    torch.save(state, path)


def _resume_training(trainer, state):
    """base_model.resume_training."""
    if isinstance(state, str):
        state = torch.load(state, map_location="cpu")
    assert len(state["optimizers"]) == 1, "Wrong lengths of optimizers"
    assert len(state["schedulers"]) == 1, "Wrong lengths of schedulers"
    trainer.optimizer.load_state_dict(state["optimizers"][0])
    trainer.step_count = int(state["schedulers"][0]["last_epoch"])
    if "loss_weights" in state and trainer.dynamic_loss is not None:
        with torch.no_grad():
            trainer.dynamic_loss.trainable_weight.copy_(state["loss_weights"].to(trainer.dynamic_loss.trainable_weight.device))
    return state.get("epoch", 0), state.get("iter", trainer.step_count)


Trainer.save_training_state = _save_training_state
Trainer.resume_training = _resume_training


def calculate_psnr(img1, img2):
    """PSNR on [0,255] images (codes/utils/util.py:646-653)."""
    mse = torch.mean((img1.double() - img2.double()) ** 2).item()
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))
