"""Device-side input preparation: the depth map is the only per-frame side input that has to
cross PCIe; the K depth-range planes and the region bytes the one-hot kernels read are derived from it on the GPU.
Masks from elsewhere are classified once per tensor (``attach_region``: one-hot -> region bytes, else a "soft" stamp;
``mark_soft`` for a loader that knows) and the answer travels with the tensor until it is edited in place.

Reference counterparts: ``LQGTker_Depth_dataset.getDepthMask`` (codes/data/LQGTker_Depth_dataset.py:204-225), the
``_disp.npy`` reader (``:152-154``) and the tensor packing (``:187-199``)."""
import numpy as np
import torch

from . import ops


def load_disp_npy(path):
    """``name_disp.npy`` as monodepth2 wrote it, ``[1,1,h,w]`` -> float32 ``[1,h,w]`` (LQGTker_Depth_dataset.py:152-154)."""
    d = np.load(path)
    if d.ndim == 4:
        d = d.squeeze(1)
    return torch.from_numpy(np.ascontiguousarray(d)).float()


def fixed_range_edges(num_masks, device):
    """Edges of the ``depthFixedRange: true`` mode: the reference evaluates ``0 + ((1-0)/K)*i`` in Python doubles
    and torch compares the float32 map against each edge rounded to float32."""
    interval = (1 - 0) / num_masks
    return torch.tensor([0 + interval * i for i in range(num_masks + 1)], dtype=torch.float64).to(torch.float32).to(device)


def depth_to_masks(depth, num_masks=10, fixed_range=False):
    """``depth`` ``[B,1,h,w]`` (or ``[B,h,w]``) float32 on the GPU -> ``DepthMaskList`` ``[B,K,h,w]`` float32, the
    tensor ``DepthNet.forward`` / the losses take.  The returned tensor carries the region bytes of the same masks
    (``_dasr_region``), which ``DepthNet`` and ``harness.fused_losses`` pick up instead of compressing the planes
    again (and without reading the one-hot flag back to the host)."""
    if depth.dtype != torch.float32:
        raise TypeError("depth_to_masks: depth must be float32")
    edges = fixed_range_edges(num_masks, depth.device) if fixed_range else None
    planes, region = ops.depth_to_masks(depth, num_masks, edges, want_planes=True)
    planes._dasr_region = region
    planes._dasr_version = ops.tensor_version(planes)     # the shortcut is dropped if the tensor is edited in place afterwards
    return planes


def depth_to_region(depth, num_masks=10, fixed_range=False):
    """Region bytes only (``[B,h,w]`` uint8; ``num_masks`` = "no bin")."""
    edges = fixed_range_edges(num_masks, depth.device) if fixed_range else None
    return ops.depth_to_masks(depth, num_masks, edges, want_planes=False)[1]


def _stamp(masks, region, soft):
    masks._dasr_region = region
    masks._dasr_soft = soft
    masks._dasr_version = ops.tensor_version(masks)       # either answer is dropped by an in-place edit (graph.attached_region)


def marked_soft(masks):
    """True while ``masks`` carries a valid "not one-hot" stamp (from ``attach_region`` or ``mark_soft``)."""
    return bool(getattr(masks, "_dasr_soft", False)) and getattr(masks, "_dasr_version", None) == ops.tensor_version(masks)


def mark_soft(masks):
    """Stamp a mask tensor as "treat as soft": no kernel, no read-back.  Always safe - the general kernels are correct for
    one-hot masks too, only slower.  A loader that knows its masks are soft calls this and gets a step free of host
    synchronisation (``attach_region`` then answers False at once).  An in-place edit of the tensor drops the stamp."""
    _stamp(masks, None, True)
    return masks


def _stamp_pair(masks, pair_k, pair_s):
    """The pair encoding of soft ``masks`` (include/dasr.h), under its own names: these bytes are not region bytes and never
    reach ``_dasr_region``.  Valid while the tensor is unmodified (``graph.attached_pair``)."""
    masks._dasr_pair = (pair_k, pair_s)
    masks._dasr_pair_version = ops.tensor_version(masks)


def pair_planes(pair_k, pair_s, K):
    """The decoding rule of the pair encoding (include/dasr.h) in torch: ``pair_k`` uint8, ``pair_s`` float32 ``[B,h,w]``
    -> planes ``[B,K,h,w]`` float32.  ``plane[k] = fl32(1 - |s|)``, ``plane[n] = |s|`` with ``n = k - 1`` for a negative
    ``s`` and ``k + 1`` otherwise, every other plane 0; a ``k >= K`` or an ``n`` outside ``0..K-1`` contributes nothing."""
    k = pair_k.to(torch.int64)
    a = pair_s.abs()
    n = torch.where(pair_s < 0, k - 1, k + 1)
    B, h, w = pair_k.shape
    planes = torch.zeros((B, K + 1, h, w), dtype=torch.float32, device=pair_s.device)   # plane K collects what is dropped
    kn = torch.where((n >= 0) & (n < K), n, torch.full_like(n, K))
    planes.scatter_(1, kn.unsqueeze(1), a.unsqueeze(1))
    planes.scatter_(1, k.clamp(max=K).unsqueeze(1), (1.0 - a).unsqueeze(1))
    return planes[:, :K].contiguous()


def depth_to_soft_masks(depth, num_masks=10, fixed_range=False, width=1.0, pair=False):
    """``depth`` ``[B,1,h,w]`` (or ``[B,h,w]``) float32 -> soft ``DepthMaskList`` ``[B,K,h,w]`` float32: hat-function
    membership in the K depth bins of ``depth_to_masks`` (``dasr_depth_to_masks_soft``; the rule is in include/dasr.h).
    ``width`` in (0, 1] is the share of a bin over which two neighbouring regions blend: 1 interpolates linearly between
    bin centres, a small width approaches the one-hot binning - but stays continuous in the depth value and in the
    sample's range, which the one-hot planes are not (a pixel crossing an edge switches region).  At most two planes are
    non-zero per pixel and they sum to 1; the maximum pixel belongs to plane K-1 (the one-hot rule leaves it in no bin).

    The result is stamped like ``mark_soft`` output: ``attach_region`` answers False at once, so ``harness.fused_losses``
    and a ``Trainer`` step (eager or captured) take the general (soft-mask) kernels without a compression pass of their
    own and without reading a flag back.

    ``pair=True``: the same launch also writes the masks' pair encoding (include/dasr.h) and the planes carry it, stamped with
    their version like the region bytes of ``depth_to_masks``: ``DepthNet`` then runs the pair-gather SEAN forward
    (``dasr_sean_fwd_pair``) instead of the general one; the backward and the losses read the planes as before.  An
    in-place edit of the planes drops the pair (and the soft stamp)."""
    # (the op raises TypeError for a depth that is not float32, ValueError for a width outside (0, 1] or more than 16 masks)
    if pair:
        planes, pair_k, pair_s = ops.depth_to_masks_soft(depth, int(num_masks), float(width), bool(fixed_range), pair=True)
        _stamp(planes, None, True)
        _stamp_pair(planes, pair_k, pair_s)
        return planes
    planes = ops.depth_to_masks_soft(depth, int(num_masks), float(width), bool(fixed_range))
    _stamp(planes, None, True)
    return planes


def attach_region(masks):
    """Give a mask tensor that did NOT come from ``depth_to_masks`` (e.g. the reference's CPU dataloader output moved to
    the GPU) its region bytes, so that the generator and the fused loss take the one-hot kernels without ever reading
    a flag back mid-step.  Costs one compression pass and ONE 4-byte read-back, here, before any of the step's work is
    queued.  Returns True when the masks are one-hot (region attached), False for soft / overlapping masks.

    Either answer is remembered on the tensor, stamped with its version: a second call on the same unmodified tensor
    launches nothing and reads nothing back, so the harness may ask again (and may ask inside a graph capture once it has
    asked before it).  A tensor stamped by ``mark_soft`` answers False without ever being looked at."""
    from . import graph
    if graph.attached_region(masks) is not None:
        return True
    if marked_soft(masks):
        return False
    if not masks.is_cuda or masks.dtype != torch.float32 or not masks.is_contiguous():
        return False
    region, flag = ops.mask_compress(masks)
    if int(flag.item()) != 0:
        _stamp(masks, None, True)
        return False
    _stamp(masks, region, False)
    return True
