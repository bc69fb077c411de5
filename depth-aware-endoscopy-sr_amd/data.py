"""Training batches from uint8 HR frames: the image half of the reference's training loader on the device.

The reference's ``LQGTker_Depth_dataset.__getitem__`` (codes/data/LQGTker_Depth_dataset.py:145-199) makes each sample on
the host: ``read_img``'s ``/ 255`` (codes/data/util.py:71-84), the MATLAB-style antialiased bicubic ``imresize_np``
(codes/data/util.py:258-458), ``getDepthMask``, ``augment`` (codes/data/util.py:101-118), BGR -> RGB, HWC -> CHW.
``BatchMaker`` takes the decoded uint8 HR frames and the LR-sized depth maps instead and makes the four tensors
``Trainer.optimize_parameters`` wants on the GPU (csrc/batch.hip): one byte per HR sample crosses PCIe.

``resize_tables`` and ``draw_augment`` are the two host-side pieces: the tap tables of the resize (float64, cached per
size) and the augmentation flags, drawn exactly as the reference draws them."""
import contextlib
import functools
import math

import numpy as np
import torch

from . import ops, prep

FLIP_H, FLIP_V, TRANSPOSE = 1, 2, 4
SCALES = (2, 3, 4, 8)


def _cubic(t):
    """Keys' cubic convolution kernel with a = -0.5 (what codes/data/util.py:258-264 evaluates), in float64."""
    t = np.abs(t)
    inner = (1.5 * t - 2.5) * t * t + 1.0
    outer = ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0
    return np.where(t <= 1, inner, np.where(t <= 2, outer, 0.0))


def reflect_lengths(s):
    """(low, high) number of samples ``imresize_np(., 1/s)`` mirrors at the two ends of an axis whose length is a
    multiple of s: 12 / 12 at s = 8, 6 / 6 at 4, 4 / 5 at 3, 3 / 3 at 2."""
    return -math.floor(0.5 - 1.5 * s), math.floor(0.5 + 1.5 * s)


@functools.lru_cache(maxsize=64)
def resize_tables(n_in, s):
    """Tap tables of ``imresize_np(img, 1/s, antialiasing=True)`` along an axis of ``n_in`` samples
    (calculate_weights_indices, codes/data/util.py:267-319, evaluated in float64): ``(weights float32 [n_out,4s], first
    int32 [n_out], reflect_lo, reflect_hi)``.  Output ``x`` (1-based) sits at ``u = s x + 0.5 (1 - s)``; its taps are the
    ``4s`` inputs ``first[x] .. first[x] + 4s - 1`` (0-based, before the symmetric reflection the kernel applies) with
    weights ``cubic((u - i) / s) / s`` normalised to sum 1.  The reference starts from ``4s + 2`` columns and drops the
    first and the last, whose weights are zero for every integer s.  The arrays are cached: do not write into them."""
    n_in, s = int(n_in), int(s)
    if s not in SCALES:
        raise ValueError("resize_tables: scale must be one of %s, got %r" % (SCALES, s))
    if n_in <= 0 or n_in % s:
        raise ValueError("resize_tables: length %d is not a positive multiple of the scale %d" % (n_in, s))
    lo, hi = reflect_lengths(s)
    if n_in < max(lo, hi):
        raise ValueError("resize_tables: length %d is shorter than the %d samples the resize mirrors at scale %d "
                         "(the reference raises there too)" % (n_in, max(lo, hi), s))
    n_out = n_in // s
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = s * x + 0.5 * (1 - s)                                   # exact: s is an integer
    first = np.floor(u - 2 * s).astype(np.int64)                # 0-based index of the first of the 4s taps that are kept
    pos = (first + 1)[:, None] + np.arange(4 * s)[None, :]      # their 1-based positions
    w = _cubic((u[:, None] - pos) / s) / s
    # the two columns the reference drops carry no weight, so the sum over the 4s kept ones is its normaliser
    assert not _cubic((u - first) / s).any() and not _cubic((u - first - 4 * s - 1) / s).any()
    w = w / w.sum(axis=1, keepdims=True)
    assert -int(first[0]) == lo and int(first[-1]) + 4 * s - n_in == hi
    first = first.astype(np.int32)
    weights = np.ascontiguousarray(w.astype(np.float32))
    weights.setflags(write=False)
    first.setflags(write=False)
    return weights, first, lo, hi


def draw_augment(rng, B, use_flip=True, use_rot=True):
    """uint8 [B] augmentation flags (bit 0 hflip, bit 1 vflip, bit 2 transpose) drawn from ``rng`` (a ``random.Random``, or
    the ``random`` module) as the reference's ``augment`` draws them for each sample (codes/data/util.py:103-105):
    ``hflip and random() < 0.5``, ``rot and random() < 0.5``, ``rot and random() < 0.5`` - an option that is off draws
    nothing.  The same seed gives the reference loader's augmentations."""
    flags = np.zeros((B,), dtype=np.uint8)
    for b in range(B):
        hflip = use_flip and rng.random() < 0.5
        vflip = use_rot and rng.random() < 0.5
        rot90 = use_rot and rng.random() < 0.5
        flags[b] = (FLIP_H if hflip else 0) | (FLIP_V if vflip else 0) | (TRANSPOSE if rot90 else 0)
    return flags


class _Buffers:
    """Static buffers of one input shape: the uploads, the per-sample tables, the resize tables and the four outputs."""

    def __init__(self, B, H, W, s, ch, cw, K, crop, device, soft=False):
        h, w = H // s, W // s
        dev = device
        self.frames = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        self.depth_in = torch.empty((B, 1, h, w), dtype=torch.float32, device=dev)
        self.flags = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.origins = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        wh, ih, _, _ = resize_tables(H, s)
        ww, iw, _, _ = resize_tables(W, s)
        self.tables = tuple(torch.from_numpy(np.array(t)).to(dev) for t in (wh, ih, ww, iw))
        self.lq = torch.empty((B, 3, ch, cw), dtype=torch.float32, device=dev)
        self.gt = torch.empty((B, 3, s * ch, s * cw), dtype=torch.float32, device=dev)
        self.depth = torch.empty((B, 1, ch, cw), dtype=torch.float32, device=dev)
        self.masks = torch.empty((B, K, ch, cw), dtype=torch.float32, device=dev)
        if not soft:                                 # soft masks have no region bytes
            self.region = torch.empty((B, ch, cw), dtype=torch.uint8, device=dev)
        if crop:                                     # the masks of the full depth map, before the window is cut out
            self.full_masks = torch.empty((B, K, h, w), dtype=torch.float32, device=dev)
            if not soft:
                self.full_region = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
        if dev.type == "cuda":
            self.pin_frames = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()
            self.pin_depth = torch.empty((B, 1, h, w), dtype=torch.float32).pin_memory()
            self.pin_flags = torch.zeros((B,), dtype=torch.uint8).pin_memory()
            self.pin_origins = torch.zeros((B, 2), dtype=torch.int32).pin_memory()
            self.uploaded = torch.cuda.Event()


class BatchMaker:
    """``mk = BatchMaker(scale); lq, gt, depth, masks = mk.make(hr_u8, depth, flags, origins)``

    ``hr_u8``: ``[B,H,W,3]`` uint8 BGR HR frames (what ``cv2.imread`` returns; numpy array, CPU or GPU tensor), ``depth``:
    ``[B,1,h,w]`` float32 at LR size (``h = H / scale``), ``flags``: uint8 ``[B]`` from ``draw_augment`` (None: no
    augmentation), ``origins``: int ``[B,2]`` LR crop origins ``(oy, ox)`` (crop mode only; None: all zero).  Returns the
    four NCHW float32 tensors ``Trainer.optimize_parameters(lq, gt, depth, masks)`` takes; ``masks`` carries its region
    bytes (``_dasr_region`` / ``_dasr_version``) like ``prep.depth_to_masks`` output.

    ``crop=None``: the whole frame.  The masks are binned from the augmented depth map: ``getDepthMask`` is pointwise
    given a sample's minimum and maximum, so this equals augmenting the reference's masks bit for bit.
    ``crop=(ch, cw)`` (LR pixels): every sample is cut to that window at its origin.  The masks are binned from the
    FULL depth map first (a window has another minimum and maximum), then the K planes and the region bytes are cut and
    augmented like the depth map (``ops.batch_plane``, float32 and uint8).

    ``soft_masks=None``: the reference's one-hot masks, as above.  A number in (0, 1] is the blend ``width`` of
    ``prep.depth_to_soft_masks``: ``masks`` are hat-function planes (``dasr_depth_to_masks_soft``), binned from the
    augmented depth map without crop (the rule is pointwise given a sample's minimum and maximum, so this equals
    augmenting the planes) and from the FULL depth map, then cut and augmented as float32 planes, with crop.  No region
    bytes exist in this mode (none are allocated); ``masks`` is re-stamped soft (``prep.mark_soft``'s stamp) after every
    ``make``.  ``harness.Trainer`` needs nothing else: it already takes soft-stamped masks through the soft-mask kernels,
    eagerly and captured (``use_graph=True``), without a read-back.

    **Lifetime.**  The four results are this object's static buffers of the input shape: the next ``make`` with frames of
    the same shape overwrites them, in stream order.  Consume them (on the same stream) before calling ``make`` again,
    or ``clone()`` them.  That is what lets ``Trainer(use_graph=True)`` see the same addresses every step and skip its
    own input copies.  Host inputs go through ONE set of pinned staging buffers per shape; ``make`` waits for the
    previous upload out of them before it writes into them again, and for nothing else.  Frames that are already on the
    GPU are copied into the static frame buffer too (device to device; 63 MB at 16 frames of 1024x1280): the chain, and a
    graph captured over it, always reads the same addresses."""

    def __init__(self, scale, num_masks=10, fixed_range=False, crop=None, device=None, max_shapes=4, soft_masks=None):
        self.scale = int(scale)
        if self.scale not in SCALES:
            raise ValueError("BatchMaker: scale must be one of %s, got %r" % (SCALES, scale))
        self.num_masks = int(num_masks)
        self.fixed_range = bool(fixed_range)
        self.soft_masks = None if soft_masks is None else float(soft_masks)
        if self.soft_masks is not None:
            if not 0.0 < self.soft_masks <= 1.0:
                raise ValueError("BatchMaker: soft_masks is the blend width, in (0, 1], got %r" % (soft_masks,))
            if not 1 <= self.num_masks <= 16:
                raise ValueError("BatchMaker: soft masks take 1..16 regions, got %d" % self.num_masks)
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        if self.crop is not None and min(self.crop) <= 0:
            raise ValueError("BatchMaker: crop must be positive, got %r" % (crop,))
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.max_shapes = int(max_shapes)
        self._edges = prep.fixed_range_edges(self.num_masks, self.device) if self.fixed_range else None
        self._shapes = {}

    def _buffers(self, B, H, W):
        s = self.scale
        if H % s or W % s:
            raise ValueError("BatchMaker: frame size %dx%d is not a multiple of the scale %d" % (H, W, s))
        resize_tables(H, s)                       # refuses sides shorter than the reflection
        resize_tables(W, s)
        ch, cw = self.crop if self.crop is not None else (H // s, W // s)
        if ch > H // s or cw > W // s:
            raise ValueError("BatchMaker: crop %dx%d is larger than the %dx%d LR image" % (ch, cw, H // s, W // s))
        key = (B, H, W)
        buf = self._shapes.pop(key, None)
        if buf is None:
            while len(self._shapes) >= self.max_shapes:
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                self._shapes.pop(next(iter(self._shapes)))
            buf = _Buffers(B, H, W, s, ch, cw, self.num_masks, self.crop is not None, self.device,
                           soft=self.soft_masks is not None)
        self._shapes[key] = buf                   # most recently used last
        return buf, ch, cw

    @staticmethod
    def _tensor(x):
        return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))

    @torch.no_grad()
    def make(self, hr_u8, depth, flags=None, origins=None):
        f, d = self._tensor(hr_u8), self._tensor(depth)
        if f.dim() != 4 or f.dtype != torch.uint8 or f.shape[-1] != 3:
            raise TypeError("BatchMaker: hr_u8 must be uint8 [B,H,W,3], got %s %s" % (f.dtype, tuple(f.shape)))
        B, H, W, _ = f.shape
        buf, ch, cw = self._buffers(B, H, W)
        h, w = H // self.scale, W // self.scale
        if d.dtype != torch.float32 or d.numel() != B * h * w:
            raise TypeError("BatchMaker: depth must be float32 [B,1,%d,%d], got %s %s" % (h, w, d.dtype, tuple(d.shape)))
        d = d.reshape(B, 1, h, w)
        fl = np.zeros((B,), dtype=np.uint8) if flags is None else flags
        if torch.is_tensor(fl):
            fl = fl.cpu().numpy()
        fl = np.asarray(fl)
        if fl.dtype != np.uint8 or fl.shape != (B,):
            raise TypeError("BatchMaker: flags must be uint8 [B], got %s %s" % (fl.dtype, fl.shape))
        if (fl > 7).any():
            raise ValueError("BatchMaker: flags use bits 0..2 only")
        transpose = bool((fl & TRANSPOSE).any())
        if transpose and ch != cw:
            raise ValueError("BatchMaker: a transposed sample needs a square window (a batch has one shape), got %dx%d"
                             % (ch, cw))
        if origins is None:
            og = np.zeros((B, 2), dtype=np.int32)
        else:
            if self.crop is None:
                raise ValueError("BatchMaker: origins need crop=(ch, cw)")
            og = origins.cpu().numpy() if torch.is_tensor(origins) else np.asarray(origins)
            if og.shape != (B, 2) or og.dtype.kind not in "iu":
                raise TypeError("BatchMaker: origins must be integers [B,2], got %s %s" % (og.dtype, og.shape))
            if (og < 0).any() or (og[:, 0] + ch > h).any() or (og[:, 1] + cw > w).any():
                raise ValueError("BatchMaker: a %dx%d crop at these origins leaves the %dx%d LR image" % (ch, cw, h, w))
            og = og.astype(np.int32)

        with torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext():
            if self.device.type != "cuda":
                buf.frames.copy_(f)
                buf.depth_in.copy_(d)
                buf.flags.copy_(torch.from_numpy(fl))
                buf.origins.copy_(torch.from_numpy(og))
            else:
                # the previous call's uploads out of the pinned buffers may still be queued: wait before rewriting them
                buf.uploaded.synchronize()
                for pin, dst, src in ((buf.pin_frames, buf.frames, f), (buf.pin_depth, buf.depth_in, d),
                                      (buf.pin_flags, buf.flags, torch.from_numpy(fl)),
                                      (buf.pin_origins, buf.origins, torch.from_numpy(og))):
                    if src.is_cuda:
                        dst.copy_(src)
                    else:
                        pin.copy_(src)
                        dst.copy_(pin, non_blocking=True)
                buf.uploaded.record()
            self._chain(buf, ch, cw, transpose)
        return buf.lq, buf.gt, buf.depth, buf.masks

    def _chain(self, buf, ch, cw, transpose):
        """The device work of one batch on the current stream; everything it reads and writes is a static buffer."""
        s, K = self.scale, self.num_masks
        win = (ch, cw)
        origins = buf.origins if self.crop is not None else None
        ops.batch_lr_u8(buf.frames, s, buf.tables, win, origins, buf.flags, transpose, out=buf.lq)
        ops.batch_gt_u8(buf.frames, s, win, origins, buf.flags, transpose, out=buf.gt)
        ops.batch_plane(buf.depth_in, win, origins, buf.flags, transpose, out=buf.depth)
        if self.soft_masks is not None:
            if self.crop is None:
                ops.depth_to_masks_soft(buf.depth, K, self.soft_masks, self.fixed_range, out=buf.masks)
            else:
                ops.depth_to_masks_soft(buf.depth_in, K, self.soft_masks, self.fixed_range, out=buf.full_masks)
                ops.batch_plane(buf.full_masks, win, origins, buf.flags, transpose, out=buf.masks)
            prep.mark_soft(buf.masks)                # soft: the general kernels, no read-back of a one-hot flag
            return
        if self.crop is None:
            ops.depth_to_masks(buf.depth, K, self._edges, out=(buf.masks, buf.region))
        else:
            ops.depth_to_masks(buf.depth_in, K, self._edges, out=(buf.full_masks, buf.full_region))
            ops.batch_plane(buf.full_masks, win, origins, buf.flags, transpose, out=buf.masks)
            ops.batch_plane(buf.full_region, win, origins, buf.flags, transpose, out=buf.region)
        buf.masks._dasr_region = buf.region
        buf.masks._dasr_version = ops.tensor_version(buf.masks)

