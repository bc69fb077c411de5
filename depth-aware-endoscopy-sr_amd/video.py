"""Video inference: uint8 frames in, uint8 frames out, the forward captured into one hipGraph.

``FrameUpscaler`` is the per-frame path of a deployed DepthNet: a camera frame is ``uint8`` HWC BGR (what ``cv2`` reads
and writes) and the network is NHWC inside, so one byte per sample crosses PCIe in each direction and no layout pass
runs on either side (csrc/frame.hip: ``dasr_frame_ingest_u8`` / ``dasr_frame_emit_u8``).  The depth masks are binned
from the depth map on the device (``dasr_depth_to_masks``), the network runs its inference plan from the NHWC image
(``DepthNet.infer_nhwc``), and with ``use_graph=True`` the whole chain - a few hundred launches that Python would
otherwise enqueue per frame - is replayed as one captured graph.

Reference counterparts: ``img2tensor`` / ``read_img`` (utils/util.py:596-605, data/util.py:78), ``F_Model_depthCond.test``
(F_model_depthCond.py:228-234), ``tensor2img`` (utils/util.py:566-590), ``getDepthMask``
(data/LQGTker_Depth_dataset.py:204-225)."""
import collections

import numpy as np
import torch

from . import ops, prep
from .depthnet import _device_guard


class _Slot:
    """Static buffers of one frame in flight: inputs and outputs of the (captured) chain, and their pinned host twins."""

    def __init__(self, B, h, w, C, scale, device, ensemble=False):
        self.frames = torch.empty((B, h, w, C), dtype=torch.uint8, device=device)
        self.depth = torch.empty((B, 1, h, w), dtype=torch.float32, device=device)
        self.out = torch.empty((B, scale * h, scale * w, C), dtype=torch.uint8, device=device)
        self.y = None                    # conv_output's NHWC result of the last run (before the clamp), for validate_u8
        if ensemble:
            # self-ensemble: the eight members of the image and of the depth map, group A (h x w) and group T (w x h) as
            # batches of 4B, and the merged (already clamped) result
            f32 = dict(dtype=torch.float32, device=device)
            self.xa, self.xt = torch.empty((4 * B, h, w, C), **f32), torch.empty((4 * B, w, h, C), **f32)
            self.da, self.dt = torch.empty((4 * B, 1, h, w), **f32), torch.empty((4 * B, 1, w, h), **f32)
            self.y = torch.empty((B, scale * h, scale * w, C), **f32)
        else:
            self.x = torch.empty((B, h, w, C), dtype=torch.float32, device=device)
        self.graph = None
        self.sig = None
        if device.type == "cuda":
            self.pin_frames = torch.empty((B, h, w, C), dtype=torch.uint8).pin_memory()
            self.pin_depth = torch.empty((B, 1, h, w), dtype=torch.float32).pin_memory()
            self.pin_out = torch.empty((B, scale * h, scale * w, C), dtype=torch.uint8).pin_memory()
            self.uploaded = torch.cuda.Event()
            self.computed = torch.cuda.Event()
            self.downloaded = torch.cuda.Event()


class _ShapeState:
    def __init__(self, *args):
        self.args = args                 # _Slot's: (B, h, w, C, scale, device, ensemble)
        self.slots = [_Slot(*self.args)]
        self.eager_calls = 0

    def slot(self, i):
        while len(self.slots) <= i:
            self.slots.append(_Slot(*self.args))
        return self.slots[i]


class FrameUpscaler:
    """``up = FrameUpscaler(net); sr = up.upscale(frames_u8, depth)``

    ``frames_u8``: ``[B,h,w,3]`` uint8 BGR (numpy array, CPU or GPU tensor; a single ``[h,w,3]`` frame is taken as B = 1),
    ``depth``: ``[B,1,h,w]`` float32.  Returns ``[B,s*h,s*w,3]`` uint8 BGR as a numpy array the caller owns.  The result
    is, byte for byte, ``tensor2img(validate.test(net, img2tensor(frames), depth, prep.depth_to_masks(depth))[b],
    min_max=min_max)``: only layout passes are left out.

    The network runs with ``eval()`` semantics under ``no_grad`` in its own compute dtype (fp32, or bf16 after
    ``net.set_compute_dtype``); ``net.min`` / ``net.max`` are the clamp of the network's output, ``min_max`` is
    ``tensor2img``'s range.

    ``soft_masks=None``: the reference's one-hot depth masks.  A number in (0, 1] is the blend ``width`` of
    ``prep.depth_to_soft_masks``: the chain bins the depth map into hat-function planes (``dasr_depth_to_masks_soft``) and
    the network runs its soft-mask kernels, so the output is continuous in the depth map from frame to frame; the result
    is then what ``validate.test`` gives with ``prep.depth_to_soft_masks(depth, num_masks, fixed_range, width)``.  It is a
    constructor constant (not part of a captured graph's signature).

    ``soft_pair=True`` (with ``soft_masks`` only, else ``ValueError``; a constructor constant too): the binning launch also
    writes the planes' pair encoding (``dasr_depth_to_masks_soft_pair``) and every SEAN forward is the pair-gather kernel
    (``dasr_sean_fwd_pair``) - the same function of the same planes as the general kernel, summed in the same order, at
    two table rows per tap instead of ``9 * num_masks`` terms.  Opt-in; the default runs the general kernels as before.

    ``self_ensemble=True``: geometric self-ensemble, ``validate.test_x8`` per frame - the result is, byte for byte,
    ``tensor2img(validate.test_x8(net, img2tensor(frames), depth, masks)[b])``.  The chain ingests the frame into its eight
    flip / transpose members (``dasr_ensemble_ingest_u8``), expands the depth map, bins the masks from the expanded depth
    maps (binning is pointwise given a sample's minimum and maximum, which do not depend on pixel order), runs two
    forwards of batch 4B - ``h x w`` and ``w x h`` - and merges (``dasr_ensemble_merge``) before the emit.  Roughly
    eight times the work per frame; a constructor constant like ``soft_masks``; everything below holds for it unchanged, the
    captured graph then contains both forwards.

    ``use_graph=True`` (GPU only, ignored elsewhere): the first two calls of an input shape run eagerly - the fold cache,
    the allocator's pools and the side stream of the depth branch come into being - the third captures
    ingest -> masks -> forward -> emit into one graph over static buffers and replays it, later calls copy in, replay and
    copy out.  A replay never runs Python, so the folded kernels inside it are those of the capture: before every replay
    the parameters' ``(data_ptr, version)`` tuple is compared with the one recorded at capture (what ``graph._folded``
    compares per kernel), and on a mismatch the graph is dropped and the shape starts its warm-up again.  One graph per
    input shape (two when ``upscale_iter`` is used), for the ``max_shapes`` most recently used shapes."""

    def __init__(self, net, num_masks=10, fixed_range=False, use_graph=True, min_max=(0, 1), max_shapes=4, soft_masks=None,
                 self_ensemble=False, soft_pair=False):
        self.net = net
        self.self_ensemble = bool(self_ensemble)
        self.num_masks = int(num_masks)
        self.fixed_range = bool(fixed_range)
        self.soft_masks = None if soft_masks is None else float(soft_masks)
        if self.soft_masks is not None and not 0.0 < self.soft_masks <= 1.0:
            raise ValueError("FrameUpscaler: soft_masks is the blend width, in (0, 1], got %r" % (soft_masks,))
        self.soft_pair = bool(soft_pair)
        if self.soft_pair and self.soft_masks is None:
            raise ValueError("FrameUpscaler: soft_pair is meaningful with soft_masks=WIDTH only")
        self.min_max = (min_max[0], min_max[1])
        p = next(net.parameters())
        self.device = p.device
        self.use_graph = bool(use_graph) and self.device.type == "cuda"
        self.max_shapes = int(max_shapes)
        self._shapes = collections.OrderedDict()
        self._edges = prep.fixed_range_edges(self.num_masks, self.device) if self.fixed_range else None
        self._copy_stream = None
        self._iterating = False          # an upscale_iter() generator of this upscaler is alive (its slots are in use)
        self.replays = 0                 # graph replays so far (tests and tools read it)
        self.captures = 0

    # ---- per-shape state ---------------------------------------------------------------------------------------------
    def _state(self, B, h, w, C):
        key = (B, h, w, C)
        st = self._shapes.get(key)
        if st is None:
            while len(self._shapes) >= self.max_shapes:         # the oldest shape goes, with its graphs and buffers
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                self._shapes.popitem(last=False)
            st = self._shapes[key] = _ShapeState(B, h, w, C, self.net.scale, self.device, self.self_ensemble)
        else:
            self._shapes.move_to_end(key)
        return st

    def _signature(self):
        """What a captured graph depends on besides its static buffers: every parameter's storage and version (the folded
        kernels inside the graph were built from them) and the compute dtype."""
        return (str(self.net._act_dtype(self.device)),
                tuple((p.data_ptr(), ops.tensor_version(p)) for p in self.net._resolve_params()))

    # ---- the chain -----------------------------------------------------------------------------------------------------
    def _masks(self, depth):
        if self.soft_pair:                               # as prep.depth_to_soft_masks(pair=True): planes and pair, one launch
            planes = prep.depth_to_soft_masks(depth, self.num_masks, self.fixed_range, self.soft_masks, pair=True)
        elif self.soft_masks is not None:
            planes = ops.depth_to_masks_soft(depth, self.num_masks, self.soft_masks, self.fixed_range)
            prep.mark_soft(planes)                       # as prep.depth_to_soft_masks: the general kernels, no read-back
        else:
            planes, region = ops.depth_to_masks(depth, self.num_masks, self._edges, want_planes=True)
            planes._dasr_region = region                 # as prep.depth_to_masks: no compression pass, no flag read-back
            planes._dasr_version = ops.tensor_version(planes)
        return planes

    def _chain(self, slot):
        if self.self_ensemble:
            B, _, h, w = slot.depth.shape
            ops.ensemble_ingest_u8(slot.frames, swap_rb=True, out=(slot.xa, slot.xt))
            ops.ensemble_expand(slot.depth.view(B, h, w, 1), out=(slot.da.view(4 * B, h, w, 1), slot.dt.view(4 * B, w, h, 1)))
            y_a = self.net.infer_nhwc(slot.xa, slot.da, self._masks(slot.da))
            y_t = self.net.infer_nhwc(slot.xt, slot.dt, self._masks(slot.dt))
            ops.ensemble_merge(y_a, y_t, self.net.min, self.net.max, out=slot.y)
        else:
            ops.frame_ingest_u8(slot.frames, swap_rb=True, out=slot.x)
            slot.y = self.net.infer_nhwc(slot.x, slot.depth, self._masks(slot.depth))
        ops.frame_emit_u8(slot.y, self.net.min, self.net.max, self.min_max, swap_rb=True, out=slot.out)

    def _compute(self, st, slot):
        """Run the chain for the frame in ``slot``'s static buffers on the current stream: eagerly, or as a graph replay."""
        if not self.use_graph:
            self._chain(slot)
            return
        sig = self._signature()
        if slot.graph is not None and slot.sig != sig:   # a parameter (or the compute dtype) changed: the graph is stale
            torch.cuda.synchronize(self.device)           # (the other slot's replay may still be running)
            for s in st.slots:
                s.graph = None
            st.eager_calls = 0
        if slot.graph is None and st.eager_calls < 2:
            st.eager_calls += 1
            self._chain(slot)
            return
        if slot.graph is None:
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            pool = next((s.graph.pool() for s in st.slots if s.graph is not None), None)
            with torch.cuda.graph(g, pool=pool):
                self._chain(slot)
            slot.graph, slot.sig = g, sig
            self.captures += 1
        slot.graph.replay()
        self.replays += 1

    # ---- input checks ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _as_tensors(frames, depth):
        f = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        d = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth))
        single = f.dim() == 3
        if single:
            f = f.unsqueeze(0)
        if f.dim() != 4 or f.dtype != torch.uint8:
            raise TypeError("FrameUpscaler: frames must be uint8 [B,h,w,C], got %s %s" % (f.dtype, tuple(f.shape)))
        B, h, w, C = f.shape
        if d.dtype != torch.float32 or d.numel() != B * h * w:
            raise TypeError("FrameUpscaler: depth must be float32 [B,1,h,w] matching the frames, got %s %s"
                            % (d.dtype, tuple(d.shape)))
        return f, d.reshape(B, 1, h, w), single

    # ---- one call ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _run(self, frames, depth):
        """upload -> chain -> (device results) on the current stream, without waiting for them.  Returns (slot, single)."""
        if self._iterating:
            raise RuntimeError("FrameUpscaler: upscale() / upscale_device() while an upscale_iter() of this upscaler is "
                               "suspended would reuse a slot with frames in flight; finish or close the iterator first")
        f, d, single = self._as_tensors(frames, depth)
        st = self._state(*f.shape)
        slot = st.slot(0)
        with _device_guard(slot.frames):
            if self.device.type != "cuda" or f.is_cuda:
                slot.frames.copy_(f)
                slot.depth.copy_(d)
            else:
                # the previous frame's upload out of these pinned buffers may still be queued behind earlier work (the
                # caller of upscale_device() does not synchronise): wait for it before the host writes into them again
                slot.uploaded.synchronize()
                slot.pin_frames.copy_(f)
                slot.pin_depth.copy_(d)
                slot.frames.copy_(slot.pin_frames, non_blocking=True)
                slot.depth.copy_(slot.pin_depth, non_blocking=True)
                slot.uploaded.record()
            self._compute(st, slot)
        return slot, single

    def upscale_device(self, frames, depth):
        """``upscale`` without the download and without any wait: returns ``(sr_u8, y)`` ON THE DEVICE - ``sr_u8``
        ``[B,s*h,s*w,3]`` uint8 BGR and ``y`` ``[B,s*h,s*w,3]`` float32, conv_output's NHWC result before the clamp to
        ``[net.min, net.max]`` (with ``self_ensemble`` the merged result, already clamped) - as work queued on the current
        stream.  Both are this upscaler's static buffers: they are valid until the next ``upscale`` / ``upscale_device`` call with frames of the same shape (which overwrites them,
        in stream order) and must be consumed on the same stream, or after a synchronise, before that.  The call never
        blocks on the GPU except to make sure the previous frame has left the pinned staging buffers.  For consumers that
        keep working on the device (``validate.validate_u8``)."""
        slot, single = self._run(frames, depth)
        return (slot.out[0], slot.y[0]) if single else (slot.out, slot.y)

    def upscale(self, frames, depth):
        slot, single = self._run(frames, depth)
        if self.device.type != "cuda":
            out = slot.out.numpy().copy()
        else:
            with _device_guard(slot.out):
                slot.pin_out.copy_(slot.out, non_blocking=True)
                torch.cuda.current_stream().synchronize()
            out = slot.pin_out.numpy().copy()
        return out[0] if single else out

    # ---- a stream of frames ------------------------------------------------------------------------------------------------
    def upscale_iter(self, pairs):
        """``for sr_u8 in up.upscale_iter((frames_u8, depth) for ...)``: results in input order, each a numpy array the
        caller owns (copied out of the pinned slot before the slot is used again).

        On the GPU this is a two-slot pipeline: two sets of pinned host and static device buffers and one copy stream; the
        upload of frame n+1 and the download of frame n-1 overlap the compute of frame n, and the result of frame n is
        yielded while frame n+2 is being staged.  A change of shape mid-stream first drains the frames in flight (they are
        yielded, in order) and then goes on with the new shape; an exception raised by ``pairs`` is re-raised after the
        frames already taken from it have been yielded; closing the generator early waits for the work in flight.
        While the generator is alive, ``upscale`` / ``upscale_device`` / a second ``upscale_iter`` of the same upscaler raise
        (they would reuse a slot with frames in flight); use a second ``FrameUpscaler`` for that."""
        if self.device.type != "cuda":
            for frames, depth in pairs:
                yield self.upscale(frames, depth)
            return
        if self._iterating:
            raise RuntimeError("FrameUpscaler: one upscale_iter() at a time (the two slots of a shape are in use)")
        with torch.cuda.device(self.device):
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=self.device)
            self._iterating = True
            try:
                yield from self._pipeline(iter(pairs), torch.cuda.current_stream(), self._copy_stream)
            finally:
                self._iterating = False

    def _finish(self, slot, single):
        slot.downloaded.synchronize()
        out = slot.pin_out.numpy().copy()
        return out[0] if single else out

    @torch.no_grad()
    def _pipeline(self, it, compute, copy):
        inflight = collections.deque()           # (slot, single), oldest first; at most two
        last = None                              # the newest frame: computed (or computing), its download not yet queued
        key, n, failure = None, 0, None

        def queue_download(slot):
            with torch.cuda.stream(copy):
                copy.wait_event(slot.computed)
                slot.pin_out.copy_(slot.out, non_blocking=True)
                slot.downloaded.record(copy)

        try:
            while True:
                try:
                    frames, depth = next(it)
                    f, d, single = self._as_tensors(frames, depth)
                except StopIteration:
                    break
                except Exception as e:           # the iterable failed: hand out what is in flight, then re-raise
                    failure = e
                    break
                if key is not None and tuple(f.shape) != key:        # a new shape: drain, then start over with it
                    if last is not None:
                        queue_download(last)
                        last = None
                    while inflight:
                        yield self._finish(*inflight.popleft())
                    n = 0
                key = tuple(f.shape)
                st = self._state(*key)
                slot = st.slot(n % 2)
                if len(inflight) == 2:           # this slot's previous frame: its download was queued one frame ago
                    yield self._finish(*inflight.popleft())
                # stage and upload frame n (copy stream), then the download of frame n-1 behind it, then compute n
                if f.is_cuda:
                    slot.frames.copy_(f)
                    slot.depth.copy_(d)
                else:
                    slot.pin_frames.copy_(f)
                    slot.pin_depth.copy_(d)
                    with torch.cuda.stream(copy):
                        slot.frames.copy_(slot.pin_frames, non_blocking=True)
                        slot.depth.copy_(slot.pin_depth, non_blocking=True)
                        slot.uploaded.record(copy)
                    compute.wait_event(slot.uploaded)
                if last is not None:
                    queue_download(last)
                self._compute(st, slot)
                slot.computed.record(compute)
                last = slot
                inflight.append((slot, single))
                n += 1
            if last is not None:
                queue_download(last)
                last = None
            while inflight:
                yield self._finish(*inflight.popleft())
            if failure is not None:
                raise failure
        finally:
            # (generator closed early, or an error in the chain itself) nothing may still be reading or writing a slot
            compute.synchronize()
            copy.synchronize()
