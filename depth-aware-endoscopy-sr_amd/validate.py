"""Validation path: the reference's `test()` + `tensor2img` + cropped PSNR + SSIM loop
(codes/train.py:219-271, models/F_model_depthCond.py:228-234, utils/util.py:566-590,646-653,
pytorch_ssim/__init__.py:7-37,65-73) for one DepthNet.  The forward is the inference plan of `DepthNet`
(`net.eval()` + `torch.no_grad()`: no tape, weights folded once); the metrics are computed where the images are."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def tensor2img(tensor, out_type=np.uint8, min_max=(0, 1)):
    """utils/util.py:566-590 for 3-D (C,H,W) and 2-D (H,W) tensors: clamp, rescale to [0,1], RGB->BGR, HWC,
    `round(x*255)` for uint8.  (The 4-D branch builds a grid with torchvision, which the validation loop never
    reaches: `visuals['SR']` is one image.)"""
    tensor = tensor.squeeze().float().cpu().clamp(*min_max)
    tensor = (tensor - min_max[0]) / (min_max[1] - min_max[0])
    if tensor.dim() == 3:
        img = np.transpose(tensor.numpy()[[2, 1, 0], :, :], (1, 2, 0))
    elif tensor.dim() == 2:
        img = tensor.numpy()
    else:
        raise TypeError("tensor2img: only 3-D and 2-D tensors are supported here, got %d-D" % tensor.dim())
    if out_type == np.uint8:
        img = (img * 255.0).round()
    return img.astype(out_type)


def calculate_psnr(img1, img2):
    """utils/util.py:646-653, images in [0,255] (numpy arrays or tensors)."""
    a = np.asarray(img1.cpu() if torch.is_tensor(img1) else img1, dtype=np.float64)
    b = np.asarray(img2.cpu() if torch.is_tensor(img2) else img2, dtype=np.float64)
    mse = np.mean((a - b) ** 2)
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))


def _window_1d(window_size=11, sigma=1.5):
    """The reference's 1-D Gaussian, built the way pytorch_ssim builds it (fp32 tensor, normalised in fp32)."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                     dtype=torch.float32)
    return g / g.sum()


def ssim(img1, img2, window_size=11, size_average=True):
    """pytorch_ssim.ssim (pytorch_ssim/__init__.py:17-37,65-73): 11x11 Gaussian (sigma 1.5) windows, zero padding,
    C1 = 0.01^2, C2 = 0.03^2 on [0,1] images `[B,C,H,W]` - one HIP kernel pass over both images (dasr_ssim: the five
    windowed moments, the SSIM ratio and its mean), no torch compute ops."""
    from . import ops
    if window_size != 11:
        raise NotImplementedError("dasr_amd.validate.ssim: the reference's 11 x 11 window only")
    out = ops.ssim(img1, img2)
    return out.mean() if size_average else out


@torch.no_grad()
def test(net, lq, depth, masks):
    """F_Model_depthCond.test (F_model_depthCond.py:228-234): eval-mode forward without autograd, back to train()."""
    was_training = net.training
    net.eval()
    try:
        return net(lq, depth, masks)
    finally:
        if was_training:
            net.train()


def _expand_conditioning(depth, masks):
    """The depth map ``[B,1,h,w]`` and the mask planes ``[B,K,h,w]`` under the eight symmetries of ``test_x8``:
    ``((depth_a, masks_a), (depth_t, masks_t))``, group A ``[4B,.,h,w]`` and group T ``[4B,.,w,h]``.  A plane is an
    ``[h,w,1]`` image to ``ops.ensemble_expand``, so each member block is again ``[B,K,..]``.  The masks' stamp travels:
    attached region bytes are expanded with them (uint8), a soft stamp is repeated, unstamped masks stay unstamped."""
    from . import graph, ops, prep
    B, K, h, w = masks.shape
    da, dt = ops.ensemble_expand(depth.contiguous().view(B, h, w, 1))
    ma, mt = ops.ensemble_expand(masks.contiguous().view(B * K, h, w, 1))
    ma, mt = ma.view(4 * B, K, h, w), mt.view(4 * B, K, w, h)
    region = graph.attached_region(masks)
    if region is not None:
        ra, rt = ops.ensemble_expand(region.contiguous().view(B, h, w, 1))
        for planes, r in ((ma, ra.view(4 * B, h, w)), (mt, rt.view(4 * B, w, h))):
            planes._dasr_region = r
            planes._dasr_version = ops.tensor_version(planes)
    elif prep.marked_soft(masks):
        prep.mark_soft(ma)
        prep.mark_soft(mt)
    return (da.view(4 * B, 1, h, w), ma), (dt.view(4 * B, 1, w, h), mt)


@torch.no_grad()
def test_x8(net, lq, depth, masks):
    """Geometric self-ensemble inference, the depth-conditioned form of ``F_Model_depthCond.test_x8``
    (F_model_depthCond.py:236-270): the frame under the eight flip / transpose symmetries - member ``m = v + 2h + 4t`` in the
    reference's list order, ``v`` a flip along W, ``h`` along H, ``t`` a transpose applied last - through the generator,
    each result mapped back, the eight averaged.  Arguments and result as ``test``: ``lq`` ``[B,3,h,w]``, ``depth``
    ``[B,1,h,w]``, ``masks`` ``[B,K,h,w]`` float32 -> ``[B,3,sh,sw]`` float32 in ``[net.min, net.max]``; eval-mode forward
    without autograd, the module's mode restored afterwards.

    The reference's own ``test_x8`` calls ``self.netG(aug)`` with the image alone: it omits the depth map and the masks
    and cannot run on ``DepthNet``, whose forward takes ``(input, depthMap, depthMask)``.  Here the depth map and the masks
    (with their region bytes or soft stamp) are transformed with the image; member order and merge rule are the
    reference's, and each member gets ``DepthNet.forward``'s output clamp before the mean.

    Two forwards, always (also for square frames): members 0..3 (``h x w``) as one batch of 4B, members 4..7 (``w x h``)
    as another.  Members of one group share a forward batch, and the fp16x2 split convolutions scale by a batch-wide
    maximum, so the result is that of these two batched forwards, not of eight separate ones.  The flips and the merge are
    HIP kernels on NHWC tensors (``ops.ensemble_expand`` / ``ops.ensemble_merge``); the sum is
    ``0.125 * (((((((z0 + z1) + z2) + z3) + z4) + z5) + z6) + z7)`` in fp32."""
    from . import ops
    from .depthnet import _device_guard
    for t, nm in ((lq, "lq"), (depth, "depth"), (masks, "masks")):
        if t.dtype != torch.float32 or t.dim() != 4 or t.device != lq.device:
            raise ValueError("test_x8: %s must be a 4-D float32 tensor on lq's device" % nm)
    B, _, h, w = lq.shape
    if tuple(depth.shape) != (B, 1, h, w) or masks.shape[0] != B or tuple(masks.shape[2:]) != (h, w):
        raise ValueError("test_x8: lq %s, depth %s and masks %s do not belong together"
                         % (tuple(lq.shape), tuple(depth.shape), tuple(masks.shape)))
    was_training = net.training
    net.eval()
    try:
        with _device_guard(lq):
            xa, xt = ops.ensemble_expand(ops.nchw_to_nhwc(lq.contiguous()))
            (da, ma), (dt, mt) = _expand_conditioning(depth, masks)
            ya = net.infer_nhwc(xa, da, ma)
            yt = net.infer_nhwc(xt, dt, mt)
            return ops.nhwc_to_nchw(ops.ensemble_merge(ya, yt, net.min, net.max))
    finally:
        if was_training:
            net.train()


def validate(net, frames, scale):
    """The validation loop of codes/train.py:219-262 over an iterable of `(LQ, GT, Depth, DepthMaskList)` frames
    (`[1,3,h,w]`, `[1,3,sh,sw]`, `[1,1,h,w]`, `[1,K,h,w]`): SSIM of the [0,1] tensors (pytorch_ssim), PSNR of the
    uint8 images with a `scale`-pixel border cropped.  Returns (avg_psnr, avg_ssim, n)."""
    psnr_sum = ssim_sum = 0.0
    n = 0
    for lq, gt, depth, masks in frames:
        sr = test(net, lq, depth, masks)
        ssim_sum += float(ssim(sr[:1].detach().float(), gt[:1].to(sr.device).float()))
        sr_img = tensor2img(sr[0]) / 255.0
        gt_img = tensor2img(gt[0]) / 255.0
        c = scale
        psnr_sum += calculate_psnr(sr_img[c:-c, c:-c, :] * 255, gt_img[c:-c, c:-c, :] * 255)
        n += 1
    return psnr_sum / max(n, 1), ssim_sum / max(n, 1), n


def validate_u8(net, frames, scale, num_masks=10, fixed_range=False, use_graph=False, soft_masks=None,
                self_ensemble=False, soft_pair=False):
    """The loop of ``validate()`` for a video source: ``frames`` yields ``(LQ, GT, Depth)`` with ``LQ`` a ``uint8``
    ``[1,h,w,3]`` (or ``[h,w,3]``) BGR frame as ``cv2`` reads it, ``GT`` the ``[1,3,sh,sw]`` float tensor and ``Depth``
    ``[1,1,h,w]``; a fourth item (the reference loader's mask list) is ignored, the masks are binned on the device.
    SR comes from ``video.FrameUpscaler``; GT is quantised by the same kernel's ``tensor2img`` half; PSNR is
    ``20 log10(255 / sqrt(ssd / n))`` from the exact integer sum of squared differences of the two uint8 images with a
    ``scale``-pixel border cropped (``dasr_frame_ssd_u8``; ``inf`` at ``ssd == 0``); SSIM is ``dasr_ssim`` of the [0,1]
    tensors as in ``validate()``.  Nothing is read back per frame: the sums stay on the device and come to the host in
    one transfer at the end.  ``soft_masks``: ``FrameUpscaler``'s (None: one-hot masks; a number: soft masks of that blend
    width; ``soft_pair``: its pair-gather forward for them).  ``self_ensemble``: ``FrameUpscaler``'s - SR is then ``test_x8``'s geometric self-ensemble, the figures of a
    paper's "+" rows.  Returns (avg_psnr, avg_ssim, n)."""
    from . import ops
    from .video import FrameUpscaler
    up = FrameUpscaler(net, num_masks=num_masks, fixed_range=fixed_range, use_graph=use_graph, min_max=(0, 1),
                       soft_masks=soft_masks, self_ensemble=self_ensemble, soft_pair=soft_pair)
    dev = up.device
    CHUNK = 256
    chunks, counts = [], []              # int64 [2*CHUNK] each: ssd in the first half, ssim (float32 bits) in the second

    def view(i):
        if i // CHUNK >= len(chunks):
            chunks.append(torch.zeros((2 * CHUNK,), dtype=torch.int64, device=dev))
        buf, j = chunks[i // CHUNK], i % CHUNK
        return buf[j:j + 1], buf[CHUNK:].view(torch.float32)[j:j + 1]

    inf = float("inf")
    with torch.no_grad():
        for i, item in enumerate(frames):
            lq, gt, depth = item[0], item[1], item[2]
            lq = lq if torch.is_tensor(lq) else torch.from_numpy(np.ascontiguousarray(lq))
            sr_u8, y = up.upscale_device(lq[None] if lq.dim() == 3 else lq, depth)     # on the device, nothing waited for
            gt = gt[:1].to(dev).float().contiguous()
            ssd_out, ssim_out = view(i)
            sr = ops.clamp_to_nchw(y[:1].contiguous(), net.min, net.max)
            ops.copy_(ssim_out, ssim(sr, gt, size_average=False))
            gt_u8 = ops.frame_emit_u8(ops.nchw_to_nhwc(gt), -inf, inf, (0, 1), swap_rb=True)
            _, H, W, C = gt_u8.shape
            ops.frame_ssd_u8(sr_u8[:1].contiguous(), gt_u8, crop=scale, out=ssd_out)
            counts.append((H - 2 * scale) * (W - 2 * scale) * C)
    n = len(counts)
    if n == 0:
        return 0.0, 0.0, 0
    host = (chunks[0] if len(chunks) == 1 else torch.cat(chunks)).cpu()          # the one read-back
    psnr_sum = ssim_sum = 0.0
    for i, cnt in enumerate(counts):
        buf, j = host[2 * CHUNK * (i // CHUNK):2 * CHUNK * (i // CHUNK + 1)], i % CHUNK
        ssd = int(buf[j])
        psnr_sum += inf if ssd == 0 else 20 * math.log10(255.0 / math.sqrt(ssd / cnt))
        ssim_sum += float(buf[CHUNK:].view(torch.float32)[j])
    return psnr_sum / n, ssim_sum / n, n


def _figures(ssd, sums, Hc, Wc, C):
    """The test script's figures of one frame from dasr_image_metrics_u8's sums (include/dasr.h): psnr and ssim, and for a
    3-channel image psnr_y and ssim_y (test.py:117-135 has no luma figures for a gray one)."""
    inf = float("inf")
    positions = (Hc - 10) * (Wc - 10)
    out = dict(psnr=inf if ssd == 0 else 20 * math.log10(255.0 / math.sqrt(ssd / (Hc * Wc * C))),
               ssim=sums[1] / (positions * C))
    if C == 3:
        out["psnr_y"] = inf if sums[0] == 0 else 20 * math.log10(255.0 / math.sqrt(sums[0] / (Hc * Wc)))
        out["ssim_y"] = sums[2] / positions
    return out


def image_metrics(sr_u8, gt_u8, crop_border):
    """PSNR, SSIM, PSNR_Y and SSIM_Y as the reference's test script computes them (codes/test.py:97-135) for uint8 images
    ``[B,H,W,C]`` (or one ``[H,W,C]``), C = 3 in BGR order or C = 1, tensors where the library computes:
    ``calculate_psnr`` and ``calculate_ssim`` (utils/util.py:646-697: the float64, valid-window, [0, 255]-scale "same as
    MATLAB" SSIM) of the images with ``crop_border`` pixels cut off every side (0: none), and of their BT.601 luma
    (``bgr2ycbcr(only_y=True)`` of the float image, data/util.py:199-213).  One kernel pass per call
    (``ops.image_metrics_u8``) and one read-back; the logarithms and divisions happen on the host.  Returns a list with one
    ``dict(psnr=, ssim=, psnr_y=, ssim_y=)`` of Python floats per frame (the dict itself for a single ``[H,W,C]`` image);
    a gray image has no ``_y`` entries.  ``psnr`` is ``inf`` for identical images.  This SSIM is not ``validate.ssim``'s
    number (``pytorch_ssim``: zero padding, fp32, [0, 1] tensors).  Fewer than 11 rows or columns inside the border raise
    ValueError (the reference returns NaN there)."""
    from . import ops
    if not (torch.is_tensor(sr_u8) and torch.is_tensor(gt_u8)):
        raise TypeError("image_metrics: sr_u8 and gt_u8 must be uint8 tensors")
    single = sr_u8.dim() == 3 and gt_u8.dim() == 3
    a, b = (sr_u8[None], gt_u8[None]) if single else (sr_u8, gt_u8)
    crop = int(crop_border)
    ssd, sums = ops.image_metrics_u8(a.contiguous(), b.contiguous(), crop)          # (checks dtypes, shapes and devices)
    B, H, W, C = a.shape
    ssd, sums = ssd.cpu().tolist(), sums.cpu().tolist()
    rows = [_figures(ssd[i], sums[i], H - 2 * crop, W - 2 * crop, C) for i in range(B)]
    return rows[0] if single else rows


def test_u8(net, frames, scale, crop_border=None, num_masks=10, fixed_range=False, use_graph=False, soft_masks=None,
            self_ensemble=False, names=None, results_file=None, soft_pair=False):
    """The loop of the reference's test script (codes/test.py:62-152) for a video source.  ``frames`` is what
    ``validate_u8`` takes: it yields ``(LQ, GT, Depth)`` with ``LQ`` a ``uint8`` ``[1,h,w,3]`` (or ``[h,w,3]``) BGR frame,
    ``GT`` the ``[1,3,sh,sw]`` float tensor and ``Depth`` ``[1,1,h,w]``; further items are ignored.  SR comes from
    ``video.FrameUpscaler`` (``num_masks`` ... ``self_ensemble`` and ``soft_pair`` are its arguments), GT is quantised by ``frame_emit_u8``
    as in ``validate_u8``, and every frame's four figures are ``image_metrics`` of the two uint8 images with
    ``crop_border`` pixels cropped (None: ``scale``, test.py:103; 0: no crop).  Nothing is read back per frame: the sums of
    ``ops.image_metrics_u8`` go into device chunks and come to the host in one transfer at the end.

    Returns ``dict(rows=[(name, psnr, ssim, psnr_y, ssim_y), ...], psnr=, ssim=, psnr_y=, ssim_y=, n=)``: the averages are
    the script's plain means (test.py:141-148; 0.0 without frames).  ``names``: one name per frame (default: the frame's
    index, six digits).  ``results_file``: a path that gets the script's tab-separated lines, one per frame and the
    ``Average`` line (test.py:133,152), six decimals."""
    from . import ops
    from .video import FrameUpscaler
    up = FrameUpscaler(net, num_masks=num_masks, fixed_range=fixed_range, use_graph=use_graph, min_max=(0, 1),
                       soft_masks=soft_masks, self_ensemble=self_ensemble, soft_pair=soft_pair)
    dev = up.device
    crop = int(scale) if crop_border is None else int(crop_border)
    CHUNK = 256
    chunks, shapes, labels = [], [], []  # int64 [4*CHUNK] each: ssd in the first quarter, the sums (float64 bits) behind it
    names = None if names is None else iter(names)

    def view(i):
        if i // CHUNK >= len(chunks):
            chunks.append(torch.zeros((4 * CHUNK,), dtype=torch.int64, device=dev))
        buf, j = chunks[i // CHUNK], i % CHUNK
        return buf[j:j + 1], buf[CHUNK:].view(torch.float64).view(CHUNK, 3)[j:j + 1]

    inf = float("inf")
    with torch.no_grad():
        for i, item in enumerate(frames):
            lq, gt, depth = item[0], item[1], item[2]
            lq = lq if torch.is_tensor(lq) else torch.from_numpy(np.ascontiguousarray(lq))
            sr_u8, _ = up.upscale_device(lq[None] if lq.dim() == 3 else lq, depth)     # on the device, nothing waited for
            gt = gt[:1].to(dev).float().contiguous()
            gt_u8 = ops.frame_emit_u8(ops.nchw_to_nhwc(gt), -inf, inf, (0, 1), swap_rb=True)
            ops.image_metrics_u8(sr_u8[:1].contiguous(), gt_u8, crop=crop, out=view(i))
            shapes.append(tuple(gt_u8.shape[1:]))
            labels.append("%06d" % i if names is None else str(next(names)))
    n = len(shapes)
    rows = []
    if n:
        host = (chunks[0] if len(chunks) == 1 else torch.cat(chunks)).cpu()      # the one read-back
        for i, (H, W, C) in enumerate(shapes):
            buf, j = host[4 * CHUNK * (i // CHUNK):4 * CHUNK * (i // CHUNK + 1)], i % CHUNK
            fig = _figures(int(buf[j]), buf[CHUNK:].view(torch.float64).view(CHUNK, 3)[j].tolist(), H - 2 * crop,
                           W - 2 * crop, C)
            rows.append((labels[i], fig["psnr"], fig["ssim"], fig["psnr_y"], fig["ssim_y"]))
    out = dict(rows=rows, n=n)
    for k, key in enumerate(("psnr", "ssim", "psnr_y", "ssim_y")):
        out[key] = sum(r[k + 1] for r in rows) / n if n else 0.0
    if results_file is not None:
        with open(results_file, "w") as fh:
            for r in rows:
                fh.write("{}\t{:.6f}\t{:.6f}\t{:.6f}\t{:.6f}\n".format(*r))
            if n:
                fh.write("Average\t{:.6f}\t{:.6f}\t{:.6f}\t{:.6f}\n".format(out["psnr"], out["ssim"], out["psnr_y"],
                                                                          out["ssim_y"]))
    return out
