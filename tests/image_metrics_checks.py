"""The test script's metrics on the device (csrc/metrics.hip: dasr_image_metrics_u8; ops.image_metrics_u8;
validate.image_metrics; validate.test_u8).  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_image_metrics.py runs them.

The yardstick is a float64 numpy restatement of the reference's functions (cv2 is not installed, so they cannot be imported):
``calculate_psnr`` (utils/util.py:646-653), ``ssim`` (utils/util.py:656-676), ``calculate_ssim`` (utils/util.py:679-697),
``bgr2ycbcr`` (data/util.py:199-213) and the data path of the test script around them (test.py:97-129: ``u8 / 255.``, crop,
``* 255``; the luma from ``bgr2ycbcr`` of the float image).  ``cv2.filter2D(img, -1, window)[5:-5, 5:-5]`` is a correlation
whose interior values do not depend on the border mode: restated as a valid correlation over ``sliding_window_view``.

GATE: |difference| <= 1e-9 on each of the four figures (absolute for SSIM, dB for PSNR).  Derived, not tuned: any fp64
summation order of a 121-term window moment of values <= 255^2 has error <= 121 * 2^-53 * 65025 ~ 9e-10, a variance term
therefore <~ 2e-9, against denominators >= C2 = 58.5: <~ 3e-10 on a map value; the relative error of the PSNR_Y sum is
<= n * 2^-53 << 1e-10 at these sizes.  Every check prints the maxima it measured (emulator and MI355X alike: 0 for PSNR,
3.4e-15 for SSIM, 7.1e-15 dB for PSNR_Y, 1.9e-14 for SSIM_Y - the last in the all-255-but-one-pixel case).

Sizes: the kernel's tile of the SSIM map is T_H x T_W = 16 x 32 (MT_H, MT_W of csrc/metrics.hip)."""
import math

import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view

from dasr_amd import _lib, ops, validate

GATE = 1e-9
T_H, T_W = 16, 32
E_UNSUPPORTED, E_WORKSPACE = -3, -4
FIGURES = ("psnr", "ssim", "psnr_y", "ssim_y")


# ---- the reference's functions, restated ----------------------------------------------------------------------------------
def gaussian_kernel():
    """cv2.getGaussianKernel(11, 1.5) as a float64 column (utils/util.py:662)."""
    k = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (k / k.sum()).reshape(11, 1)


def _filter_valid(img, window):
    """cv2.filter2D(img, -1, window)[5:-5, 5:-5] (utils/util.py:665): every channel by itself."""
    return np.einsum("ij...kl,kl->ij...", sliding_window_view(img, (11, 11), axis=(0, 1)), window)


def ref_calculate_psnr(img1, img2):
    """utils/util.py:646-653."""
    img1 = img1.astype(np.float64)
    img2 = img2.astype(np.float64)
    mse = np.mean((img1 - img2) ** 2)
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))


def ref_ssim(img1, img2):
    """utils/util.py:656-676."""
    C1 = (0.01 * 255) ** 2
    C2 = (0.03 * 255) ** 2
    img1 = img1.astype(np.float64)
    img2 = img2.astype(np.float64)
    kernel = gaussian_kernel()
    window = np.outer(kernel, kernel.transpose())
    mu1 = _filter_valid(img1, window)
    mu2 = _filter_valid(img2, window)
    mu1_sq = mu1 ** 2
    mu2_sq = mu2 ** 2
    mu1_mu2 = mu1 * mu2
    sigma1_sq = _filter_valid(img1 ** 2, window) - mu1_sq
    sigma2_sq = _filter_valid(img2 ** 2, window) - mu2_sq
    sigma12 = _filter_valid(img1 * img2, window) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean()


def ref_calculate_ssim(img1, img2):
    """utils/util.py:679-697."""
    if not img1.shape == img2.shape:
        raise ValueError("Input images must have the same dimensions.")
    if img1.ndim == 2:
        return ref_ssim(img1, img2)
    if img1.ndim == 3:
        if img1.shape[2] == 3:
            return np.array([ref_ssim(img1, img2) for _ in range(3)]).mean()
        if img1.shape[2] == 1:
            return ref_ssim(np.squeeze(img1), np.squeeze(img2))
    raise ValueError("Wrong input image dimensions.")


def ref_bgr2ycbcr_y(img):
    """data/util.py:199-213 with only_y=True for a float image in [0, 1] (its `img *= 255.` on a copy)."""
    assert img.dtype == np.float64
    rlt = np.dot(img * 255., [24.966, 128.553, 65.481]) / 255.0 + 16.0
    rlt /= 255.
    return rlt


def ref_figures(sr_u8, gt_u8, crop_border):
    """test.py:97-129 with the four calls as written behind its comment signs, for uint8 [H,W,C] images."""
    gt_img = gt_u8 / 255.
    sr_img = sr_u8 / 255.
    c = crop_border
    cut = (lambda x: x) if c == 0 else (lambda x: x[c:-c, c:-c])
    out = dict(psnr=ref_calculate_psnr(cut(sr_img) * 255, cut(gt_img) * 255),
               ssim=float(ref_calculate_ssim(cut(sr_img) * 255, cut(gt_img) * 255)))
    if gt_img.shape[2] == 3:
        sr_y, gt_y = ref_bgr2ycbcr_y(sr_img), ref_bgr2ycbcr_y(gt_img)
        out["psnr_y"] = ref_calculate_psnr(cut(sr_y) * 255, cut(gt_y) * 255)
        out["ssim_y"] = float(ref_calculate_ssim(cut(sr_y) * 255, cut(gt_y) * 255))
    return out


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _dev(x, device, off=0):
    """``x`` on ``device``; ``off`` > 0: as a slice that starts ``off`` bytes into a larger buffer."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if off == 0:
        return t.to(device)
    buf = torch.zeros((t.numel() + off + 5,), dtype=torch.uint8, device=device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == off % 4
    return v


def _diff(got, want):
    if math.isinf(got) or math.isinf(want):
        return 0.0 if got == want else float("inf")
    return abs(got - want)


def _compare(a, b, crop, device, worst, tag, off_b=0):
    """image_metrics of the uint8 batches against the restatement, frame by frame; the ssd against numpy and frame_ssd_u8."""
    B, H, W, C = a.shape
    ad, bd = _dev(a, device), _dev(b, device, off_b)
    ssd, sums = ops.image_metrics_u8(ad, bd, crop)
    assert ssd.dtype == torch.int64 and tuple(ssd.shape) == (B,) and sums.dtype == torch.float64 and tuple(sums.shape) == (B, 3)
    ac, bc = a[:, crop:H - crop, crop:W - crop].astype(np.int64), b[:, crop:H - crop, crop:W - crop].astype(np.int64)
    want_ssd = ((ac - bc) ** 2).reshape(B, -1).sum(axis=1)
    assert np.array_equal(ssd.cpu().numpy(), want_ssd), (tag, ssd, want_ssd)
    assert torch.equal(ssd, ops.frame_ssd_u8(ad, bd.contiguous(), crop)), tag
    got = validate.image_metrics(ad, bd, crop)
    assert len(got) == B
    for i in range(B):
        want = ref_figures(a[i], b[i], crop)
        assert set(got[i]) == set(want) == set(FIGURES[:4 if C == 3 else 2]), (tag, got[i])
        for k, v in want.items():
            assert isinstance(got[i][k], float)
            d = _diff(got[i][k], v)
            worst[k] = max(worst.get(k, 0.0), d)
            assert d <= GATE, (tag, i, k, got[i][k], v, d)
    return got


def _noisy(gen, shape, levels):
    """GT and SR = GT + bounded integer noise, clipped; one noise level per frame."""
    gt = gen.integers(0, 256, size=shape, dtype=np.uint8)
    sr = np.stack([np.clip(gt[i].astype(np.int64) + gen.integers(-lv, lv + 1, size=shape[1:]), 0, 255).astype(np.uint8)
                   for i, lv in enumerate(levels)])
    return sr, gt


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def check_against_restatement(device):
    """C = 3, B = 3; SSIM-map heights 1, T-1, T, T+1, 2T+3 times the same widths (1 x 1: an 11 x 11 cropped image); crop
    0, 3 and 8 in turn.  H = map height + 10 + 2 crop: odd wherever the map extent is, and for the two even extents (T_H, T_W)
    the crop is chosen so that H / W is no multiple of 4.  Two cases hand `b` over 1 and 3 bytes off the dword grid."""
    gen = np.random.default_rng(41)
    worst, cases, n = {}, 0, 0
    crops_seen, shapes = set(), []
    for hm in (1, T_H - 1, T_H, T_H + 1, 2 * T_H + 3):
        for wm in (1, T_W - 1, T_W, T_W + 1, 2 * T_W + 3):
            crop = (0, 3, 8)[n % 3]
            n += 1
            if (hm + 10 + 2 * crop) % 4 == 0 or (wm + 10 + 2 * crop) % 4 == 0:
                crop = 8 if crop == 3 else 0
            H, W = hm + 10 + 2 * crop, wm + 10 + 2 * crop
            assert H % 4 and W % 4 and (H % 2 or hm == T_H) and (W % 2 or wm == T_W)
            sr, gt = _noisy(gen, (3, H, W, 3), (2, 12, 60))
            off_b = {(T_H + 1, T_W - 1): 1, (2 * T_H + 3, 2 * T_W + 3): 3}.get((hm, wm), 0)
            got = _compare(sr, gt, crop, device, worst, (H, W, crop), off_b)
            assert got[0]["psnr"] > got[1]["psnr"] > got[2]["psnr"] and got[0]["ssim_y"] > got[2]["ssim_y"]
            crops_seen.add(crop)
            shapes.append((H, W, crop))
            cases += 1
    assert crops_seen == {0, 3, 8}
    return dict(cases=cases, worst=worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. flat and extreme images
# ---------------------------------------------------------------------------------------------------------------------
def check_flat_and_extreme(device):
    """All 0 against all 255; all 255 against all 255 with one pixel 254 (E[x^2] - mu^2 cancels at 65025: the worst case
    for the moments); a frame whose R channel is saturated in both images."""
    gen = np.random.default_rng(42)
    worst = {}
    for (H, W), crop in (((29, 37), 0), ((31, 53), 3)):
        a = np.zeros((3, H, W, 3), dtype=np.uint8)
        b = np.full((3, H, W, 3), 255, dtype=np.uint8)
        a[1] = 255
        a[1, H // 2, W // 2, 0] = 254
        sr, gt = _noisy(gen, (1, H, W, 3), (9,))
        a[2], b[2] = sr[0], gt[0]
        a[2, :, :, 2] = b[2, :, :, 2] = 255
        got = _compare(a, b, crop, device, worst, ("flat", H, W, crop))
        assert got[0]["psnr"] == 0.0 and got[0]["ssim"] < 1e-3                 # 20 log10(255 / 255)
        assert got[1]["ssim"] > 0.99 and math.isfinite(got[1]["psnr_y"])
    return dict(worst=worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. identical images
# ---------------------------------------------------------------------------------------------------------------------
def check_identical(device):
    gen = np.random.default_rng(43)
    worst = 0.0
    for shape, crop in (((2, 27, 45, 3), 0), ((1, 43, 29, 3), 8)):
        a = gen.integers(0, 256, size=shape, dtype=np.uint8)
        ad, bd = _dev(a, device), _dev(a.copy(), device)
        ssd, sums = ops.image_metrics_u8(ad, bd, crop)
        assert ssd.cpu().tolist() == [0] * shape[0]
        assert sums[:, 0].cpu().tolist() == [0.0] * shape[0]
        for fig in validate.image_metrics(ad, bd, crop):
            assert fig["psnr"] == float("inf") and fig["psnr_y"] == float("inf")
            worst = max(worst, abs(fig["ssim"] - 1.0), abs(fig["ssim_y"] - 1.0))
            assert abs(fig["ssim"] - 1.0) <= GATE and abs(fig["ssim_y"] - 1.0) <= GATE, fig
    return dict(worst_ssim_minus_1=worst)


# ---------------------------------------------------------------------------------------------------------------------
# 4. gray images
# ---------------------------------------------------------------------------------------------------------------------
def check_gray(device):
    gen = np.random.default_rng(44)
    worst = {}
    for (H, W), crop in (((27, 45), 0), ((T_H + 17, 2 * T_W + 19), 3)):
        sr, gt = _noisy(gen, (2, H, W, 1), (3, 30))
        got = _compare(sr, gt, crop, device, worst, ("gray", H, W, crop))
        assert all(set(g) == {"psnr", "ssim"} for g in got)
        _, sums = ops.image_metrics_u8(_dev(sr, device), _dev(gt, device), crop)
        assert sums[:, 0].cpu().tolist() == [0.0, 0.0] and sums[:, 2].cpu().tolist() == [0.0, 0.0]
        assert set(validate.image_metrics(_dev(sr[0], device), _dev(gt[0], device), crop)) == {"psnr", "ssim"}
    return dict(worst=worst)


# ---------------------------------------------------------------------------------------------------------------------
# 5. alone, in a batch, again
# ---------------------------------------------------------------------------------------------------------------------
def _bits(ssd, sums):
    return ssd.cpu().tolist(), sums.cpu().contiguous().view(torch.int64).tolist()


def check_batch_and_repeat(device):
    gen = np.random.default_rng(45)
    H, W, crop = T_H + 19, 2 * T_W + 15, 3                     # 2 x 3 tiles per frame
    sr, gt = _noisy(gen, (3, H, W, 3), (5, 20, 50))
    alone = _bits(*ops.image_metrics_u8(_dev(sr[:1], device), _dev(gt[:1], device), crop))
    assert alone[0][0] > 0 and all(v != 0 for v in alone[1][0])
    for order in ((0, 1, 2), (1, 2, 0)):
        pos = order.index(0)
        ad, bd = _dev(sr[list(order)], device), _dev(gt[list(order)], device)
        first = _bits(*ops.image_metrics_u8(ad, bd, crop))
        assert ([first[0][pos]], [first[1][pos]]) == alone, order
        assert _bits(*ops.image_metrics_u8(ad, bd, crop)) == first, order          # the call repeated
        # caller-owned slices: the results land there and nowhere else
        ssd_buf = torch.full((5,), -7, dtype=torch.int64, device=device)
        sums_buf = torch.full((5, 3), -7.0, dtype=torch.float64, device=device)
        r = ops.image_metrics_u8(ad, bd, crop, out=(ssd_buf[1:4], sums_buf[1:4]))
        assert r[0].data_ptr() == ssd_buf[1:4].data_ptr() and _bits(ssd_buf[1:4], sums_buf[1:4]) == first
        assert ssd_buf[[0, 4]].cpu().tolist() == [-7, -7] and sums_buf[[0, 4]].cpu().flatten().tolist() == [-7.0] * 6
    return dict(ssd=alone[0][0])


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def check_refusals(device):
    """C = 2, Hc = 10, 2 crop >= H and a workspace one byte short: the library's code, the results and the workspace
    untouched (nothing was launched); the Python layers raise ValueError."""
    lib = _lib.get()
    p64 = lambda t: _lib.ptr(t, dtype=torch.int64)                                              # noqa: E731
    pf64 = lambda t: _lib.ptr(t, dtype=torch.float64)                                           # noqa: E731
    need = int(lib.dasr_image_metrics_u8_workspace(2, 21, 23, 3, 0))
    assert need > 0 and need % 8 == 0
    cases = dict(c2=((2, 21, 23, 2, 0), E_UNSUPPORTED, need), hc10=((2, 16, 23, 3, 3), E_UNSUPPORTED, need),
                 wc10=((2, 21, 20, 3, 5), E_UNSUPPORTED, need), crop_ge_h=((2, 21, 23, 3, 11), E_UNSUPPORTED, need),
                 workspace=((2, 21, 23, 3, 0), E_WORKSPACE, need - 1))
    for name, ((B, H, W, C, crop), code, nbytes) in cases.items():
        if code == E_UNSUPPORTED:
            assert int(lib.dasr_image_metrics_u8_workspace(B, H, W, C, crop)) == 0, name
        a = torch.zeros((B, H, W, C), dtype=torch.uint8, device=device)
        ssd = torch.full((B,), -7, dtype=torch.int64, device=device)
        sums = torch.full((B, 3), -7.0, dtype=torch.float64, device=device)
        ws = torch.full((need // 8,), -7, dtype=torch.int64, device=device)
        rc = lib.dasr_image_metrics_u8(ops._pu8(a), ops._pu8(a), p64(ssd), pf64(sums), p64(ws), nbytes, B, H, W, C, crop,
                                       _lib.stream())
        assert rc == code, (name, rc)
        assert ssd.cpu().tolist() == [-7] * B and sums.cpu().flatten().tolist() == [-7.0] * (3 * B), name
        assert ws.cpu().tolist() == [-7] * (need // 8), name
        if code == E_UNSUPPORTED:
            for fn in (lambda: ops.image_metrics_u8(a, a, crop), lambda: validate.image_metrics(a, a, crop)):
                try:
                    fn()
                    raise AssertionError("%s accepted" % name)
                except ValueError:
                    pass
    return dict(cases=len(cases))


# ---------------------------------------------------------------------------------------------------------------------
# 7. validate.test_u8
# ---------------------------------------------------------------------------------------------------------------------
# On the emulator a forward of the x2 net with depth blocks costs seconds whatever the frame size; there the check runs on
# the same x2 nb = 4 trunk without depth blocks (tests/video_checks.py: X2_LIGHT), on the MI355X with all four.
X2_16 = dict(name="x2_nb4", scale=2, which=[0, 1, 2, 3], L=32, nb=4, B=1, H=16, W=20)
X2_16_LIGHT = dict(X2_16, name="x2_nb4_light", which=[])
X4 = dict(name="x4_nb4", scale=4, which=[0, 1], L=32, nb=4, B=1, H=12, W=16)


def _source(case, n, seed):
    """n items (uint8 BGR LQ frame [1,h,w,3], GT [1,3,sh,sw] float, depth [1,1,h,w]) as validate_u8 / test_u8 take them."""
    from dasr_amd import synth
    items = []
    for i in range(n):
        lq, gt, dm, _ = synth.seeded_batch(seed + i, 1, case["H"], case["W"], case["scale"])
        items.append((validate.tensor2img(lq[0])[None], gt, dm))
    return items


def _rows_by_hand(net, items, crop, device, names, **upscaler):
    """The rows from FrameUpscaler's output and frame_emit_u8's GT through validate.image_metrics, frame by frame."""
    from dasr_amd.video import FrameUpscaler
    up = FrameUpscaler(net, use_graph=False, **upscaler)
    inf = float("inf")
    rows = []
    for name, (f, gt, dm) in zip(names, items):
        sr_u8 = torch.from_numpy(up.upscale(f, dm)).to(device)
        gt_u8 = ops.frame_emit_u8(ops.nchw_to_nhwc(gt.to(device).float().contiguous()), -inf, inf, (0, 1), swap_rb=True)
        fig = validate.image_metrics(sr_u8, gt_u8, crop)[0]
        rows.append((name,) + tuple(fig[k] for k in FIGURES))
    return rows


def _means_ok(res):
    n = len(res["rows"])
    assert res["n"] == n
    for k, key in enumerate(FIGURES):
        assert res[key] == sum(r[k + 1] for r in res["rows"]) / n, key                 # test.py:141-148


def check_test_u8(device):
    import os
    import tempfile
    from tests import video_checks as vc
    case = X2_16 if device == "cuda" else X2_16_LIGHT
    net, _ = vc._net(case, device)
    s = case["scale"]
    items = _source(case, 3, 300)
    names = ["img_%d" % i for i in range(3)]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "results.txt")
        res = validate.test_u8(net, iter(items), s, names=names, results_file=path)      # crop_border=None: the scale
        lines = open(path).read().split("\n")
    assert net.training
    want = _rows_by_hand(net, items, s, device, names)
    assert res["rows"] == want, (res["rows"], want)                                       # exactly
    _means_ok(res)
    assert all(math.isfinite(v) for r in res["rows"] for v in r[1:])
    assert len({r[1] for r in res["rows"]}) == 3                                          # three different frames
    # the file: test.py:133 per frame, test.py:152 at the end, six decimals
    assert lines[-1] == "" and len(lines) == 5
    for line, row in zip(lines[:3], res["rows"]):
        cells = line.split("\t")
        assert cells[0] == row[0] and cells[1:] == ["%.6f" % v for v in row[1:]], (line, row)
        assert all(abs(float(c) - v) <= 0.5e-6 for c, v in zip(cells[1:], row[1:]))
    assert lines[3].split("\t") == ["Average"] + ["%.6f" % res[k] for k in FIGURES]
    # crop_border=None is crop_border=scale; default names are the frame index.  (A forward takes a second on the emulator:
    # one frame there, all three on the MI355X - and there another border as well: the crop is part of the figures.)
    k = 3 if device == "cuda" else 1
    same = validate.test_u8(net, iter(items[:k]), s, crop_border=s)
    assert [r[0] for r in same["rows"]] == ["%06d" % i for i in range(k)]
    assert [r[1:] for r in same["rows"]] == [r[1:] for r in res["rows"][:k]]
    if device == "cuda":
        other = validate.test_u8(net, iter(items), s, crop_border=0, names=names)
        assert other["rows"] != res["rows"] and other["rows"] == _rows_by_hand(net, items, 0, device, names)
    assert validate.test_u8(net, iter([]), s) == dict(rows=[], n=0, psnr=0.0, ssim=0.0, psnr_y=0.0, ssim_y=0.0)
    return dict(psnr=res["psnr"], ssim=res["ssim"], psnr_y=res["psnr_y"], ssim_y=res["ssim_y"])


def check_test_u8_options(device):
    """GPU only.  One x4 net, two frames: self_ensemble=True gives the rows of validate.test_x8's images; use_graph=True the
    eager rows - the two frames are handed over twice, so that the second pass is the capture and a replay (the first two
    calls of a shape run eagerly)."""
    from tests import video_checks as vc
    from dasr_amd import prep
    case = X4
    net, _ = vc._net(case, device)
    s = case["scale"]
    items = _source(case, 2, 400)
    eager = validate.test_u8(net, iter(items), s)
    assert [r[1:] for r in eager["rows"]] == [r[1:] for r in _rows_by_hand(net, items, s, device, "ab")]
    graph = validate.test_u8(net, iter(items + items), s, use_graph=True)
    assert graph["n"] == 4 and graph["rows"][:2] == eager["rows"]
    assert [r[1:] for r in graph["rows"][2:]] == [r[1:] for r in eager["rows"]]
    _means_ok(graph)
    ens = validate.test_u8(net, iter(items), s, self_ensemble=True)
    assert [r[1:] for r in ens["rows"]] == [r[1:] for r in _rows_by_hand(net, items, s, device, "ab", self_ensemble=True)]
    inf = float("inf")
    for row, (f, gt, dm) in zip(ens["rows"], items):      # and from test_x8 itself, through tensor2img on the host
        dd = dm.to(device)
        sr = validate.test_x8(net, vc.img2tensor(f[0])[None].to(device), dd, prep.depth_to_masks(dd, 10))
        sr_img = torch.from_numpy(validate.tensor2img(sr[0])[None]).to(device)
        gt_img = torch.from_numpy(validate.tensor2img(gt[0])[None]).to(device)
        fig = validate.image_metrics(sr_img, gt_img, s)[0]
        assert row[1:] == tuple(fig[k] for k in FIGURES)
    assert ens["rows"] != eager["rows"]
    soft = validate.test_u8(net, iter(items), s, soft_masks=0.5, fixed_range=True)
    assert soft["rows"] != eager["rows"] and soft["n"] == 2
    return dict(eager=eager["psnr"], ensemble=ens["psnr"], soft=soft["psnr"])
