"""Video inference (csrc/frame.hip: dasr_frame_ingest_u8 / dasr_frame_emit_u8 / dasr_frame_ssd_u8; graph.depthnet_infer_nhwc;
video.FrameUpscaler; validate.validate_u8).  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_video.py runs them.

The kernel checks are exact (== on bytes / bits): the three kernels restate integer or correctly rounded fp32 formulas of the
reference (img2tensor, tensor2img, calculate_psnr's mse).  The whole-path checks are exact too where both sides run the same
kernels (FrameUpscaler against validate.test + tensor2img: only layout passes differ); against the CPU oracle a pixel may
differ by one level, and only where the oracle's value lies within the forward gate of a rounding boundary."""
import functools
import math

import numpy as np
import torch

from dasr_amd import _lib, ops, prep, synth, validate
from dasr_amd.video import FrameUpscaler
from oracle import depthnet_oracle as O
from tests.golden_cases import DEPTHNET_CASES
from tests.parity_checks import build_net

E_UNSUPPORTED = -3
# the issue's shapes (B, H, W): 105 bytes per 3-channel frame (frame bases off the dword grid, a tail), one pixel, a multiple of
# everything; ALL holds every byte value in every channel / every special value at once (969 = 12 * 80 + 9 bytes: a tail too)
SHAPES = [(2, 5, 7), (1, 1, 1), (3, 4, 16)]
X2 = next(c for c in DEPTHNET_CASES if c["name"] == "x2_nb4")      # the smallest x2 / x8 nets the golden cases build
X8 = next(c for c in DEPTHNET_CASES if c["name"] == "x8_nb4")
FWD_GATE = 2e-4                      # parity_checks._compare_with_oracle's forward gate for these configurations


def img2tensor(img):
    """The reference's formula (utils/util.py:596-605): BGR uint8 HWC -> RGB float CHW."""
    img = img.astype(np.float32) / 255.
    img = img[:, :, [2, 1, 0]]
    return torch.from_numpy(np.ascontiguousarray(np.transpose(img, (2, 0, 1)))).float()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _offset_view(t, off, device):
    """A contiguous copy of ``t`` on ``device`` whose storage starts ``off`` elements into an allocation."""
    buf = torch.empty((t.numel() + off,), dtype=t.dtype, device=device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# 1. ingest
# ---------------------------------------------------------------------------------------------------------------------
def check_ingest_u8(device):
    gen = np.random.default_rng(11)
    cases = 0
    for C in (3, 1):
        frames = [gen.integers(0, 256, size=(B, H, W, C), dtype=np.uint8) for (B, H, W) in SHAPES]
        allv = np.zeros((1, 17, 19, C), dtype=np.uint8)           # every byte value in every channel (7 is a unit mod 256)
        p = np.arange(17 * 19)
        for c in range(C):
            allv[0, :, :, c] = ((p * 7 + 85 * c) % 256).reshape(17, 19)
            assert len(set(allv[0, :, :, c].ravel().tolist())) == 256
        for x in frames + [allv]:
            for swap in (True, False):
                want = x.astype(np.float32) / 255.
                if swap and C == 3:
                    want = want[..., ::-1]
                # aligned buffers; both buffers 3 elements into an allocation (a real head: 9 elements with the swap, 1
                # without); only the source off the grid (no aligned group exists: the scalar path takes everything)
                for off_in, off_out in ((0, 0), (3, 3), (1, 0)):
                    xd = _offset_view(torch.from_numpy(x), off_in, device)
                    out = _offset_view(torch.full(x.shape, -1.0), off_out, device)
                    got = ops.frame_ingest_u8(xd, swap_rb=swap, out=out).cpu().numpy()
                    assert np.array_equal(_bits(got), _bits(want)), (x.shape, swap, off_in, off_out)
                    cases += 1
                if C == 3 and swap:                               # permuted to NCHW: the reference's img2tensor
                    got = ops.frame_ingest_u8(torch.from_numpy(x).to(device), swap_rb=True).cpu()
                    for b in range(x.shape[0]):
                        assert torch.equal(got[b].permute(2, 0, 1).contiguous().view(torch.int32),
                                           img2tensor(x[b]).view(torch.int32)), (x.shape, b)
    return dict(cases=cases)


# ---------------------------------------------------------------------------------------------------------------------
# 2. emit
# ---------------------------------------------------------------------------------------------------------------------
def _specials():
    """Every rounding tie (k + 0.5) / 255 as fp32 with its two fp32 neighbours, mapped into each of the three ranges of the
    check; exact 0, -0.0, 1, nextafter(1, 2); values outside every range; +-1e30; denormals."""
    k = np.arange(255, dtype=np.float64)
    out = []
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (0.1, 0.9)):
        t = (lo + (hi - lo) * (k + 0.5) / 255.0).astype(np.float32)
        out += [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))]
    one = np.float32(1.0)
    out.append(np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(2.0)), np.nextafter(one, np.float32(0.0)), -1.0,
                         np.nextafter(-one, np.float32(-2.0)), 0.1, 0.9, -0.5, 1.5, -2.0, 3.0, 1e30, -1e30, 1e-40, -1e-40,
                         1e-45, -1e-45, 0.5, 0.25], dtype=np.float32))
    return np.concatenate(out).astype(np.float32)


def _t2i(chw, min_max):
    """validate.tensor2img of one [C,H,W] image.  Its squeeze() would drop a height or width of 1 together with the batch
    axis; such an image goes in tiled to twice its size and the first copy is cut back out (the function is per sample)."""
    C, H, W = chw.shape
    if H == 1 or W == 1:
        return validate.tensor2img(chw.repeat(1, 2, 2), min_max=min_max)[:H, :W]
    return validate.tensor2img(chw, min_max=min_max)


def check_emit_u8(device):
    gen = np.random.default_rng(12)
    sp = _specials()
    cases = 0
    for C, big in ((3, (1, 31, 29)), (1, (1, 53, 51))):
        assert big[1] * big[2] * C >= sp.size
        for (B, H, W) in SHAPES + [big]:
            n = B * H * W * C
            y = gen.uniform(-1.3, 1.3, size=n).astype(np.float32)
            pick = gen.permutation(sp)[:n] if n < sp.size else sp           # the big shape holds every special value
            y[gen.permutation(n)[:pick.size]] = pick
            y = torch.from_numpy(y.reshape(B, H, W, C))
            for (lo, hi), mm in (((0, 1), (0, 1)), ((-1, 1), (-1, 1)), ((0, 1), (0.1, 0.9))):
                yd = y.to(device)
                ref = ops.clamp_to_nchw(yd, lo, hi).cpu()
                for off_in, off_out in ((0, 0), (3, 3), (0, 1)):
                    out = _offset_view(torch.zeros((B, H, W, C), dtype=torch.uint8), off_out, device)
                    got = ops.frame_emit_u8(_offset_view(y, off_in, device), lo, hi, mm, swap_rb=True, out=out).cpu().numpy()
                    for b in range(B):
                        want = _t2i(ref[b], mm)
                        assert want.dtype == np.uint8
                        assert np.array_equal(got[b] if C == 3 else got[b, :, :, 0], want), (C, (B, H, W), lo, hi, mm, b)
                    cases += 1
    # A NaN pixel: a uint8 cannot carry it.  The emit's first clamp is fminf(fmaxf(y, net_lo), net_hi), which returns net_lo
    # for NaN, so the pixel leaves as the byte of a pixel that holds net_lo (ops.clamp_to_nchw, the float path, keeps the
    # NaN as torch.clamp does).  NaNs in the scalar head, in the vector body and in the last element.
    for (lo, hi), mm in (((0, 1), (0, 1)), ((-1, 1), (-1, 1)), ((0.25, 1), (0, 1))):
        y = torch.from_numpy(gen.uniform(-1.3, 1.3, size=(1, 7, 9, 3)).astype(np.float32))
        twin = y.clone()
        for pos in (0, 1, 17, 100, y.numel() - 1):
            y.view(-1)[pos] = float("nan")
            twin.view(-1)[pos] = lo
        for off_in in (0, 3):
            got = ops.frame_emit_u8(_offset_view(y, off_in, device), lo, hi, mm, swap_rb=False).cpu()
            want = ops.frame_emit_u8(_offset_view(twin, off_in, device), lo, hi, mm, swap_rb=False).cpu()
            assert torch.equal(got, want), ("NaN pixel", lo, hi, mm, off_in)
            byte = int(round((min(max(lo, mm[0]), mm[1]) - mm[0]) / (mm[1] - mm[0]) * 255.0))
            assert got.view(-1)[[0, 1, 17, 100, y.numel() - 1]].tolist() == [byte] * 5, ("NaN pixel byte", lo, hi, mm, byte)
            cases += 1
    y2 = torch.zeros((1, 4, 4, 2), device=device)
    o2 = torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device=device)
    rc = _lib.get().dasr_frame_emit_u8(ops._p(y2), ops._pu8(o2), 1, 4, 4, 2, 0.0, 1.0, 0.0, 1.0, 1, _lib.stream())
    assert rc == E_UNSUPPORTED, rc
    return dict(cases=cases, specials=int(sp.size))


# ---------------------------------------------------------------------------------------------------------------------
# 3. sum of squared differences
# ---------------------------------------------------------------------------------------------------------------------
def _psnr_from_ssd(ssd, n):
    return float("inf") if ssd == 0 else 20 * math.log10(255.0 / math.sqrt(ssd / n))


def check_ssd_u8(device):
    gen = np.random.default_rng(13)
    cases = 0
    for (H, W) in ((9, 11), (40, 48)):
        for C in (3, 1):
            a = gen.integers(0, 256, size=(2, H, W, C), dtype=np.uint8)
            pairs = dict(random=(a, gen.integers(0, 256, size=a.shape, dtype=np.uint8)), identical=(a, a.copy()),
                         extremes=(np.zeros_like(a), np.full_like(a, 255)))
            for name, (x, z) in pairs.items():
                for crop in (0, 2, 4):
                    got = ops.frame_ssd_u8(torch.from_numpy(x).to(device), torch.from_numpy(z).to(device), crop).cpu().numpy()
                    xc, zc = x[:, crop:H - crop, crop:W - crop], z[:, crop:H - crop, crop:W - crop]
                    want = ((xc.astype(np.int64) - zc.astype(np.int64)) ** 2).reshape(2, -1).sum(axis=1)
                    assert got.dtype == np.int64 and np.array_equal(got, want), (name, H, W, C, crop, got, want)
                    for b in range(2):
                        ps, ps_ref = _psnr_from_ssd(int(got[b]), xc[b].size), validate.calculate_psnr(xc[b], zc[b])
                        if name == "identical":
                            assert ps == float("inf") and ps_ref == float("inf")
                        else:
                            assert abs(ps - ps_ref) <= 1e-12, (name, H, W, C, crop, ps, ps_ref)
                    cases += 1
    a = torch.zeros((2, 9, 11, 3), dtype=torch.uint8, device=device)
    out = torch.zeros((2,), dtype=torch.int64, device=device)
    ws = torch.zeros((64,), dtype=torch.int64, device=device)
    p64 = lambda t: _lib.ptr(t, dtype=torch.int64)                                              # noqa: E731
    rc = _lib.get().dasr_frame_ssd_u8(ops._pu8(a), ops._pu8(a), p64(out), p64(ws), 512, 2, 9, 11, 3, 5, _lib.stream())
    assert rc == E_UNSUPPORTED, rc
    return dict(cases=cases)


def check_ssd_u8_large(device):
    """One 1024 x 1280 x 3 frame, all 0 against all 255: 255^2 * 3 932 160 = 2.56e11 needs the 64-bit partials and sum."""
    a = torch.zeros((1, 1024, 1280, 3), dtype=torch.uint8, device=device)
    b = torch.full((1, 1024, 1280, 3), 255, dtype=torch.uint8, device=device)
    got = int(ops.frame_ssd_u8(a, b, 0).cpu()[0])
    assert got == 255 * 255 * 3932160, got
    return dict(ssd=got)


# ---------------------------------------------------------------------------------------------------------------------
# whole path
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_for(h, w, B, seed):
    """Random uint8 BGR frames [B,h,w,3] and a random depth map in [0,1) [B,1,h,w]; computed once per key, never modified."""
    gen = np.random.default_rng(1000 + seed)
    f = gen.integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    d = torch.from_numpy(gen.random(size=(B, 1, h, w), dtype=np.float32))
    return f, d


def _net(case, device, dtype=torch.float32):
    net, cfg = build_net(case, device)
    net.set_compute_dtype(dtype)
    return net, cfg


def _via_validate(net, f, d, device, min_max=(0, 1)):
    """The path as it was: host img2tensor, fp32 upload, validate.test, fp32 download, tensor2img per frame."""
    lq = torch.stack([img2tensor(f[b]) for b in range(f.shape[0])]).to(device)
    dd = d.to(device)
    sr = validate.test(net, lq, dd, prep.depth_to_masks(dd, 10))
    return np.stack([validate.tensor2img(sr[b], min_max=min_max) for b in range(f.shape[0])])


def check_upscaler_matches_validate(device):
    configs = [(X2, torch.float32)] if device == "cpu" else \
        [(X2, torch.float32), (X8, torch.float32), (X2, torch.bfloat16), (X8, torch.bfloat16)]
    out = {}
    for case, dtype in configs:
        net, _ = _net(case, device, dtype)
        up = FrameUpscaler(net, use_graph=False)
        for B in (1, 2):
            f, d = frames_for(case["H"], case["W"], B, B)
            got = up.upscale(f, d)
            want = _via_validate(net, f, d, device)
            assert got.dtype == np.uint8 and got.shape == want.shape == (B, case["scale"] * case["H"], case["scale"] * case["W"], 3)
            assert np.array_equal(got, want), (case["name"], dtype, B, int((got != want).sum()))
            interior = float(((got > 0) & (got < 255)).mean())
            assert interior > 0.2, interior            # the comparison is not one of saturated images
            out["%s/%s/B%d" % (case["name"], str(dtype).split(".")[-1], B)] = interior
        assert net.training                            # the upscaler leaves the module's mode alone
    return out


def check_upscaler_vs_oracle(device):
    net, cfg = _net(X8, device)
    f, d = frames_for(X8["H"], X8["W"], 2, 7)
    got = FrameUpscaler(net, use_graph=False).upscale(f, d)
    lq = torch.stack([img2tensor(f[b]) for b in range(2)])
    mk = prep.depth_to_masks(d.to(device), 10).cpu()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = O.depthnet_forward(sd, cfg, lq, d, mk)
    differing = total = 0
    for b in range(2):
        want = validate.tensor2img(ref[b])
        diff = np.abs(got[b].astype(np.int64) - want.astype(np.int64))
        assert diff.max() <= 1, int(diff.max())
        v = np.transpose(ref[b].double().clamp(0, 1).numpy()[[2, 1, 0]], (1, 2, 0)) * 255.0     # the oracle's value, BGR HWC
        off_half = np.abs(v - np.floor(v) - 0.5)                                                 # distance to a half-integer
        assert (off_half[diff > 0] <= 255.0 * FWD_GATE).all(), float(off_half[diff > 0].max())
        differing += int((diff > 0).sum())
        total += diff.size
    print("upscaler vs oracle: %d of %d samples differ by one level (%.4f %%)" % (differing, total, 100.0 * differing / total))
    return dict(differing=differing, total=total)


def check_graph_replay(device):
    case = X2
    net, _ = _net(case, device)
    up_g = FrameUpscaler(net, use_graph=True)
    up_e = FrameUpscaler(net, use_graph=False)
    h, w = case["H"], case["W"]
    seq = [frames_for(h, w, 1, 20 + i) for i in range(5)]
    for i, (f, d) in enumerate(seq):
        got = up_g.upscale(f, d)
        assert np.array_equal(got, up_e.upscale(f, d)), i
        assert up_g.replays == max(0, i - 1), (i, up_g.replays)          # two eager calls, then a replay per call
    assert up_g.captures == 1
    before = got
    # an in-place parameter edit: the captured graph holds the folded kernels of the old value and must not be replayed
    with torch.no_grad():
        net.get_parameter("conv_output.weight").mul_(1.5)
    f, d = seq[4]
    replays = up_g.replays
    after = up_g.upscale(f, d)
    assert up_g.replays == replays                                       # back in the warm-up
    assert np.array_equal(after, FrameUpscaler(net, use_graph=False).upscale(f, d))
    assert not np.array_equal(after, before)
    # a second shape in between, then the first shape again, through its second warm-up call, its new capture and a replay
    f2, d2 = frames_for(h + 2, w + 3, 1, 30)
    assert np.array_equal(up_g.upscale(f2, d2), up_e.upscale(f2, d2))
    for i in range(3):
        f, d = seq[i]
        assert np.array_equal(up_g.upscale(f, d), up_e.upscale(f, d)), i
    assert up_g.captures == 2 and up_g.replays == replays + 2, (up_g.captures, up_g.replays)
    assert np.array_equal(up_g.upscale(f2, d2), up_e.upscale(f2, d2))
    return dict(replays=up_g.replays, captures=up_g.captures)


# On the emulator a forward of X2 costs about four seconds whatever the frame size (its three depth blocks' mask branches),
# and this check needs fourteen of them to say something about ORDER, not about the network: there it runs on the same x2
# trunk without depth blocks (a sixth of the time).  On the MI355X it runs on X2 itself.
X2_LIGHT = dict(name="x2_nb4_light", scale=2, which=[], L=32, nb=4, B=1, H=8, W=12)


def check_pipeline_order(device):
    case = X2 if device == "cuda" else X2_LIGHT
    net, _ = _net(case, device)
    h, w = case["H"], case["W"]
    seq = [frames_for(h, w, 1, 40 + i) for i in range(7)]
    sync = FrameUpscaler(net, use_graph=False)
    want = [sync.upscale(f, d) for f, d in seq]
    assert all(not np.array_equal(want[i], want[j]) for i in range(7) for j in range(i))          # seven distinct results
    out = {}
    for use_graph in ((False, True) if device == "cuda" else (False,)):
        up = FrameUpscaler(net, use_graph=use_graph)
        got = list(up.upscale_iter(iter(seq)))         # collected first, compared afterwards: a reused slot would show
        assert len(got) == 7
        for i in range(7):
            assert np.array_equal(got[i], want[i]), (use_graph, i)
        out["replays" if use_graph else "eager"] = up.replays
        if use_graph:
            assert up.replays == 5 and up.captures == 2          # one graph per slot, after the shape's two eager frames

        if device != "cuda":                          # (no streams, no slots: upscale_iter is a loop over upscale there)
            continue
        # a change of shape mid-stream, then a failing source: everything taken from it comes out, in order, then the error
        other = [frames_for(h + 1, w + 2, 1, 50 + i) for i in range(2)]

        def source():
            yield from seq[:3]
            yield from other
            yield seq[3]
            raise KeyError("camera unplugged")

        got, err = [], None
        try:
            for r in up.upscale_iter(source()):
                got.append(r)
        except KeyError as e:
            err = e
        assert err is not None and len(got) == 6, (err, len(got))
        for r, (f, d) in zip(got, seq[:3] + other + [seq[3]]):
            assert np.array_equal(r, sync.upscale(f, d))
    return out


def check_validate_u8(device):
    case = X2
    net, cfg = _net(case, device)
    h, w, s = case["H"], case["W"], case["scale"]
    old, new = [], []
    for i in range(3):
        lq, gt, dm, _ = synth.seeded_batch(i, 1, h, w, s)
        f = validate.tensor2img(lq[0])                                   # a uint8 BGR camera frame
        dd = dm.to(device)
        old.append((img2tensor(f)[None].to(device), gt.to(device), dd, prep.depth_to_masks(dd, 10)))
        new.append((f[None], gt, dm))
    psnr, ssim_v, n = validate.validate(net, old, s)
    psnr8, ssim8, n8 = validate.validate_u8(net, new, s)
    assert n == n8 == 3
    assert math.isfinite(psnr) and abs(psnr - psnr8) <= 1e-9, (psnr, psnr8)
    assert abs(ssim_v - ssim8) <= 2e-6, (ssim_v, ssim8)                  # check_ssim_kernel's tolerance
    return dict(psnr=psnr8, ssim=ssim8)


def check_validate_u8_graph(device):
    """validate_u8(use_graph=True) with the GT already on the device: nothing in the loop synchronises, so the host runs
    ahead of the GPU by whole frames - through the warm-up, the capture and six replays.  Every frame is different and the
    metrics must be those of validate() on the same frames: a frame staged over the previous one's queued upload, or a
    replay reading the wrong buffers, changes them."""
    case = X2
    net, cfg = _net(case, device)
    h, w, s = case["H"], case["W"], case["scale"]
    old, new = [], []
    for i in range(9):
        lq, gt, dm, _ = synth.seeded_batch(100 + i, 1, h, w, s)
        f = validate.tensor2img(lq[0])
        dd, gd = dm.to(device), gt.to(device)
        old.append((img2tensor(f)[None].to(device), gd, dd, prep.depth_to_masks(dd, 10)))
        new.append((f[None], gd, dm))                                    # uint8 frame and depth on the host, GT on the device
    psnr, ssim_v, n = validate.validate(net, old, s)
    psnr8, ssim8, n8 = validate.validate_u8(net, new, s, use_graph=True)
    assert n == n8 == 9
    assert math.isfinite(psnr) and abs(psnr - psnr8) <= 1e-9, (psnr, psnr8)
    assert abs(ssim_v - ssim8) <= 2e-6, (ssim_v, ssim8)
    return dict(psnr=psnr8, ssim=ssim8)


def check_upscaler_fixed_range(device):
    """FrameUpscaler(fixed_range=True): the [0,1] bins of depthFixedRange, eagerly and from a captured graph (the edges are
    device constants of the upscaler: nothing is uploaded inside the capture).  Depth values below 0 and above 1 (no bin)
    are part of the input."""
    case = X2
    net, _ = _net(case, device)
    h, w = case["H"], case["W"]
    out = {}
    for use_graph in (False, True):
        up = FrameUpscaler(net, fixed_range=True, use_graph=use_graph)
        for i in range(4):
            f, d = frames_for(h, w, 1, 60 + i)
            d = d * 1.4 - 0.2
            dd = d.to(device)
            lq = img2tensor(f[0])[None].to(device)
            sr = validate.test(net, lq, dd, prep.depth_to_masks(dd, 10, fixed_range=True))
            assert np.array_equal(up.upscale(f, d)[0], validate.tensor2img(sr[0])), (use_graph, i)
        out["graph" if use_graph else "eager"] = up.replays
    assert out == dict(eager=0, graph=2), out
    return out
