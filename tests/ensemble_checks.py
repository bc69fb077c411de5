"""Geometric self-ensemble inference (csrc/ensemble.hip: dasr_ensemble_expand_f32 / _u8 / dasr_ensemble_ingest_u8 /
dasr_ensemble_merge; validate.test_x8; video.FrameUpscaler(self_ensemble=True); validate.validate_u8(self_ensemble=True)).
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_ensemble.py runs them.

Every comparison is exact (== on bytes or bits): the kernels move data, divide a byte by 255 as frame_ingest_u8 does, or add
eight clamped values in a stated order; the whole-path checks compare against the same forward kernels run on the same
batches, with the flips done by torch.  Member m = v + 2 h + 4 t (v: flip along W, h: flip along H, t: transpose, last);
member m of image n is image (m % 4) * N + n of its group's tensor (include/dasr.h)."""
import numpy as np
import torch

from dasr_amd import _lib, ops, prep, synth, validate
from dasr_amd.video import FrameUpscaler
from tests import video_checks as vc
from tests.video_checks import X2, X2_LIGHT, X8, frames_for, img2tensor

E_UNSUPPORTED = -3
# (N, H, W, C): a single pixel, 105-byte frames, a multiple of everything, both sides of the 32- and 64-wide tile edges, a
# single row, a single column
SHAPES = [(1, 1, 1, 3), (2, 5, 7, 3), (3, 4, 16, 3), (1, 33, 31, 3), (1, 31, 65, 1), (2, 64, 32, 1), (1, 1, 40, 1), (1, 40, 1, 3)]
GUARD = 8                                # untouched elements asked for behind every output


def _i32(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    """Bit equality (NaNs of equal bits are equal, 0.0 and -0.0 are not)."""
    return a.shape == b.shape and torch.equal(_i32(a.cpu()), _i32(b.cpu()))


def _same_nan(a, b):
    """NaNs at the same places, equal bits everywhere else (the sign and payload of a NaN that an addition produces - inf
    plus -inf - are the adder's own choice and differ between the host and the device)."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and _same(torch.where(na, 0.0, a), torch.where(nb, 0.0, b))


# ---- the index formulas, in torch ------------------------------------------------------------------------------------------
def _flip(x, m, dh, dw):
    """g[.., r, c, ..] = x[.., fh(r), fv(c), ..] for member m's h and v; dh / dw: the H and W axes of x."""
    dims = ([dh] if (m >> 1) & 1 else []) + ([dw] if m & 1 else [])
    return torch.flip(x, dims) if dims else x


def member(x, m, dh=1, dw=2):
    """x_m of the issue: t = 0: x[fh(r), fv(c)];  t = 1: x[fh(c), fv(r)] = the flipped image, transposed."""
    g = _flip(x, m, dh, dw)
    return (g.transpose(dh, dw) if m >= 4 else g).contiguous()


def unmember(y, m, dh=1, dw=2):
    """z_m of the merge: t = 0: y[fh(r), fv(c)];  t = 1: y[fv(c), fh(r)] = the transposed result, flipped."""
    return _flip(y.transpose(dh, dw) if m >= 4 else y, m, dh, dw).contiguous()


def groups(x, dh=1, dw=2):
    return (torch.cat([member(x, m, dh, dw) for m in range(4)]), torch.cat([member(x, m, dh, dw) for m in range(4, 8)]))


def merged(y_a, y_t, lo, hi, dh=1, dw=2):
    """The inverse maps, torch.clamp, seven sequential fp32 additions, times 0.125."""
    N = y_a.shape[0] // 4
    acc = None
    for m in range(8):
        y = (y_a if m < 4 else y_t)[(m % 4) * N:(m % 4 + 1) * N]
        z = torch.clamp(unmember(y, m, dh, dw), lo, hi)
        acc = z if acc is None else acc + z
    return acc * 0.125


def _guarded(shape, dtype, off, sentinel, device):
    """(view, buffer): a contiguous tensor of ``shape`` ``off`` elements into an allocation that is full of ``sentinel`` and
    has GUARD more elements behind the view."""
    n = int(np.prod(shape))
    buf = torch.full((off + n + GUARD,), sentinel, dtype=dtype).to(device)
    return buf[off:off + n].view(shape), buf


def _guards_intact(buf, off, n, sentinel):
    b = buf.cpu()
    want = torch.full((1,), sentinel, dtype=b.dtype)
    return _same(b[:off], want.expand(off)) and _same(b[off + n:], want.expand(GUARD))


def _random(shape, dtype, gen):
    if dtype == torch.uint8:
        return torch.from_numpy(gen.integers(0, 255, size=shape, dtype=np.uint8))       # 255 is the sentinel
    return torch.from_numpy(gen.standard_normal(size=shape).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. expand
# ---------------------------------------------------------------------------------------------------------------------
def check_expand(device):
    gen = np.random.default_rng(31)
    cases = 0
    for dtype, sentinel, offsets in ((torch.float32, float("nan"), ((0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 0))),
                                     (torch.uint8, 255, ((0, 0, 0), (1, 2, 3), (2, 3, 1), (3, 1, 2)))):
        for shape in SHAPES:
            N, H, W, C = shape
            x = _random(shape, dtype, gen)
            want_a, want_t = groups(x)
            assert want_a.shape == (4 * N, H, W, C) and want_t.shape == (4 * N, W, H, C)
            for off_x, off_a, off_t in offsets:
                xd = vc._offset_view(x, off_x, device)
                a, buf_a = _guarded(want_a.shape, dtype, off_a, sentinel, device)
                t, buf_t = _guarded(want_t.shape, dtype, off_t, sentinel, device)
                got_a, got_t = ops.ensemble_expand(xd, out=(a, t))
                assert got_a is a and got_t is t
                # the sentinel is no value of x: equality says that every element was written
                assert _same(a, want_a), (dtype, shape, off_x, off_a)
                assert _same(t, want_t), (dtype, shape, off_x, off_t)
                assert _guards_intact(buf_a, off_a, a.numel(), sentinel), (dtype, shape, off_a)
                assert _guards_intact(buf_t, off_t, t.numel(), sentinel), (dtype, shape, off_t)
                cases += 1
            got_a, got_t = ops.ensemble_expand(x.to(device))                    # buffers of the op's own
            assert _same(got_a, want_a) and _same(got_t, want_t), (dtype, shape)
    lib = _lib.get()
    x2 = torch.zeros((1, 4, 4, 2), device=device)
    o2 = torch.zeros((4, 4, 4, 2), device=device)
    assert lib.dasr_ensemble_expand_f32(ops._p(x2), ops._p(o2), ops._p(o2.clone()), 1, 4, 4, 2, _lib.stream()) == E_UNSUPPORTED
    u2, q2 = x2.to(torch.uint8), o2.to(torch.uint8)
    assert lib.dasr_ensemble_expand_u8(ops._pu8(u2), ops._pu8(q2), ops._pu8(q2.clone()), 1, 4, 4, 2, _lib.stream()) == E_UNSUPPORTED
    assert lib.dasr_ensemble_ingest_u8(ops._pu8(u2), ops._p(o2), ops._p(o2.clone()), 1, 4, 4, 2, 1, _lib.stream()) == E_UNSUPPORTED
    assert lib.dasr_ensemble_merge(ops._p(o2), ops._p(o2.clone()), ops._p(x2), 1, 4, 4, 2, 0.0, 1.0, _lib.stream()) == E_UNSUPPORTED
    for bad in (x2, x2.to(torch.uint8)):
        try:
            ops.ensemble_expand(bad)
            raise AssertionError("C = 2 accepted")
        except ValueError:
            pass
    return dict(cases=cases)


# ---------------------------------------------------------------------------------------------------------------------
# 2. ingest
# ---------------------------------------------------------------------------------------------------------------------
def check_ingest(device):
    gen = np.random.default_rng(32)
    cases = 0
    inputs = [torch.from_numpy(gen.integers(0, 256, size=s, dtype=np.uint8)) for s in SHAPES]
    for C in (3, 1):
        allv = np.zeros((1, 17, 19, C), dtype=np.uint8)           # every byte value in every channel (7 is a unit mod 256)
        p = np.arange(17 * 19)
        for c in range(C):
            allv[0, :, :, c] = ((p * 7 + 85 * c) % 256).reshape(17, 19)
            assert len(set(allv[0, :, :, c].ravel().tolist())) == 256
        inputs.append(torch.from_numpy(allv))
    nan = float("nan")
    for x in inputs:
        N, H, W, C = x.shape
        for swap in (True, False):
            for off_x, off_a, off_t in ((0, 0, 0), (1, 1, 1), (2, 1, 0), (3, 0, 1)):
                xd = vc._offset_view(x, off_x, device)
                a, buf_a = _guarded((4 * N, H, W, C), torch.float32, off_a, nan, device)
                t, buf_t = _guarded((4 * N, W, H, C), torch.float32, off_t, nan, device)
                ops.ensemble_ingest_u8(xd, swap_rb=swap, out=(a, t))
                want_a, want_t = ops.ensemble_expand(ops.frame_ingest_u8(xd, swap_rb=swap))
                assert _same(a, want_a) and _same(t, want_t), (tuple(x.shape), swap, off_x, off_a, off_t)
                assert _guards_intact(buf_a, off_a, a.numel(), nan) and _guards_intact(buf_t, off_t, t.numel(), nan)
                cases += 1
            if C == 3 and swap:                                   # member 0, permuted to NCHW: the reference's img2tensor
                a0 = ops.ensemble_ingest_u8(x.to(device), swap_rb=True)[0][:N].cpu()
                for b in range(N):
                    assert _same(a0[b].permute(2, 0, 1).contiguous(), img2tensor(x[b].numpy())), (tuple(x.shape), b)
    return dict(cases=cases)


# ---------------------------------------------------------------------------------------------------------------------
# 3. merge
# ---------------------------------------------------------------------------------------------------------------------
def check_merge(device):
    gen = np.random.default_rng(33)
    inf = float("inf")
    cases = 0
    for shape in SHAPES:
        N, H, W, C = shape
        for lo, hi in ((0.0, 1.0), (-1.0, 1.0)):
            # eight independently drawn members, inside and outside [lo, hi]; the special values at random places of every
            # member (the largest shape holds them all in each)
            special = np.array([np.nan, inf, -inf, -0.0, lo, hi, 0.0, np.nextafter(np.float32(hi), np.float32(2 * hi))],
                               dtype=np.float32)
            ys = []
            for (n4, a, b) in ((4 * N, H, W), (4 * N, W, H)):
                y = gen.uniform(lo - 0.5, hi + 0.5, size=(n4, a, b, C)).astype(np.float32)
                flat = y.reshape(n4, -1)
                for i in range(n4):
                    k = min(special.size, max(1, flat.shape[1] // 4))
                    flat[i, gen.permutation(flat.shape[1])[:k]] = gen.permutation(special)[:k]
                ys.append(torch.from_numpy(y))
            want = merged(ys[0], ys[1], lo, hi)
            for off_a, off_t, off_o in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
                out, buf = _guarded(shape, torch.float32, off_o, 777.0, device)
                got = ops.ensemble_merge(vc._offset_view(ys[0], off_a, device), vc._offset_view(ys[1], off_t, device), lo, hi,
                                         out=out)
                assert got is out
                assert _same_nan(out, want), (shape, lo, hi, off_a, off_t, off_o)
                assert _guards_intact(buf, off_o, out.numel(), 777.0)
                cases += 1
        # The round trip merge(expand(x)) with an open clamp.  The seven additions are rounded one by one, so eight equal
        # values sum exactly only while 3 v, 5 v, 6 v and 7 v are fp32 numbers (1 + 2^-23 is a counter-example: 3 v already
        # rounds): for x with at most 21 significant bits the round trip is x itself, bit for bit (-0.0 included); for any
        # finite x it is the sequential sum of eight copies.
        x = _random(shape, torch.float32, gen)
        x.view(-1)[0] = -0.0
        x21 = (x.view(torch.int32) & ~7).view(torch.float32)
        for v in (x21, x):
            a, t = ops.ensemble_expand(v.to(device))
            got = ops.ensemble_merge(a, t, -inf, inf)
            assert _same(got, merged(*groups(v), -inf, inf)), shape
            if v is x21:
                assert _same(got, v), shape
    return dict(cases=cases)


# ---------------------------------------------------------------------------------------------------------------------
# 4. binning the expanded depth = expanding the binned planes
# ---------------------------------------------------------------------------------------------------------------------
def _expand_planes(planes):
    B, K, h, w = planes.shape
    a, t = ops.ensemble_expand(planes.contiguous().view(B * K, h, w, 1))
    return a.view(4 * B, K, h, w), t.view(4 * B, K, w, h)


def check_masks_commute(device):
    gen = np.random.default_rng(34)
    B, h, w, K = 2, 5, 7, 10
    d = torch.from_numpy(gen.random(size=(B, 1, h, w), dtype=np.float32)).to(device)
    da, dt = ops.ensemble_expand(d.view(B, h, w, 1))
    da, dt = da.view(4 * B, 1, h, w), dt.view(4 * B, 1, w, h)
    assert _same(da, groups(d.cpu(), 2, 3)[0]) and _same(dt, groups(d.cpu(), 2, 3)[1])
    out = {}
    for name, edges in (("per_sample", None), ("fixed", prep.fixed_range_edges(K, torch.device(device)))):
        planes, region = ops.depth_to_masks(d, K, edges)
        assert float(planes.sum()) > 0.5 * B * h * w                       # the planes are not empty
        want_pa, want_pt = _expand_planes(planes)
        want_ra, want_rt = ops.ensemble_expand(region.view(B, h, w, 1))
        for dd, want_p, want_r in ((da, want_pa, want_ra), (dt, want_pt, want_rt)):
            got_p, got_r = ops.depth_to_masks(dd, K, edges)
            assert _same(got_p, want_p), name
            assert _same(got_r, want_r.view(got_r.shape)), name
        out[name] = int(region.max())
    for fixed in (False, True):
        planes = ops.depth_to_masks_soft(d, K, 0.5, fixed)
        assert float(((planes > 0) & (planes < 1)).sum()) > 0              # really soft
        want_pa, want_pt = _expand_planes(planes)
        assert _same(ops.depth_to_masks_soft(da, K, 0.5, fixed), want_pa), fixed
        assert _same(ops.depth_to_masks_soft(dt, K, 0.5, fixed), want_pt), fixed
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 5. validate.test_x8 = two batched validate.test calls on torch-flipped inputs, merged in torch
# ---------------------------------------------------------------------------------------------------------------------
def _masks_of(kind, d):
    if kind == "stamped":
        return prep.depth_to_masks(d, 10)
    if kind == "unstamped":
        return prep.depth_to_masks(d, 10).clone()
    return prep.depth_to_soft_masks(d, 10, width=0.5)


def _group_masks(kind, masks, device):
    """The torch-flipped mask batches of the two groups, stamped as ``masks`` is."""
    from dasr_amd import graph
    ga, gt = (g.to(device) for g in groups(masks.cpu(), 2, 3))
    if kind == "stamped":
        region = graph.attached_region(masks)
        assert region is not None
        for g, r in zip((ga, gt), groups(region.cpu(), 1, 2)):
            g._dasr_region = r.to(device)
            g._dasr_version = ops.tensor_version(g)
            assert graph.attached_region(g) is not None
    elif kind == "soft":
        assert prep.marked_soft(masks)
        prep.mark_soft(ga)
        prep.mark_soft(gt)
    else:
        assert graph.attached_region(masks) is None and not prep.marked_soft(masks)
    return ga, gt


def _x8_by_hand(net, lq, d, kind, masks, device):
    xa, xt = (g.to(device) for g in groups(lq.cpu(), 2, 3))
    da, dt = (g.to(device) for g in groups(d.cpu(), 2, 3))
    ma, mt = _group_masks(kind, masks, device)
    ya = validate.test(net, xa, da, ma).cpu()
    yt = validate.test(net, xt, dt, mt).cpu()
    return merged(ya, yt, net.min, net.max, 2, 3)


def _members_check(device, configs, batches, kinds=("stamped", "unstamped", "soft")):
    out = {}
    for case, dtype in configs:
        net, _ = vc._net(case, device, dtype)
        h, w, s = case["H"], case["W"], case["scale"]
        assert h != w
        for B in batches:
            f, d = frames_for(h, w, B, 70 + B)
            lq = torch.stack([img2tensor(f[b]) for b in range(B)]).to(device)
            dd = d.to(device)
            for kind in kinds:
                masks = _masks_of(kind, dd)
                got = validate.test_x8(net, lq, dd, masks)
                assert net.training                                        # the module's mode is left alone
                want = _x8_by_hand(net, lq, dd, kind, masks, device)
                assert got.dtype == torch.float32 and tuple(got.shape) == (B, 3, s * h, s * w)
                assert _same(got, want), (case["name"], dtype, B, kind, float((got.cpu() - want).abs().max()))
                g = got.cpu()
                assert float(g.min()) >= net.min and float(g.max()) <= net.max
                out["%s/%s/B%d/%s" % (case["name"], str(dtype).split(".")[-1], B, kind)] = \
                    float(((g > net.min) & (g < net.max)).float().mean())
        if device != "cpu":
            net.eval()
            assert _same(validate.test_x8(net, lq, dd, masks), got)            # an eval() module stays in eval()
            assert not net.training
    assert all(v > 0.2 for v in out.values()), out                         # no comparison of saturated images
    return out


def check_conditioning_stamps(device):
    """validate._expand_conditioning: what test_x8 hands the two forwards beside the image.  The expanded depth and planes
    are the torch-flipped ones, and the masks' stamp travels: region bytes expanded with them, a soft stamp repeated, no
    stamp left as none."""
    from dasr_amd import graph
    gen = np.random.default_rng(35)
    B, h, w = 2, 5, 7
    d = torch.from_numpy(gen.random(size=(B, 1, h, w), dtype=np.float32)).to(device)
    for kind in ("stamped", "unstamped", "soft"):
        masks = _masks_of(kind, d)
        (da, ma), (dt, mt) = validate._expand_conditioning(d, masks)
        want_ma, want_mt = _group_masks(kind, masks, device)
        for got, want in ((da, groups(d.cpu(), 2, 3)[0]), (dt, groups(d.cpu(), 2, 3)[1]), (ma, want_ma), (mt, want_mt)):
            assert got.is_contiguous() and _same(got, want), kind
        for got, want in ((ma, want_ma), (mt, want_mt)):
            assert prep.marked_soft(got) == prep.marked_soft(want) == (kind == "soft"), kind
            r, rw = graph.attached_region(got), graph.attached_region(want)
            assert (r is None) == (rw is None) == (kind != "stamped"), kind
            assert r is None or _same(r, rw), kind
    return dict(kinds=3)


def check_test_x8_members(device):
    """On the emulator a batch-4 forward of even the depth-block-free x2 trunk takes seconds, and a comparison needs four:
    there the forwards run for the stamped masks only (a network with depth blocks would need ten seconds per forward, so
    none runs there) and check_conditioning_stamps covers what differs between the three kinds of masks; the MI355X runs
    every kind, with depth blocks."""
    if device == "cpu":
        return _members_check(device, [(X2_LIGHT, torch.float32)], (1,), kinds=("stamped",))
    return _members_check(device, [(X2, torch.float32), (X2, torch.bfloat16)], (1, 2))


def check_test_x8_members_x8(device):
    return _members_check(device, [(X8, torch.float32), (X8, torch.bfloat16)], (1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# 6. FrameUpscaler(self_ensemble=True) = tensor2img(validate.test_x8(img2tensor(frames)))
# ---------------------------------------------------------------------------------------------------------------------
def _via_test_x8(net, f, d, device, min_max=(0, 1)):
    lq = torch.stack([img2tensor(f[b]) for b in range(f.shape[0])]).to(device)
    dd = d.to(device)
    sr = validate.test_x8(net, lq, dd, prep.depth_to_masks(dd, 10))
    return np.stack([validate.tensor2img(sr[b], min_max=min_max) for b in range(f.shape[0])])


def check_upscaler_ensemble(device):
    configs = [(X2_LIGHT, torch.float32)] if device == "cpu" else \
        [(X2, torch.float32), (X8, torch.float32), (X2, torch.bfloat16), (X8, torch.bfloat16)]
    out = {}
    for case, dtype in configs:
        net, _ = vc._net(case, device, dtype)
        up = FrameUpscaler(net, use_graph=False, self_ensemble=True)
        plain = FrameUpscaler(net, use_graph=False)
        for B in ((1,) if device == "cpu" else (1, 2)):      # (a batch-8 forward on the emulator takes seven seconds)
            f, d = frames_for(case["H"], case["W"], B, B)
            got = up.upscale(f, d)
            want = _via_test_x8(net, f, d, device)
            assert got.dtype == np.uint8 and got.shape == want.shape == (B, case["scale"] * case["H"], case["scale"] * case["W"], 3)
            assert np.array_equal(got, want), (case["name"], dtype, B, int((got != want).sum()))
            interior = float(((got > 0) & (got < 255)).mean())
            assert interior > 0.2, interior            # the comparison is not one of saturated images
            out["%s/%s/B%d" % (case["name"], str(dtype).split(".")[-1], B)] = interior
            base = plain.upscale(f, d)                 # self_ensemble=False: what it was
            assert np.array_equal(base, vc._via_validate(net, f, d, device)), (case["name"], dtype, B)
            assert not np.array_equal(base, got)
        assert net.training
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GPU only: the captured chain, validate_u8
# ---------------------------------------------------------------------------------------------------------------------
def check_ensemble_graph(device):
    case = X2
    net, _ = vc._net(case, device)
    up_g = FrameUpscaler(net, use_graph=True, self_ensemble=True)
    up_e = FrameUpscaler(net, use_graph=False, self_ensemble=True)
    h, w = case["H"], case["W"]
    seq = [frames_for(h, w, 1, 80 + i) for i in range(5)]
    want = [up_e.upscale(f, d) for f, d in seq]
    assert all(not np.array_equal(want[i], want[j]) for i in range(5) for j in range(i))
    for i, (f, d) in enumerate(seq):
        assert np.array_equal(up_g.upscale(f, d), want[i]), i
        assert up_g.replays == max(0, i - 1), (i, up_g.replays)          # two eager calls, then a replay per call
    assert up_g.captures == 1
    # the same five frames through the two-slot pipeline of a second upscaler
    up_i = FrameUpscaler(net, use_graph=True, self_ensemble=True)
    got = list(up_i.upscale_iter(iter(seq)))
    assert len(got) == 5 and all(np.array_equal(got[i], want[i]) for i in range(5))
    assert up_i.captures == 2 and up_i.replays == 3, (up_i.captures, up_i.replays)
    # an in-place parameter edit: the captured graph holds the folded kernels of the old value and must not be replayed
    with torch.no_grad():
        net.get_parameter("conv_output.weight").mul_(1.5)
    f, d = seq[4]
    replays = up_g.replays
    after = up_g.upscale(f, d)
    assert up_g.replays == replays                                       # back in the warm-up
    assert np.array_equal(after, FrameUpscaler(net, use_graph=False, self_ensemble=True).upscale(f, d))
    assert not np.array_equal(after, want[4])
    return dict(replays=up_g.replays, captures=up_g.captures)


def check_validate_u8_ensemble(device):
    case = X2
    net, _ = vc._net(case, device)
    h, w, s = case["H"], case["W"], case["scale"]
    new = []
    psnr = ssim_v = 0.0
    for i in range(3):
        lq, gt, dm, _ = synth.seeded_batch(200 + i, 1, h, w, s)
        f = validate.tensor2img(lq[0])                                   # a uint8 BGR camera frame
        dd = dm.to(device)
        sr = validate.test_x8(net, img2tensor(f)[None].to(device), dd, prep.depth_to_masks(dd, 10))
        sr_img, gt_img = validate.tensor2img(sr[0]), validate.tensor2img(gt[0])
        psnr += validate.calculate_psnr(sr_img[s:-s, s:-s, :], gt_img[s:-s, s:-s, :])
        ssim_v += float(validate.ssim(sr[:1], gt[:1].to(device).float().contiguous()))
        new.append((f[None], gt, dm))
    psnr8, ssim8, n8 = validate.validate_u8(net, new, s, self_ensemble=True)
    assert n8 == 3
    assert np.isfinite(psnr8) and psnr8 == psnr / 3, (psnr8, psnr / 3)   # an integer sum of squares on both sides
    assert ssim8 == ssim_v / 3, (ssim8, ssim_v / 3)                      # the same kernel on the same tensor
    plain = validate.validate_u8(net, new, s)
    assert plain[0] != psnr8                                             # the ensemble is not the single forward
    return dict(psnr=psnr8, ssim=ssim8, plain_psnr=plain[0])
