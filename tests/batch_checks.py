"""Training batches from uint8 HR frames (csrc/batch.hip: dasr_batch_lr_u8 / dasr_batch_gt_u8 / dasr_batch_plane_f32 / _u8;
ops.batch_lr_u8 / batch_gt_u8 / batch_plane; data.resize_tables / draw_augment / BatchMaker).  Each check takes the device
("cpu": the kernel emulator, "cuda": the MI355X); tests/test_batch.py runs them.

The fixtures tests/golden/batch_*.npz hold what the reference's loader functions computed (tools/make_batch_golden.py).
Everything except the LR value is compared bit for bit; the LR value is gated against a float64 evaluation of the resize
by a multiple of the reference's own distance from it (check_lr_value)."""
import functools
import os
import random

import numpy as np
import torch

from dasr_amd import _lib, data, harness, ops, prep
from tests.parity_checks import build_net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(48, 64, 8), (36, 48, 3), (39, 51, 3), (40, 56, 2), (48, 48, 4), (264, 152, 8), (16, 24, 8)]
E_REF_MAX = 2.5e-7          # the reference's own fp32 rounding against float64 on these shapes (measured 5e-8 .. 2.0e-7)
GATE = 4.0                  # max|lr_hip - lr64| <= GATE * e_ref of the case
E_SHAPE, E_UNSUPPORTED = -2, -3
K = 10


@functools.lru_cache(maxsize=None)
def fixture(H, W, s):
    """The arrays of one case; loaded once, never modified."""
    with np.load(os.path.join(GOLDEN, "batch_%dx%dx%d.npz" % (H, W, s))) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def np_augment(img, flags):
    """The reference's _augment (data/util.py:107-114) on an HWC array."""
    if flags & 1:
        img = img[:, ::-1, :]
    if flags & 2:
        img = img[::-1, :, :]
    if flags & 4:
        img = img.transpose(1, 0, 2)
    return img


def np_pack(img_hwc_bgr, flags):
    """augment, BGR -> RGB, HWC -> CHW (LQGTker_Depth_dataset.py:176-193) of one image."""
    img = np_augment(img_hwc_bgr, flags)
    if img.shape[2] == 3:
        img = img[:, :, [2, 1, 0]]
    return np.ascontiguousarray(np.transpose(img, (2, 0, 1)))


def _tables(H, W, s, device):
    wh, ih, _, _ = data.resize_tables(H, s)
    ww, iw, _, _ = data.resize_tables(W, s)
    return tuple(torch.from_numpy(np.array(t)).to(device) for t in (wh, ih, ww, iw))


def _reflect(i, n):
    i = np.where(i < 0, -i - 1, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


@functools.lru_cache(maxsize=None)
def lr64(H, W, s):
    """The resize in float64: the fp32 image ``u8 / 255`` widened, float64 weights ``cubic((u - i) / s) / s`` normalised
    per output, ``u = s x + 0.5 (1 - s)``, 4s taps, symmetric reflection, H pass then W pass, nothing rounded.  [h,w,3] BGR."""
    img = (fixture(H, W, s)["hr"].astype(np.float32) / np.float32(255.)).astype(np.float64)

    def axis_tables(n):
        x = np.arange(1, n // s + 1, dtype=np.float64)
        u = s * x + 0.5 * (1 - s)
        first = np.floor(u - 2 * s).astype(np.int64) + 1                     # 1-based: the 4s columns the reference keeps
        idx = first[:, None] + np.arange(4 * s)[None, :]
        t = np.abs((u[:, None] - idx) / s)
        w = np.where(t <= 1, 1.5 * t ** 3 - 2.5 * t ** 2 + 1, np.where(t <= 2, -0.5 * t ** 3 + 2.5 * t ** 2 - 4 * t + 2, 0.0)) / s
        return w / w.sum(axis=1, keepdims=True), _reflect(idx - 1, n)

    wy, iy = axis_tables(H)
    wx, ix = axis_tables(W)
    mid = np.einsum("rk,rkxc->rxc", wy, img[iy])                                 # [h, W, 3]
    out = np.einsum("ck,rckd->rcd", wx, mid[:, ix])                              # [h, w, 3]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _full_lr(H, W, s, device):
    """ops.batch_lr_u8 of the case's frame, whole, unaugmented: [3,h,w] RGB numpy; computed once per device."""
    hr = torch.from_numpy(fixture(H, W, s)["hr"])[None].to(device)
    out = ops.batch_lr_u8(hr, s, _tables(H, W, s, device)).cpu().numpy()[0]
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a. LR value
# ---------------------------------------------------------------------------------------------------------------------
def check_lr_value(device):
    """Measured (emulator and MI355X give the same bits): ratio max|lr_hip - lr64| / e_ref per case is recorded in
    DESIGN.md section 4.14."""
    out = {}
    for (H, W, s) in CASES:
        fx = fixture(H, W, s)
        want = lr64(H, W, s)
        e_ref = float(np.abs(fx["lr"].astype(np.float64) - want).max())
        got = _full_lr(H, W, s, device)                                          # [3,h,w] RGB
        assert got.shape == (3, H // s, W // s) and got.dtype == np.float32
        e_hip = float(np.abs(np.transpose(got[::-1], (1, 2, 0)).astype(np.float64) - want).max())
        print("lr %dx%d x%d: e_ref %.3e  e_hip %.3e  ratio %.3f" % (H, W, s, e_ref, e_hip, e_hip / e_ref))
        out["%dx%dx%d" % (H, W, s)] = round(e_hip / e_ref, 3)
        assert 0 < e_ref <= E_REF_MAX, (H, W, s, e_ref)
        assert e_hip <= GATE * e_ref, (H, W, s, e_hip, e_ref)
        if s == 2:
            assert got.min() < 0 or got.max() > 1, (got.min(), got.max())        # not clamped: the overshoot is there
    return out


# ---------------------------------------------------------------------------------------------------------------------
# b. invariants, bitwise
# ---------------------------------------------------------------------------------------------------------------------
def check_lr_invariants(device):
    n = 0
    for (H, W, s), (ch, cw), origins in (((264, 152, 8), (9, 10), [(0, 0), (24, 9), (7, 3)]),
                                         ((39, 51, 3), (5, 16), [(8, 1), (3, 0)]),
                                         ((40, 56, 2), (17, 19), [(3, 9), (0, 2)])):
        hr = fixture(H, W, s)["hr"]
        full = _full_lr(H, W, s, device)
        tb = _tables(H, W, s, device)
        # a crop window is that window of the full-frame LR
        B = len(origins)
        frames = torch.from_numpy(np.stack([hr] * B)).to(device)
        og = torch.tensor(origins, dtype=torch.int32, device=device)
        got = ops.batch_lr_u8(frames, s, tb, (ch, cw), og).cpu().numpy()
        for b, (oy, ox) in enumerate(origins):
            assert _same(got[b], full[:, oy:oy + ch, ox:ox + cw]), ("crop", H, W, s, b)
            n += 1
        # sample b of a batch of three is that frame alone
        other = np.random.default_rng(5).integers(0, 256, size=(2,) + hr.shape, dtype=np.uint8)
        batch = torch.from_numpy(np.stack([other[0], hr, other[1]])).to(device)
        assert _same(ops.batch_lr_u8(batch, s, tb).cpu().numpy()[1], full), ("batch", H, W, s)
        # base pointers 1, 2, 3 bytes off the dword grid
        for off in (1, 2, 3):
            buf = torch.zeros((hr.size + off,), dtype=torch.uint8, device=device)
            view = buf[off:].view((1,) + hr.shape)
            view.copy_(torch.from_numpy(hr)[None])
            assert view.data_ptr() % 4 == off
            assert _same(ops.batch_lr_u8(view, s, tb).cpu().numpy()[0], full), ("offset", H, W, s, off)
            n += 1
        # tables whose outputs do not start s rows apart (every output row twice; still non-decreasing) take the kernel's
        # general H pass: the same bits as the block-wise one the regular tables get
        h = H // s
        dup = torch.arange(h, device=device) // 2
        got = ops.batch_lr_u8(frames[:1], s, (tb[0][dup].contiguous(), tb[1][dup].contiguous(), tb[2], tb[3])).cpu().numpy()[0]
        assert _same(got, np.ascontiguousarray(full[:, np.arange(h) // 2])), ("irregular tables", H, W, s)
        n += 1
    return dict(cases=n)


# ---------------------------------------------------------------------------------------------------------------------
# c. GT
# ---------------------------------------------------------------------------------------------------------------------
def _gt_reference(hr, device):
    """ops.frame_ingest_u8 -> permute: [B,3,H,W] RGB numpy."""
    x = ops.frame_ingest_u8(torch.from_numpy(hr).to(device), swap_rb=True)
    return x.permute(0, 3, 1, 2).contiguous().cpu().numpy()


def check_gt(device):
    n = 0
    # (case, LR window, LR origin, flag values): window origins and sizes that are no multiple of the 32 x 64 tile
    for (H, W, s), (ch, cw), (oy, ox), flagset in (((264, 152, 8), (17, 17), (9, 1), range(8)),
                                                   ((48, 48, 4), (12, 12), (0, 0), range(8)),
                                                   ((39, 51, 3), (11, 15), (2, 1), range(4)),
                                                   ((39, 51, 3), (13, 17), (0, 0), range(4))):
        hr = fixture(H, W, s)["hr"]
        flagset = list(flagset)
        B = len(flagset)
        frames = np.stack([np.roll(hr, b, axis=0) for b in range(B)])               # B different frames
        ref = _gt_reference(frames, device)
        fl = torch.tensor(flagset, dtype=torch.uint8, device=device)
        og = torch.tensor([(oy, ox)] * B, dtype=torch.int32, device=device)
        got = ops.batch_gt_u8(torch.from_numpy(frames).to(device), s, (ch, cw), og, fl, allow_transpose=ch == cw).cpu().numpy()
        assert got.shape == (B, 3, s * ch, s * cw)
        for b, f in enumerate(flagset):
            win = ref[b][:, s * oy:s * (oy + ch), s * ox:s * (ox + cw)]
            want = np.transpose(np_augment(np.transpose(win, (1, 2, 0)), f), (2, 0, 1))
            assert _same(got[b], np.ascontiguousarray(want)), ("gt", H, W, s, f)
            n += 1
    # the reference's own augmented GT (fixture), whole frame
    for (H, W, s) in ((48, 64, 8), (48, 48, 4)):
        fx = fixture(H, W, s)
        f = int(fx["aug_flags"].reshape(-1)[0])
        fl = torch.tensor([f], dtype=torch.uint8, device=device)
        got = ops.batch_gt_u8(torch.from_numpy(fx["hr"])[None].to(device), s, flags=fl, allow_transpose=H == W).cpu().numpy()[0]
        assert _same(got, np_pack(fx["aug_gt"], 0)), ("gt fixture", H, W, s)
        n += 1
    return dict(cases=n)


# ---------------------------------------------------------------------------------------------------------------------
# d. planes
# ---------------------------------------------------------------------------------------------------------------------
def check_plane(device):
    gen = np.random.default_rng(21)
    n = 0
    for (h, w), (ch, cw), (oy, ox), flagset in (((45, 70), (37, 37), (5, 30), range(8)),
                                                ((12, 12), (12, 12), (0, 0), range(8)),
                                                ((13, 17), (11, 15), (2, 1), range(4)),
                                                ((13, 17), (13, 17), (0, 0), range(4))):
        flagset = list(flagset)
        B = len(flagset)
        fl = torch.tensor(flagset, dtype=torch.uint8, device=device)
        og = torch.tensor([(oy, ox)] * B, dtype=torch.int32, device=device)
        for C in (1, 10):
            for dtype in (np.float32, np.uint8):
                x = gen.standard_normal((B, C, h, w)).astype(np.float32) if dtype == np.float32 else \
                    gen.integers(0, 256, size=(B, C, h, w), dtype=np.uint8)
                got = ops.batch_plane(torch.from_numpy(x).to(device), (ch, cw), og, fl, allow_transpose=ch == cw).cpu().numpy()
                for b, f in enumerate(flagset):
                    win = x[b][:, oy:oy + ch, ox:ox + cw]
                    want = np.transpose(np_augment(np.transpose(win, (1, 2, 0)), f), (2, 0, 1))
                    assert _same(got[b], np.ascontiguousarray(want)), ("plane", h, w, C, dtype, f)
                    n += 1
    x3 = gen.integers(0, 256, size=(2, 13, 17), dtype=np.uint8)                      # [B,h,w] region bytes
    got = ops.batch_plane(torch.from_numpy(x3).to(device), flags=torch.tensor([1, 2], dtype=torch.uint8, device=device))
    assert _same(got.cpu().numpy(), np.stack([x3[0][:, ::-1], x3[1][::-1]]))
    return dict(cases=n)


# ---------------------------------------------------------------------------------------------------------------------
# e. masks
# ---------------------------------------------------------------------------------------------------------------------
def _region_of(masks_u8):
    """Region byte per pixel of one-hot uint8 planes [K,h,w]: the plane's index, K where no plane is set."""
    Kp = masks_u8.shape[0]
    return np.where(masks_u8.any(axis=0), masks_u8.argmax(axis=0), Kp).astype(np.uint8)


def check_masks(device):
    n = 0
    for (H, W, s) in ((48, 64, 8), (48, 48, 4), (39, 51, 3)):
        fx = fixture(H, W, s)
        for fixed, key in ((False, "masks"), (True, "masks_fixed")):
            mk = data.BatchMaker(s, K, fixed_range=fixed, device=device)
            flagset = list(range(8)) if H == W else list(range(4))
            B = len(flagset)
            lq, gt, depth, masks = mk.make(np.stack([fx["hr"]] * B), np.stack([fx["depth"]] * B),
                                           np.array(flagset, dtype=np.uint8))
            for b, f in enumerate(flagset):
                want = np_pack(np.transpose(fx[key], (1, 2, 0)).astype(np.float32), f)
                assert _same(masks[b].cpu().numpy(), want), ("masks", H, W, s, fixed, f)
                assert _same(masks._dasr_region[b].cpu().numpy(), _region_of(want.astype(np.uint8))), ("region", H, W, s, f)
                assert _same(depth[b].cpu().numpy(), np_pack(np.transpose(fx["depth"], (1, 2, 0)), f))
                n += 1
            assert masks._dasr_version == ops.tensor_version(masks)
        if "aug_flags" in fx:                                                     # the reference's own augmented tuple
            f = int(fx["aug_flags"].reshape(-1)[0])
            mk = data.BatchMaker(s, K, device=device)
            lq, gt, depth, masks = mk.make(fx["hr"][None], fx["depth"][None], np.array([f], dtype=np.uint8))
            assert _same(masks[0].cpu().numpy(), np_pack(fx["aug_masks"].astype(np.float32), 0))
            assert _same(depth[0].cpu().numpy(), np_pack(fx["aug_depth"], 0))
            assert _same(gt[0].cpu().numpy(), np_pack(fx["aug_gt"], 0))
            assert _same(lq[0].cpu().numpy(), np_pack(np.transpose(_full_lr(H, W, s, device)[::-1], (1, 2, 0)), f))
            e = float(np.abs(lq[0].cpu().numpy().astype(np.float64) - np_pack(fx["aug_lr"], 0)).max())
            assert e <= (1 + GATE) * E_REF_MAX, e          # two fp32 evaluations of the same resize, augmented alike
            n += 1
    # crop mode: binned from the full depth map, then cut and augmented
    H, W, s = 264, 152, 8
    fx = fixture(H, W, s)
    for fixed, key in ((False, "masks"), (True, "masks_fixed")):
        mk = data.BatchMaker(s, K, fixed_range=fixed, crop=(11, 11), device=device)
        flagset, origins = [0, 5, 3, 6], [(0, 0), (22, 8), (7, 3), (13, 1)]
        lq, gt, depth, masks = mk.make(np.stack([fx["hr"]] * 4), np.stack([fx["depth"]] * 4),
                                       np.array(flagset, dtype=np.uint8), np.array(origins))
        full = _full_lr(H, W, s, device)
        for b, (f, (oy, ox)) in enumerate(zip(flagset, origins)):
            win = fx[key][:, oy:oy + 11, ox:ox + 11]
            want = np_pack(np.transpose(win, (1, 2, 0)).astype(np.float32), f)
            assert _same(masks[b].cpu().numpy(), want), ("crop masks", fixed, b)
            assert _same(masks._dasr_region[b].cpu().numpy(), _region_of(want.astype(np.uint8))), ("crop region", fixed, b)
            assert _same(depth[b].cpu().numpy(), np_pack(np.transpose(fx["depth"][:, oy:oy + 11, ox:ox + 11], (1, 2, 0)), f))
            assert _same(lq[b].cpu().numpy(), np_pack(np.transpose(full[::-1, oy:oy + 11, ox:ox + 11], (1, 2, 0)), f))
            n += 1
    return dict(cases=n)


# ---------------------------------------------------------------------------------------------------------------------
# f. draw_augment (host only)
# ---------------------------------------------------------------------------------------------------------------------
def check_draw_augment():
    with np.load(os.path.join(GOLDEN, "batch_augment_flags.npz")) as z:
        options, flags, nxt = z["options"], z["flags"], z["next_random"]
    assert flags.shape == (4, 32) and len({tuple(o) for o in options.tolist()}) == 4
    for o, (use_flip, use_rot) in enumerate(options.tolist()):
        for k in range(32):
            rng = random.Random(k)
            got = data.draw_augment(rng, 1, bool(use_flip), bool(use_rot))
            assert got.dtype == np.uint8 and got.shape == (1,) and got[0] == flags[o, k], (use_flip, use_rot, k, got, flags[o, k])
            assert rng.random() == nxt[o, k], (use_flip, use_rot, k)              # the same number of draws
    rng, ref = random.Random(3), random.Random(3)                                  # a batch is B samples in a row
    got = data.draw_augment(rng, 5)
    assert got.tolist() == [int(data.draw_augment(ref, 1)[0]) for _ in range(5)] and rng.random() == ref.random()
    assert len(set(flags[0].tolist())) == 8                                        # every flag value occurs
    return dict(seeds=32, settings=4)


# ---------------------------------------------------------------------------------------------------------------------
# g. refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raises(exc, fn, *args, **kw):
    try:
        fn(*args, **kw)
    except exc:
        return True
    except Exception as e:                                                         # noqa: BLE001
        raise AssertionError("expected %s, got %r" % (exc, e))
    raise AssertionError("expected %s, nothing was raised" % (exc,))


def check_refusals(device):
    lib = _lib.get()
    st = _lib.stream()
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=device)                       # noqa: E731
    tb = _tables(48, 64, 8, device)
    p, pu8, pi = ops._p, ops._pu8, ops._pi32
    sentinel = torch.full((1, 3, 6, 8), -7.0, device=device)

    def lr_rc(frames, H, W, s, ch, cw, tr):
        return lib.dasr_batch_lr_u8(pu8(frames), p(sentinel), p(tb[0]), pi(tb[1]), p(tb[2]), pi(tb[3]), None, None, 1, H, W, s,
                                    ch, cw, tr, st)

    # H % s != 0
    assert lr_rc(u8(1, 47, 64, 3), 47, 64, 8, 5, 8, 0) == E_SHAPE
    assert _raises(ValueError, ops.batch_lr_u8, u8(1, 47, 64, 3), 8, tb)
    assert _raises(ValueError, data.BatchMaker(8, device=device).make, np.zeros((1, 47, 64, 3), np.uint8),
                   np.zeros((1, 1, 5, 8), np.float32))
    # a side shorter than the reflection (8 x 8 at s = 8: the reference raises there)
    assert lr_rc(u8(1, 8, 8, 3), 8, 8, 8, 1, 1, 0) == E_SHAPE
    assert _raises(ValueError, data.resize_tables, 8, 8)
    assert _raises(ValueError, data.BatchMaker(8, device=device).make, np.zeros((1, 8, 8, 3), np.uint8),
                   np.zeros((1, 1, 1, 1), np.float32))
    t8 = tuple(torch.zeros(sh, dtype=dt, device=device) for sh, dt in (((1, 32), torch.float32), ((1,), torch.int32)) * 2)
    assert _raises(ValueError, ops.batch_lr_u8, u8(1, 8, 8, 3), 8, t8)
    # a scale without a kernel
    assert lr_rc(u8(1, 48, 64, 3), 48, 64, 16, 3, 4, 0) == E_UNSUPPORTED
    assert _raises(ValueError, data.resize_tables, 48, 16)
    # transpose with a window that is not square
    fl = torch.tensor([4], dtype=torch.uint8, device=device)
    assert lr_rc(u8(1, 48, 64, 3), 48, 64, 8, 6, 8, 1) == E_SHAPE
    assert lib.dasr_batch_gt_u8(pu8(u8(1, 48, 64, 3)), p(torch.zeros((1, 3, 48, 64), device=device)), None, pu8(fl), 1, 48, 64,
                                8, 6, 8, 1, st) == E_SHAPE
    x = torch.zeros((1, 1, 6, 8), device=device)
    assert lib.dasr_batch_plane_f32(p(x), p(torch.zeros_like(x)), None, pu8(fl), 1, 1, 6, 8, 6, 8, 1, st) == E_SHAPE
    xb = torch.zeros((1, 1, 6, 8), dtype=torch.uint8, device=device)
    assert lib.dasr_batch_plane_u8(pu8(xb), pu8(torch.zeros_like(xb)), None, pu8(fl), 1, 1, 6, 8, 6, 8, 1, st) == E_SHAPE
    assert _raises(ValueError, ops.batch_lr_u8, u8(1, 48, 64, 3), 8, tb, flags=fl, allow_transpose=True)
    assert _raises(ValueError, ops.batch_gt_u8, u8(1, 48, 64, 3), 8, flags=fl, allow_transpose=True)
    assert _raises(ValueError, ops.batch_plane, x, flags=fl, allow_transpose=True)
    assert _raises(ValueError, data.BatchMaker(8, device=device).make, np.zeros((1, 48, 64, 3), np.uint8),
                   np.zeros((1, 1, 6, 8), np.float32), np.array([4], dtype=np.uint8))
    # a crop outside the frame
    assert lr_rc(u8(1, 48, 64, 3), 48, 64, 8, 7, 8, 0) == E_SHAPE
    assert lib.dasr_batch_gt_u8(pu8(u8(1, 48, 64, 3)), p(torch.zeros((1, 3, 48, 72), device=device)), None, None, 1, 48, 64, 8,
                                6, 9, 0, st) == E_SHAPE
    assert lib.dasr_batch_plane_f32(p(x), p(torch.zeros((1, 1, 7, 8), device=device)), None, None, 1, 1, 6, 8, 7, 8, 0, st) == E_SHAPE
    assert _raises(ValueError, ops.batch_lr_u8, u8(1, 48, 64, 3), 8, tb, (7, 8))
    assert _raises(ValueError, ops.batch_plane, x, (6, 9))
    mk = data.BatchMaker(8, crop=(4, 4), device=device)
    hr0, d0 = np.zeros((1, 48, 64, 3), np.uint8), np.zeros((1, 1, 6, 8), np.float32)
    assert _raises(ValueError, mk.make, hr0, d0, None, np.array([(3, 0)]))
    assert _raises(ValueError, mk.make, hr0, d0, None, np.array([(0, -1)]))
    assert _raises(ValueError, data.BatchMaker(8, crop=(7, 4), device=device).make, hr0, d0)
    assert _raises(ValueError, data.BatchMaker(8, device=device).make, hr0, d0, None, np.array([(0, 0)]))   # origins without crop
    # wrong dtypes
    assert _raises(TypeError, ops.batch_lr_u8, torch.zeros((1, 48, 64, 3), device=device), 8, tb)
    assert _raises(TypeError, ops.batch_gt_u8, torch.zeros((1, 48, 64, 3), device=device), 8)
    assert _raises(TypeError, ops.batch_plane, torch.zeros((1, 1, 6, 8), dtype=torch.float64, device=device))
    assert _raises(TypeError, ops.batch_lr_u8, u8(1, 48, 64, 3), 8, tb, flags=torch.zeros((1,), dtype=torch.int32, device=device))
    assert _raises(TypeError, ops.batch_lr_u8, u8(1, 48, 64, 3), 8, tb, (4, 4), torch.zeros((1, 2), dtype=torch.int64, device=device))
    assert _raises(TypeError, ops.batch_lr_u8, u8(1, 48, 64, 3), 8, tb, out=torch.zeros((1, 3, 6, 8), dtype=torch.float64, device=device))
    assert _raises(TypeError, data.BatchMaker(8, device=device).make, hr0.astype(np.float32), d0)
    assert _raises(TypeError, data.BatchMaker(8, device=device).make, hr0, d0.astype(np.float64))
    assert _raises(TypeError, data.BatchMaker(8, device=device).make, hr0, d0, np.array([0], dtype=np.int64))
    # NULL pointers
    assert lib.dasr_batch_lr_u8(None, p(sentinel), p(tb[0]), pi(tb[1]), p(tb[2]), pi(tb[3]), None, None, 1, 48, 64, 8, 6, 8, 0, st) == -1
    assert lib.dasr_batch_gt_u8(None, None, None, None, 1, 48, 64, 8, 6, 8, 0, st) == -1
    assert lib.dasr_batch_plane_f32(None, None, None, None, 1, 1, 6, 8, 6, 8, 0, st) == -1
    # nothing was launched: the output every refused dasr_batch_lr_u8 call pointed at is untouched
    assert bool((sentinel == -7.0).all())
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# h. end to end
# ---------------------------------------------------------------------------------------------------------------------
TINY_X8 = dict(name="x8_nb1_light", scale=8, which=[], L=32, nb=1, B=1, H=4, W=4)
E2E_CROP, E2E_ORIGIN, E2E_FLAGS = (4, 4), (1, 3), 5                  # a square window off the grid; hflip + transpose


def _spread_depth(gen, h, w, window=None):
    """A depth map [1,h,w] whose K per-sample bins are all populated (an empty bin makes the reference's region loss 0 / 0);
    with ``window`` = (oy, ox, ch, cw) they are populated inside that window too, which then holds the minimum and maximum."""
    d = gen.uniform(0.05, 0.95, size=(h, w))
    if window is None:
        d = gen.permutation(np.linspace(0.0, 1.0, h * w)).reshape(h, w)
    else:
        oy, ox, ch, cw = window
        d[oy:oy + ch, ox:ox + cw] = gen.permutation(np.linspace(0.0, 1.0, ch * cw)).reshape(ch, cw)
    return d.astype(np.float32)[None]


def _e2e_inputs(seed, B=2):
    """B frames of the (48,64,8) class, depth maps and flags (48 x 64: no transpose) that differ from seed to seed."""
    fx = fixture(48, 64, 8)
    gen = np.random.default_rng(300 + seed)
    hr = np.stack([np.roll(fx["hr"], (seed + 3 * b, 5 * b), axis=(0, 1)) for b in range(B)])
    if seed % 2:
        hr = hr // 4                                                             # a dark batch: another loss level
    depth = np.stack([_spread_depth(gen, 6, 8) for b in range(B)])
    flags = np.array([(seed + 1 + 2 * b) % 4 for b in range(B)], dtype=np.uint8)
    return hr, depth, flags


def check_end_to_end(device):
    """One Trainer step on what BatchMaker.make returns, and one on the same batch packed by numpy as the reference's loader
    packs it (from the kernel's own full-frame LR).  Crop mode, so that the whole chain runs (LR window, GT window, depth
    window, masks binned before the cut, region bytes cut as bytes) and the step stays small.

    Bit for bit on both devices: the four tensors, the region bytes, and the network's forward output from either feed -
    everything the loss kernels read.  The losses themselves are bit-equal on the emulator.  On the MI355X they cannot be
    asked to be: dasr_loss_sums adds its terms with float atomics, so its result depends on arrival order - on IDENTICAL
    sr / gt / region it returned 10 different bit patterns in 12 launches, and twelve steps fed the very same make() tensors
    logged two different l_all (1.7820768 and 1.7820771) while the forward output had one bit pattern in 12 runs.  There
    the two steps' losses must agree within what reordering an fp32 sum of N non-negative terms can change, 2 (N - 1)
    2^-24 relative (each order is within (N - 1) 2^-24 sum|x| of the exact sum), N = 3 * 32 * 32 terms: 3.7e-4."""
    (ch, cw), (oy, ox), f = E2E_CROP, E2E_ORIGIN, E2E_FLAGS
    fx = fixture(48, 64, 8)
    hr = fx["hr"][None]
    depth = _spread_depth(np.random.default_rng(77), 6, 8, (oy, ox, ch, cw))[None]
    mk = data.BatchMaker(8, K, crop=(ch, cw), device=device)
    batch = mk.make(hr, depth, np.array([f], dtype=np.uint8), np.array([(oy, ox)]))
    assert [tuple(t.shape) for t in batch] == [(1, 3, ch, cw), (1, 3, 8 * ch, 8 * cw), (1, 1, ch, cw), (1, K, ch, cw)]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in batch)
    assert int(batch[3].sum(dim=(0, 2, 3)).min()) >= 1                            # every region is populated

    # the numpy path
    lq_full = ops.batch_lr_u8(torch.from_numpy(hr).to(device), 8, _tables(48, 64, 8, device)).cpu().numpy()[0]
    full_masks = prep.depth_to_masks(torch.from_numpy(depth).to(device), K)
    cut = lambda a, s=1: a[:, s * oy:s * (oy + ch), s * ox:s * (ox + cw)]                          # noqa: E731
    aug = lambda chw: np.ascontiguousarray(np.transpose(np_augment(np.transpose(chw, (1, 2, 0)), f), (2, 0, 1)))  # noqa: E731
    gt_full = np.transpose((hr[0].astype(np.float32) / 255.)[:, :, [2, 1, 0]], (2, 0, 1))
    lq2, gt2, dm2, mk2 = (torch.from_numpy(aug(a)[None]).to(device) for a in
                          (cut(lq_full), cut(gt_full, 8), cut(depth[0]), cut(full_masks[0].cpu().numpy())))
    region2 = torch.from_numpy(aug(cut(full_masks._dasr_region.cpu().numpy()))).to(device)
    mk2._dasr_region, mk2._dasr_version = region2, ops.tensor_version(mk2)        # what prep.depth_to_masks attaches
    other = (lq2, gt2, dm2, mk2)
    for a, b in zip(batch, other):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(batch[3]._dasr_region, region2)

    logs, srs = [], []
    for tensors in (batch, other):
        net, _ = build_net(TINY_X8, device)
        with torch.no_grad():
            srs.append(net(*tensors[:1], *tensors[2:]).clone())                   # net(lq, depth, masks)
        logs.append(harness.Trainer(net, K).optimize_parameters(*tensors))
    assert torch.equal(srs[0].view(torch.int32), srs[1].view(torch.int32))         # the forward: deterministic everywhere
    n_terms = srs[0].numel()
    reorder = 2.0 * (n_terms - 1) * 2.0 ** -24
    for k in ("l_all", "l_pix", "l_dynamic"):
        a, b = logs[0][k].detach().float().cpu().reshape(-1), logs[1][k].detach().float().cpu().reshape(-1)
        assert torch.isfinite(a).all() and a.numel() == 1, (k, a)
        if device == "cpu":
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, a, b)
        else:
            print("%s: %.9g vs %.9g (bound %.3g relative)" % (k, float(a), float(b), reorder))
            assert abs(float(a) - float(b)) <= reorder * abs(float(a)), (k, float(a), float(b))
    # the static buffers: a second call hands out the same tensors, rewritten
    again = mk.make(255 - hr, depth, np.array([2], dtype=np.uint8), np.array([(2, 0)]))
    assert all(x is y for x, y in zip(batch, again))
    assert not torch.equal(again[0], lq2)
    return {k: float(v) for k, v in logs[0].items()}


def check_graphed_trainer(device):
    """GPU only (the bound is a tolerance on chaotic training, like its model's: it can be missed by run-to-run noise of the
    atomically summed weight gradients, not only by a fault of BatchMaker).  BatchMaker (whole frames, two samples) feeds Trainer(use_graph=True) through three eager steps, the capture
    and three replays; its static outputs ARE the captured inputs (no copy in between), so a replay reads what the latest
    make() wrote.  Against an eager trainer fed with clones of the same batches: the per-step losses agree to 3e-3 (the bound
    and its reason are test_gpu_parity.test_graphed_trainer_matches_eager's: training is chaotic at this scale and the
    weight gradients are summed with atomics); consecutive batches differ by far more."""
    runs = {}
    for use_graph in (False, True):
        net, _ = build_net(TINY_X8, device)
        tr = harness.Trainer(net, K, use_graph=use_graph)
        mk = data.BatchMaker(8, K, device=device)
        losses = []
        for step in range(7):
            batch = mk.make(*_e2e_inputs(step))
            if not use_graph:
                batch = tuple(t.clone() for t in batch[:3]) + (prep.depth_to_masks(batch[2].clone(), K),)
            losses.append(float(tr.optimize_parameters(*batch)["l_all"]))
        assert (tr._graph is not None) == use_graph
        if use_graph:
            assert all(a is b for a, b in zip(tr._static, batch))                  # the fast path: nothing was copied
        runs[use_graph] = losses
    le, lg = runs[False], runs[True]
    print("graphed vs eager losses", le, lg)
    assert all(abs(a - b) <= 3e-3 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    # consecutive batches differ by ten times the bound above: a replay that read the previous batch would show
    assert min(abs(a - b) for a, b in zip(le[:-1], le[1:])) > 3e-2, le
    return dict(eager=le, graph=lg)
