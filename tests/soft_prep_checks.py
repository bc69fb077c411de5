"""Soft depth masks from the depth map (csrc/prep.hip: dasr_depth_to_masks_soft; ops.depth_to_masks_soft;
prep.depth_to_soft_masks; FrameUpscaler / validate_u8 / BatchMaker ``soft_masks=``).  Each check takes the device ("cpu": the
kernel emulator, "cuda": the MI355X); tests/test_soft_prep.py runs them.

The rule is restated here in numpy (``np_rule``), operation by operation, once in float32 (the kernel must give the same
bits) and once in float64 (the properties and the error bound)."""
import functools
import os

import numpy as np
import torch

from dasr_amd import _lib, data, graph, harness, ops, prep, synth, validate
from dasr_amd.depthnet import DepthNet
from dasr_amd.video import FrameUpscaler
from oracle import depthnet_oracle as O
from tests.golden_cases import DEPTHNET_CASES
from tests.parity_checks import _oracle_sd, build_net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4
SHAPES = [(2, 5, 7), (3, 4, 8), (2, 3, 11), (1, 72, 64)]      # scalar only | vector only | mixed, odd plane offsets | 2 partials
KS = (1, 2, 7, 10, 16)
WIDTHS = (1.0, 0.5, 0.125)
X4 = next(c for c in DEPTHNET_CASES if c["name"] == "x4_nb4")
TINY_X8 = dict(name="x8_nb1_light", scale=8, which=[], L=32, nb=1, B=1, H=4, W=6)      # no depth blocks: host plumbing only


def err_bound(K, width):
    """Max |float32 plane - float64 plane|.  u = (v - lo) / interval <= K is the result of a subtraction and a division
    (2^-24 relative each) by an interval that itself carries a subtraction and a division: |du| <= 4 * 2^-24 * K.
    r = u - k is exact, the band divides by width (du / width), and r / width, 0.5 - ., 1 - . add one rounding each of a
    value below 1 where the weight is not clamped: 3 * 2^-25.  Doubled for margin: 8 * 2^-24 * K / width."""
    return 8.0 * 2.0 ** -24 * K / width


def np_rule(depth, K, width, fixed_range, dtype=np.float32):
    """The membership rule of include/dasr.h on ``depth`` [B,h,w] float32, every operation in ``dtype``: -> [B,K,h,w]."""
    f = dtype
    B, h, w = depth.shape
    HW = h * w
    out = np.zeros((B, K, HW), dtype=f)
    idx = np.arange(HW)
    for b in range(B):
        v = depth[b].reshape(HW).astype(f)                      # (exact: float32 -> float32 / float64)
        lo, hi = (f(0), f(1)) if fixed_range else (v.min(), v.max())
        interval = f(f(hi - lo) / f(K))
        if not interval > 0:
            out[b, 0] = f(1)
            continue
        u = (v - lo) / interval
        u = np.minimum(np.maximum(u, f(0)), f(K))
        k = np.minimum(np.floor(u).astype(np.int64), K - 1)
        r = u - k.astype(f)
        low = r < f(0.5)
        n = np.where(low, k - 1, k + 1)
        s = np.where(low, f(0.5) - r / f(width), f(0.5) - (f(1) - r) / f(width))
        s = np.maximum(s, f(0))
        s[(n < 0) | (n >= K)] = f(0)
        assert u.dtype == r.dtype == s.dtype == f
        out[b, k, idx] = f(1) - s
        on = s > 0
        out[b, n[on], idx[on]] = s[on]
    return out.reshape(B, K, h, w)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(d, K, width, fixed, device):
    return ops.depth_to_masks_soft(torch.tensor(d, device=device), K, width, fixed).cpu().numpy()


@functools.lru_cache(maxsize=None)
def planted_maps(shape, K, fixed, rot):
    """hash_uniform maps [B,h,w] float32 with values planted on purpose (never modified afterwards).  Per-sample range:
    values in [0.125, 0.875] with the minimum at the first and the maximum at the last pixel (two min / max partials at
    HW > PREP_CHUNK), then exact edges and bin centres as the rule computes them (lo + interval * i) and the floats one ulp
    either side of each edge.  Fixed range: values in [0,1) and the same around the edges i / K, plus values below 0, above
    1, exactly 0 and exactly 1.  The planted list is rotated by ``rot`` so that small maps cover different parts of it."""
    f = np.float32
    B, h, w = shape
    HW = h * w
    d = synth.hash_uniform(B * HW, "soft_prep/%s/%d/%d" % (shape, K, fixed)).numpy().astype(f).reshape(B, HW)
    for b in range(B):
        if fixed:
            lo, hi = f(0), f(1)
            extra = [f(-0.25), f(1.5), f(0), f(1), np.nextafter(f(0), f(-1)), np.nextafter(f(1), f(2))]
            first = 0
        else:
            d[b] = f(0.125) + d[b] * f(0.75)
            lo, hi = f(0.0625) + f(0.001) * f(b), f(0.9375) - f(0.003) * f(b)
            d[b, 0], d[b, -1] = lo, hi
            extra, first = [], 1
        interval = f(f(hi - lo) / f(K))
        planted = list(extra)
        for i in range(K + 1):
            e = f(lo + f(interval * f(i)))
            planted += [e, np.nextafter(e, f(-1)), np.nextafter(e, f(2))]
            if i < K:
                planted.append(f(lo + f(interval * f(i + 0.5))))
        if not fixed:                                           # nothing may leave the pinned range
            planted = [p for p in planted if lo <= p <= hi]
        r = (rot + 7 * b) % len(planted)
        planted = (planted[r:] + planted[:r])[:max(0, HW - 2)]
        d[b, first:first + len(planted)] = planted
        if not fixed:
            assert d[b].min() == lo and d[b].max() == hi
    d = d.reshape(B, h, w)
    d.setflags(write=False)
    return d


def _with_constant(d):
    """The batch plus one constant map."""
    return np.concatenate([d, np.full((1,) + d.shape[1:], np.float32(0.375))])


# ---------------------------------------------------------------------------------------------------------------------
# the rule, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def check_soft_rule_bits(device):
    n = 0
    for si, shape in enumerate(SHAPES):
        for K in KS:
            for wi, width in enumerate(WIDTHS):
                for fixed in (False, True):
                    base = planted_maps(shape, K, fixed, 11 * wi + 5 * si)
                    for d in (base, _with_constant(base)):
                        got = _run(d, K, width, fixed, device)
                        want = np_rule(d, K, width, fixed)
                        assert got.shape == want.shape and got.dtype == np.float32
                        same = _bits(got) == _bits(want)
                        assert same.all(), (shape, K, width, fixed, int((~same).sum()),
                                            float(np.abs(got.astype(np.float64) - want).max()))
                        n += 1
                    if not fixed:                               # the constant map: plane 0, nothing else
                        assert (got[-1, 0] == 1).all() and (K == 1 or (got[-1, 1:] == 0).all())
    # out= writes into the caller's buffer, every element (a poisoned buffer comes back clean)
    d = planted_maps((2, 3, 11), 7, False, 0)
    buf = torch.full((2, 7, 3, 11), float("nan"), device=device)
    res = ops.depth_to_masks_soft(torch.tensor(d, device=device), 7, 0.5, out=buf)
    assert res is buf and (_bits(buf.cpu().numpy()) == _bits(np_rule(d, 7, 0.5, False))).all()
    # [B,1,h,w] input, and a plane buffer 4 bytes off the 16-byte grid (scalar stores where the vector path was)
    d = planted_maps((3, 4, 8), 10, False, 0)
    store = torch.full((3 * 10 * 32 + 1,), float("nan"), device=device)
    off = store[1:].view(3, 10, 4, 8)
    ops.depth_to_masks_soft(torch.tensor(d[:, None], device=device), 10, 1.0, out=off)
    assert (_bits(off.cpu().numpy()) == _bits(np_rule(d, 10, 1.0, False))).all()
    return dict(cases=n + 2)


# ---------------------------------------------------------------------------------------------------------------------
# properties, against float64
# ---------------------------------------------------------------------------------------------------------------------
def check_soft_rule_properties(device):
    """Measured worst |float32 - float64| over these cases, as a share of err_bound(K, width) (emulator and MI355X give
    the same bits, check_soft_rule_bits): 0.143; printed below."""
    worst = 0.0
    for shape in ((2, 16, 20), (2, 3, 11), (1, 72, 64)):
        for K in KS:
            for wi, width in enumerate(WIDTHS):
                for fixed in (False, True):
                    d = _with_constant(planted_maps(shape, K, fixed, 3 * wi))
                    got = _run(d, K, width, fixed, device).astype(np.float64)
                    want = np_rule(d, K, width, fixed, np.float64)
                    assert got.min() >= 0.0 and got.max() <= 1.0
                    nz = got != 0
                    assert nz.sum(axis=1).max() <= 2 and nz.sum(axis=1).min() >= 1
                    first = nz.argmax(axis=1)
                    last = K - 1 - nz[:, ::-1].argmax(axis=1)
                    assert (last - first <= 1).all()                               # the two are neighbours
                    assert np.abs(got.sum(axis=1) - 1.0).max() <= 2.0 ** -23
                    e = float(np.abs(got - want).max())
                    worst = max(worst, e / err_bound(K, width))
                    assert e <= err_bound(K, width), (shape, K, width, fixed, e, err_bound(K, width))
    print("soft rule: worst error / bound %.3f" % worst)

    # width 0.125: away from the edges the planes are the reference's one-hot planes
    shares = {}
    for shape in ((1, 72, 64), (2, 16, 20)):
        for K in (2, 7, 10, 16):
            for fixed in (False, True):
                B, h, w = shape
                d = synth.hash_uniform(B * h * w, "soft_prep/uniform/%s/%d" % (shape, K)).numpy().astype(np.float32).reshape(shape)
                dt = torch.from_numpy(d).to(device)
                soft = ops.depth_to_masks_soft(dt, K, 0.125, fixed).cpu().numpy()
                edges = prep.fixed_range_edges(K, dt.device) if fixed else None
                hard = ops.depth_to_masks(dt, K, edges)[0].cpu().numpy()
                far = np.zeros(shape, dtype=bool)
                for b in range(B):
                    lo, hi = (np.float32(0), np.float32(1)) if fixed else (d[b].min(), d[b].max())
                    interval = np.float32(np.float32(hi - lo) / np.float32(K))
                    e = np.array([np.float32(lo + np.float32(interval * np.float32(i))) for i in range(K + 1)], dtype=np.float64)
                    dist = np.abs(d[b].astype(np.float64)[..., None] - e).min(axis=-1)
                    far[b] = dist > 0.07 * float(interval)
                    if not fixed:                          # the maximum: plane K-1 here; there no bin (or, where the last
                        top = d[b] == hi                   # edge rounds up past it, bin K-1): excepted
                        assert (soft[b, K - 1][top] == 1).all()
                        far[b] &= ~top
                sel = np.broadcast_to(far[:, None], soft.shape)
                assert np.array_equal(soft[sel], hard[sel]), (shape, K, fixed)
                shares["%s/K%d/%s" % ("x".join(map(str, shape)), K, "fixed" if fixed else "range")] = float(far.mean())
                assert far.mean() >= 0.8, (shape, K, fixed, float(far.mean()))
    return dict(worst_over_bound=round(worst, 3), min_share=round(min(shares.values()), 3))


# ---------------------------------------------------------------------------------------------------------------------
# continuity: the point of the feature
# ---------------------------------------------------------------------------------------------------------------------
def check_soft_continuity(device):
    """A [1,16,20] map on the 2^-16 grid with lo = 0 and hi = 1 pinned (the two extreme pixels stay), and the same map
    plus eps = 2^-12 (hi - lo) - exact in float32 on that grid, so the perturbation is eps and nothing else."""
    K, f = 10, np.float32
    eps = f(2.0 ** -12)
    g = np.floor(synth.hash_uniform(320, "soft_prep/continuity").numpy() * (0.75 * 65536)) / 65536 + 0.125   # [0.125, 0.875)
    d = g.astype(f).reshape(1, 16, 20)
    d[0, 0, 0], d[0, -1, -1] = 0.0, 1.0
    interval = f(f(1) / f(K))
    edge = f(f(0) + f(interval * f(5)))
    d[0, 3, 3] = f((np.ceil(float(edge) * 65536) - 1) / 65536)                      # within 2^-16 < eps below edge 5
    assert d[0, 3, 3] < edge <= d[0, 3, 3] + eps
    d2 = d + eps
    d2[0, 0, 0], d2[0, -1, -1] = 0.0, 1.0
    assert np.array_equal(d2.astype(np.float64), np.where((d == 0) | (d == 1), d, d.astype(np.float64) + float(eps)))
    out = {}
    for width in WIDTHS:
        a, b = _run(d, K, width, False, device), _run(d2, K, width, False, device)
        step = float(np.abs(a.astype(np.float64) - b).max())
        bound = float(eps) / (float(interval) * width) + err_bound(K, width)
        out["w%g" % width] = (step, bound)
        assert 0 < step <= bound, (width, step, bound)
    t, t2 = torch.from_numpy(d).to(device), torch.from_numpy(d2).to(device)
    h1, h2 = ops.depth_to_masks(t, K)[0].cpu().numpy(), ops.depth_to_masks(t2, K)[0].cpu().numpy()
    assert np.abs(h1 - h2).max() == 1.0                         # the one-hot planes jump
    assert h1[0, 4, 3, 3] == 1 and h2[0, 5, 3, 3] == 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raises(exc, fn, *args, **kw):
    try:
        fn(*args, **kw)
    except exc:
        return True
    except Exception as e:                                                         # noqa: BLE001
        raise AssertionError("expected %s, got %r" % (exc, e))
    raise AssertionError("expected %s, nothing was raised" % (exc,))


def check_soft_refusals(device):
    lib, st, p = _lib.get(), _lib.stream(), ops._p
    d = torch.full((2, 5, 7), 0.5, device=device)
    sentinel = torch.full((2, 17, 5, 7), -7.0, device=device)
    nbytes = int(lib.dasr_depth_to_masks_soft_workspace(2, 35))
    assert nbytes >= 16
    ws = torch.zeros((nbytes // 4,), device=device)

    def rc(K=10, width=1.0, masks=sentinel, wsb=nbytes, depth=d):
        return lib.dasr_depth_to_masks_soft(p(depth, True), p(masks, True), p(ws), wsb, 2, 35, K, width, 0, st)

    for width in (0.0, -1.0, 1.5, float("nan")):
        assert rc(width=width) == E_SHAPE, width
        assert _raises(ValueError, ops.depth_to_masks_soft, d, 10, width)
        assert _raises(ValueError, prep.depth_to_soft_masks, d, 10, False, width)
        assert _raises(ValueError, FrameUpscaler, torch.nn.Linear(1, 1), soft_masks=width)
        assert _raises(ValueError, data.BatchMaker, 4, soft_masks=width, device=device)
    assert rc(K=17) == E_UNSUPPORTED
    assert _raises(ValueError, ops.depth_to_masks_soft, d, 17)
    assert _raises(ValueError, prep.depth_to_soft_masks, d, 17)
    assert rc(K=0) == E_SHAPE
    for bad in (d.double(), d.half(), (d * 255).to(torch.uint8)):
        assert _raises(TypeError, ops.depth_to_masks_soft, bad, 10)
        assert _raises(TypeError, prep.depth_to_soft_masks, bad, 10)
    assert rc(wsb=nbytes - 1) == E_WORKSPACE
    assert rc(masks=None) == E_NULL
    assert rc(depth=None) == E_NULL
    assert _raises(ValueError, ops.depth_to_masks_soft, d, 10, out=torch.zeros((2, 9, 5, 7), device=device))
    assert bool((sentinel == -7.0).all())                       # nothing was launched
    ok = torch.full((2, 10, 5, 7), -7.0, device=device)
    assert rc(masks=ok) == 0 and bool((ok != -7.0).all())
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# the stamp
# ---------------------------------------------------------------------------------------------------------------------
def check_prep_stamp(device):
    d = torch.tensor(planted_maps((2, 5, 7), 10, False, 0), device=device)
    for dd in (d, d[:, None]):
        m = prep.depth_to_soft_masks(dd, 10, width=0.5)
        assert tuple(m.shape) == (2, 10, 5, 7) and m.dtype == torch.float32
        assert prep.marked_soft(m) is True
        assert m._dasr_region is None and graph.attached_region(m) is None
    # attach_region answers from the stamp: no compression pass (hence no flag to read back) is reached
    keep = ops.mask_compress

    def no_launch(*a, **k):
        raise AssertionError("attach_region launched dasr_mask_compress on a soft-stamped tensor")

    ops.mask_compress = no_launch
    try:
        assert prep.attach_region(m) is False
    finally:
        ops.mask_compress = keep
    assert graph.attached_region(m) is None
    same = prep.depth_to_soft_masks(d, 10, False, 0.5)
    assert torch.equal(same, m) and not torch.equal(prep.depth_to_soft_masks(d, 10, True, 0.5), m)
    m.mul_(1.0)                                                 # an in-place edit drops the stamp
    assert prep.marked_soft(m) is False
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# the whole net's forward on these planes
# ---------------------------------------------------------------------------------------------------------------------
def check_whole_net_forward(device):
    """Forward only (gate: parity_checks._compare_with_oracle's, 2e-4)."""
    out = {}
    for K in (10, 16):
        cfg = O.make_cfg(which_ResBlk_depth=[0, 1], nb=4, scale=2, depth_latent_ch=32, depthRangeNum=K)
        net = DepthNet(which_ResBlk_depth=[0, 1], nb=4, scale=2, depth_latent_ch=32, depthRangeNum=K)
        synth.closed_form_fill_(net.state_dict().items())
        net = net.to(device)
        lq, _, dm, _ = synth.closed_form_batch(1, 2, 8, 12, 2, K)
        mk = prep.depth_to_soft_masks(dm.to(device), K, width=1.0)
        assert prep.marked_soft(mk) and float((mk > 0).sum(dim=1).float().mean()) > 1.0      # soft indeed
        with torch.no_grad():
            sr = net(lq.to(device), dm.to(device), mk)
            ref = O.depthnet_forward(_oracle_sd(net), cfg, lq, dm, mk.cpu())
        err = (sr.cpu() - ref).abs().max().item()
        out["K%d" % K] = err
        assert err <= 2e-4, (K, err)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# BatchMaker
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_frames(B):
    """B different frames / depth maps of the 48x48x4 class (rolled copies of the fixture's); never modified."""
    with np.load(os.path.join(GOLDEN, "batch_48x48x4.npz")) as z:
        hr, depth = z["hr"], z["depth"]
    frames = np.stack([np.roll(hr, (b, 2 * b), axis=(0, 1)) for b in range(B)])
    depths = np.stack([np.roll(depth, (b, 3 * b), axis=(1, 2)) for b in range(B)])
    return frames, depths


def _torch_augment(x, f):
    """augment (codes/data/util.py:107-114) of [..., h, w] with torch indexing."""
    if f & 1:
        x = x.flip(-1)
    if f & 2:
        x = x.flip(-2)
    if f & 4:
        x = x.transpose(-1, -2)
    return x


def _eq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_batch_maker_soft(device):
    K, width = 10, 0.5
    # (a) whole frames, flags 0..3
    frames, depths = _fixture_frames(4)
    flags = np.arange(4, dtype=np.uint8)
    mk = data.BatchMaker(scale=4, num_masks=K, soft_masks=width, device=device)
    ref = data.BatchMaker(scale=4, num_masks=K, device=device)
    lq, gt, depth, masks = mk.make(frames, depths, flags)
    want = ref.make(frames, depths, flags)
    assert all(_eq(a, b) for a, b in zip((lq, gt, depth), want[:3]))
    assert _eq(masks, prep.depth_to_soft_masks(depth, K, width=width))
    assert prep.marked_soft(masks) and masks._dasr_region is None and graph.attached_region(masks) is None
    assert not _eq(masks, want[3])
    buf = next(iter(mk._shapes.values()))
    assert not hasattr(buf, "region") and not hasattr(buf, "full_region") and not hasattr(buf, "full_masks")
    again = mk.make(frames[::-1].copy(), depths[::-1].copy(), flags)              # re-stamped after every make
    assert again[3] is masks and prep.marked_soft(masks)
    assert _eq(masks, prep.depth_to_soft_masks(again[2], K, width=width))

    # (b) crop: binned from the FULL depth map, then cut and augmented
    frames, depths = _fixture_frames(8)
    flags = np.arange(8, dtype=np.uint8)
    origins = np.array([(0, 0), (4, 4), (3, 1), (4, 0)] * 2)
    mk = data.BatchMaker(scale=4, num_masks=K, soft_masks=width, crop=(8, 8), device=device)
    ref = data.BatchMaker(scale=4, num_masks=K, crop=(8, 8), device=device)
    lq, gt, depth, masks = mk.make(frames, depths, flags, origins)
    want = ref.make(frames, depths, flags, origins)
    assert all(_eq(a, b) for a, b in zip((lq, gt, depth), want[:3]))
    full = prep.depth_to_soft_masks(torch.from_numpy(depths).to(device), K, width=width)
    for b, (f, (oy, ox)) in enumerate(zip(flags.tolist(), origins.tolist())):
        assert _eq(masks[b], _torch_augment(full[b][:, oy:oy + 8, ox:ox + 8], f)), ("crop", b)
    assert not _eq(masks, prep.depth_to_soft_masks(depth, K, width=width))        # a window has another range
    assert prep.marked_soft(masks) and masks._dasr_region is None
    buf = next(iter(mk._shapes.values()))
    assert hasattr(buf, "full_masks") and not hasattr(buf, "region") and not hasattr(buf, "full_region")
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# defaults
# ---------------------------------------------------------------------------------------------------------------------
def _frames(h, w, B, seed):
    gen = np.random.default_rng(4000 + seed)
    return gen.integers(0, 256, size=(B, h, w, 3), dtype=np.uint8), torch.from_numpy(gen.random(size=(B, 1, h, w), dtype=np.float32))


def check_defaults_unchanged(device):
    """``soft_masks=None`` is the call without the keyword: same outputs, same buffers."""
    case = X4 if device == "cuda" else TINY_X8           # (an emulator forward of X4 costs seconds, and four run here)
    net, _ = build_net(case, device)
    h, w, s = case["H"], case["W"], case["scale"]
    f, d = _frames(h, w, 1, 0)
    ups = [FrameUpscaler(net, use_graph=False), FrameUpscaler(net, use_graph=False, soft_masks=None)]
    a, b = (u.upscale(f, d) for u in ups)
    assert np.array_equal(a, b) and a.shape == (1, s * h, s * w, 3)
    slots = [next(iter(u._shapes.values())).slots[0] for u in ups]
    assert sorted(vars(slots[0])) == sorted(vars(slots[1]))
    assert ups[1].soft_masks is None

    gt = torch.from_numpy(np.random.default_rng(5).random(size=(1, 3, s * h, s * w), dtype=np.float32))
    items = [(f, gt, d)]
    r0 = validate.validate_u8(net, items, s)
    r1 = validate.validate_u8(net, items, s, soft_masks=None)
    assert r0 == r1 and r0[2] == 1

    frames, depths = _fixture_frames(4)
    flags = np.array([0, 5, 3, 6], dtype=np.uint8)
    for crop, origins in ((None, None), ((8, 8), np.array([(0, 0), (4, 4), (3, 1), (4, 0)]))):
        mks = [data.BatchMaker(4, 10, crop=crop, device=device), data.BatchMaker(4, 10, crop=crop, device=device, soft_masks=None)]
        outs = [m.make(frames, depths, flags, origins) for m in mks]
        assert all(_eq(x, y) for x, y in zip(*outs))
        assert torch.equal(outs[0][3]._dasr_region, outs[1][3]._dasr_region)
        assert graph.attached_region(outs[1][3]) is not None and not prep.marked_soft(outs[1][3])
        bufs = [next(iter(m._shapes.values())) for m in mks]
        assert sorted(vars(bufs[0])) == sorted(vars(bufs[1])) and hasattr(bufs[1], "region")
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# GPU only
# ---------------------------------------------------------------------------------------------------------------------
def _img2tensor(img):
    """The reference's formula (utils/util.py:596-605): BGR uint8 HWC -> RGB float CHW."""
    img = img.astype(np.float32) / 255.
    return torch.from_numpy(np.ascontiguousarray(np.transpose(img[:, :, [2, 1, 0]], (2, 0, 1)))).float()


def _via_validate(net, f, d, device, width):
    lq = torch.stack([_img2tensor(f[b]) for b in range(f.shape[0])]).to(device)
    dd = d.to(device)
    sr = validate.test(net, lq, dd, prep.depth_to_soft_masks(dd, width=width))
    return np.stack([validate.tensor2img(sr[b]) for b in range(f.shape[0])])


def check_upscaler_soft(device):
    out = {}
    f, d = _frames(12, 16, 2, 1)
    for dtype in ("fp32", "bf16"):
        net, _ = build_net(X4, device)
        net.set_compute_dtype(dtype)
        got = FrameUpscaler(net, soft_masks=1.0, use_graph=False).upscale(f, d)
        want = _via_validate(net, f, d, device, 1.0)
        assert got.dtype == np.uint8 and got.shape == want.shape == (2, 48, 64, 3)
        assert np.array_equal(got, want), (dtype, int((got != want).sum()))
        hard = FrameUpscaler(net, use_graph=False).upscale(f, d)
        out[dtype] = int((got != hard).sum())
        assert out[dtype] >= 1, dtype                            # the feature is switched on
    return out


def check_upscaler_soft_graph(device):
    queues = os.environ.get("GPU_MAX_HW_QUEUES")
    net, _ = build_net(X4, device)
    up_g = FrameUpscaler(net, soft_masks=1.0, use_graph=True)
    up_e = FrameUpscaler(net, soft_masks=1.0, use_graph=False)
    seq = [_frames(12, 16, 2, 10 + i) for i in range(5)]
    for i, (f, d) in enumerate(seq):
        assert np.array_equal(up_g.upscale(f, d), up_e.upscale(f, d)), i
    assert up_g.captures == 1 and up_g.replays >= 2, (up_g.captures, up_g.replays)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd["conv_output.weight"] = sd["conv_output.weight"] * 1.5
    net.load_state_dict(sd)
    f, d = seq[4]
    replays = up_g.replays
    after = up_g.upscale(f, d)                                   # stale graph: dropped, the shape warms up again
    assert up_g.replays == replays
    assert np.array_equal(after, FrameUpscaler(net, soft_masks=1.0, use_graph=False).upscale(f, d))
    for i in range(2):
        assert np.array_equal(up_g.upscale(*seq[i]), up_e.upscale(*seq[i])), i
    assert up_g.captures == 2, up_g.captures
    assert os.environ.get("GPU_MAX_HW_QUEUES") == queues
    return dict(captures=up_g.captures, replays=up_g.replays)


def check_trainer_takes_soft_batches(device):
    K = 10
    frames, depths = _fixture_frames(2)
    flags = np.array([1, 2], dtype=np.uint8)
    case = dict(name="x4_nb4_dgb", scale=4, which=[0, 1], L=32, nb=4, B=2, H=12, W=12)
    logs = []
    for feed in ("maker", "marked"):
        net, _ = build_net(case, device)
        batch = data.BatchMaker(4, K, soft_masks=1.0, device=device).make(frames, depths, flags)
        if feed == "marked":
            batch = tuple(t.clone() for t in batch)
            prep.mark_soft(batch[3])
        logs.append({k: float(v) for k, v in harness.Trainer(net, K).optimize_parameters(*batch).items()})
    print("soft batches, eager first step:", logs)
    for k in ("l_all", "l_dynamic"):
        a, b = logs[0][k], logs[1][k]
        assert np.isfinite(a) and np.isfinite(b), (k, a, b)
        assert abs(a - b) <= 1e-6 * abs(a), (k, a, b)
    net, _ = build_net(case, device)
    tr = harness.Trainer(net, K, use_graph=True)
    mk = data.BatchMaker(4, K, soft_masks=1.0, device=device)
    losses = []
    for step in range(5):
        fr, dp = np.roll(frames, step, axis=1), np.roll(depths, step, axis=2)
        log = tr.optimize_parameters(*mk.make(fr, dp, flags))
        losses.append({k: float(v) for k, v in log.items()})
    assert tr._graph is not None
    assert all(np.isfinite(v) for log in losses for v in log.values()), losses
    return dict(eager=logs[0], graph=losses[-1])
