"""The pair encoding of two-plane soft depth masks (include/dasr.h): the producer dasr_depth_to_masks_soft_pair, the
pair-gather SEAN forward k_sean_fwd_pair behind dasr_sean_fwd_pair[_bf16], MaskPack / sean_mod, and the ``soft_pair=``
switch of FrameUpscaler / validate_u8 / test_u8.  Each check takes the device ("cpu": the kernel emulator, "cuda": the
MI355X); tests/test_soft_pair.py runs them.

References are float64 torch (tests/sean_exact_checks.reference on the DECODED planes, prep.pair_planes restated by hand
where the decoding itself is under test), never another entry point of the library - except where a check says so: the
planes of ops.depth_to_masks_soft, the region-only gather forward on pairs without a second plane, and the general forward
whose distance is printed, not gated."""
import contextlib
import math

import numpy as np
import torch

from dasr_amd import _lib, graph, harness, ops, prep, synth, validate
from dasr_amd.depthnet import DepthNet
from dasr_amd.video import FrameUpscaler
from oracle import depthnet_oracle as O
from tests import sean_exact_checks as sx
from tests import soft_prep_checks as sp
from tests.bf16_exact_checks import _nbad, _take
from tests.parity_checks import _compare_with_oracle, _oracle_sd, build_net

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
BASE = (2, 9, 33)                   # one row past an 8-row tile, one column past a 32-column tile
E_NULL, E_UNSUPPORTED = -1, -3


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _counting(mod, *names):
    """Call counters of ``mod.name`` for the duration of the block."""
    n = {nm: 0 for nm in names}
    keep = {nm: getattr(mod, nm) for nm in names}

    def wrap(nm):
        def f(*a, **k):
            n[nm] += 1
            return keep[nm](*a, **k)
        return f

    for nm in names:
        setattr(mod, nm, wrap(nm))
    try:
        yield n
    finally:
        for nm in names:
            setattr(mod, nm, keep[nm])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the producer
# ---------------------------------------------------------------------------------------------------------------------
def check_producer(device):
    """HW in {33, 35, 4608} x K in {1, 2, 10, 16} x width in {1, 0.125} x both range modes on the planted maps of
    soft_prep_checks (centres, edges, one ulp either side, the extremes) plus a constant map: planes bit-identical to
    ops.depth_to_masks_soft, pair_planes(pair) == planes bit for bit, |pair_s| <= 0.5, no -0.0 (bit pattern), a valid
    neighbour wherever pair_s != 0, and masks = NULL writes the same side-cars."""
    lib, st = _lib.get(), _lib.stream()
    n = second = 0
    for si, shape in enumerate(((2, 3, 11), (2, 5, 7), (1, 72, 64))):
        for K in (1, 2, 10, 16):
            for wi, width in enumerate((1.0, 0.125)):
                for fixed in (False, True):
                    d = torch.tensor(sp._with_constant(sp.planted_maps(shape, K, fixed, 11 * wi + 5 * si)), device=device)
                    want = ops.depth_to_masks_soft(d, K, width, fixed)
                    planes, pk, ps = ops.depth_to_masks_soft(d, K, width, fixed, pair=True)
                    what = (shape, K, width, fixed)
                    assert pk.dtype == torch.uint8 and ps.dtype == F32 and pk.shape == ps.shape == d.shape, what
                    assert _same_bits(planes, want), ("planes differ from dasr_depth_to_masks_soft", what)
                    assert _same_bits(prep.pair_planes(pk, ps, K), want), ("pair_planes(pair) != planes", what)
                    assert float(ps.abs().max()) <= 0.5 and int(pk.max()) < K, what
                    assert not bool((_bits(ps) == -2 ** 31).any()), ("-0.0 in pair_s", what)
                    nb = torch.where(ps < 0, pk.long() - 1, pk.long() + 1)
                    assert bool(((ps == 0) | ((nb >= 0) & (nb < K))).all()), ("neighbour outside 0..K-1", what)
                    # masks = NULL: the same side-cars, nothing else to write
                    B, HW = d.shape[0], d.shape[1] * d.shape[2]
                    pk2 = torch.full_like(pk, 255)
                    ps2 = torch.full_like(ps, -7.0)
                    nbytes = int(lib.dasr_depth_to_masks_soft_workspace(B, HW))
                    ws = torch.zeros((max(nbytes, 4) // 4,), device=device)
                    rc = lib.dasr_depth_to_masks_soft_pair(ops._p(d), None, _lib.ptr(pk2, dtype=torch.uint8), ops._p(ps2),
                                                           ops._p(ws), nbytes, B, HW, K, width, int(fixed), st)
                    assert rc == 0 and torch.equal(pk2, pk) and _same_bits(ps2, ps), ("masks = NULL", what)
                    second += int((ps != 0).sum())
                    n += 1
    assert second > 0
    return dict(runs=n, pixels_with_second_plane=second)


def check_producer_refusals(device):
    """The refusals of check_soft_refusals (which runs here unchanged, on the plain entry point) for the pair entry
    point, plus NULL pair_k and NULL pair_s; nothing is launched on a refusal."""
    sp.check_soft_refusals(device)
    lib, st, p = _lib.get(), _lib.stream(), ops._p
    pu8 = lambda t: _lib.ptr(t, True, dtype=torch.uint8)
    d = torch.full((2, 5, 7), 0.5, device=device)
    planes = torch.full((2, 17, 5, 7), -7.0, device=device)
    pk = torch.full((2, 5, 7), 99, dtype=torch.uint8, device=device)
    ps = torch.full((2, 5, 7), -7.0, device=device)
    nbytes = int(lib.dasr_depth_to_masks_soft_workspace(2, 35))
    ws = torch.zeros((nbytes // 4,), device=device)

    def rc(K=10, width=1.0, masks=planes, k=pk, s=ps, wsb=nbytes, depth=d):
        return lib.dasr_depth_to_masks_soft_pair(p(depth, True), p(masks, True), pu8(k), p(s, True), p(ws), wsb, 2, 35, K,
                                                 width, 0, st)

    for width in (0.0, -1.0, 1.5, float("nan")):
        assert rc(width=width) == sp.E_SHAPE, width
        assert sp._raises(ValueError, ops.depth_to_masks_soft, d, 10, width, pair=True)
        assert sp._raises(ValueError, prep.depth_to_soft_masks, d, 10, False, width, pair=True)
    assert rc(K=17) == sp.E_UNSUPPORTED and rc(K=0) == sp.E_SHAPE
    assert sp._raises(ValueError, ops.depth_to_masks_soft, d, 17, pair=True)
    assert sp._raises(TypeError, ops.depth_to_masks_soft, d.double(), 10, pair=True)
    assert rc(wsb=nbytes - 1) == sp.E_WORKSPACE
    assert rc(depth=None) == E_NULL and rc(k=None) == E_NULL and rc(s=None) == E_NULL
    assert bool((planes == -7.0).all()) and bool((pk == 99).all()) and bool((ps == -7.0).all())    # nothing was launched
    assert rc(masks=None) == 0 and bool((pk < 10).all()) and bool((ps != -7.0).all()) and bool((planes == -7.0).all())
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# the forward at op level
# ---------------------------------------------------------------------------------------------------------------------
def run_pair(device, inp, pk, ps, relu, use_res, dtype=F32, amax=False):
    """dasr_sean_fwd_pair[_bf16]: the poisoned-after-reading CPU copy of out (and, with ``amax``, the fused maximum)."""
    dev = lambda x: x.to(F32).to(device).contiguous()
    act = lambda x: x.to(F32).to(dtype).to(device).contiguous()
    for k in ("t", "gb2", "res"):
        assert torch.equal(inp[k].to(F32).to(dtype).to(F64), inp[k]), (k, dtype)
    scal = lambda a: torch.full((1,), a, dtype=F32, device=device)
    t = act(inp["t"])
    buf = ops.amax_buffer(t) if amax else None
    y = ops.sean_fwd_pair(t, dev(inp["mean"]), dev(inp["var"]), act(inp["gb2"]), pk.to(device).contiguous(),
                          ps.to(device).contiguous(), dev(inp["D"]), dev(inp["bg"]), dev(inp["bb"]), scal(inp["ag"]),
                          scal(inp["ab"]), act(inp["res"]) if use_res else None, relu, **({"amax": buf} if amax else {}))
    out = _take(y)
    return (out, ops.amax_value(buf)) if amax else out


def _decode(pk, ps, K):
    return prep.pair_planes(pk, ps, K).to(F64)


def _hashed_k(B, K, H, W):
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    return (((b * 37 + y * 131 + x * 71 + 5) * 2654435761 % 2 ** 32) // 128 % K).to(torch.uint8)


def _valid_sign(pk, ps, K):
    """Signs kept valid at the end planes: k = 0 has no lower neighbour, k = K - 1 no upper one (K = 1: no neighbour)."""
    ps = torch.where((pk == 0) & (ps < 0), -ps, ps)
    ps = torch.where((pk == K - 1) & (ps > 0), -ps, ps)
    ps = torch.where((pk == 0) & (pk == K - 1), torch.zeros_like(ps), ps)
    return torch.where(ps == 0, torch.zeros_like(ps), ps)                   # (+0.0 only)


def _int_pairs(B, K, H, W, gen):
    """pair_k hashed per pixel, pair_s from {0, +-0.25, +-0.5}; planted: a pair on each side of the tile corner (7,31) /
    (8,32), the last column, an image corner whose neighbour taps fall outside the image, and a 3 x 3 block of unclaimed
    pixels (byte K) whose centre sees the bias only."""
    pk = _hashed_k(B, K, H, W)
    ps = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5])[torch.randint(0, 5, (B, H, W), generator=gen)]
    for i, (y, x) in enumerate(((7, 31), (8, 32), (7, 32), (8, 31), (H // 2, W - 1), (0, 0), (H - 1, W - 1))):
        ps[:, y, x] = (0.25, -0.5, 0.5, -0.25)[i % 4]
    ps = _valid_sign(pk, ps, K)
    pk[:, 3:6, 10:13] = K
    ps[:, 3:6, 10:13] = 0.0
    return pk, ps


def _exact_eighths(ref):
    """Every term of beta1 is a multiple of 1/4 (weights in {1/4, 1/2, 3/4, 1}, integer D and bias), the alphas are in
    {0, 1/2, 1}: every partial sum of out, in any order, is a multiple of 1/8 far below 2^21 - a float32 number."""
    assert torch.equal(ref["T_b1"] * 8, (ref["T_b1"] * 8).round()) and float(ref["T_b1"].max()) < 2.0 ** 21
    assert float(ref["xh"].abs().max()) == 0.0 and sx._is32(ref["out"])
    assert torch.equal(ref["out"] * 8, (ref["out"] * 8).round())


# (C, K, storage types): (96, 10) second slice half dead; (32, 16) half of the slice dead, SEAN_MAXK; (128, 1) two slices
E_TABLE = ((64, 10, (F32, BF16)), (96, 10, (F32,)), (32, 16, (F32, BF16)), (128, 1, (F32,)))


def check_forward_exact(device):
    """Gate E.  int_inputs data (t == mean: out = a_b b1 + (1 - a_b) b2 (+ res), ReLU on and off) with pairs from
    _int_pairs at 2 x 9 x 33: out == reference(inp, pair_planes(pair))["out"] after one rounding to the storage type, for
    E_TABLE over the cycled E_COMBOS.  Then, per case: all pair_s == 0 equals the region-only gather forward with
    region = pair_k (both exact on this data); the centre of the unclaimed block is the bias-only value; and malformed
    input (k = 0 with s < 0, k = K - 1 with s > 0, k = K + 3) drops the offending term and nothing else, against planes
    written out by hand."""
    B, H, W = BASE
    n = 0
    stats = {"runs": 0, "malformed": 0}
    for ci, (C, K, dtypes) in enumerate(E_TABLE):
        gen = torch.Generator().manual_seed(9300 + ci)
        pk, ps = _int_pairs(B, K, H, W, gen)
        assert K == 1 or int((ps != 0).sum()) > B * H * W // 2
        mask = _decode(pk, ps, K)
        for dtype in dtypes:
            for _ in range(2):
                relu, use_res, ag, ab = sx.E_COMBOS[n % len(sx.E_COMBOS)]
                n += 1
                inp = sx.int_inputs(C, K, BASE, gen, ag, ab)
                ref = sx.reference(inp, mask, relu, use_res)
                _exact_eighths(ref)
                got = run_pair(device, inp, pk, ps, relu, use_res, dtype)
                bad = _nbad(got, sx._once(ref["out"], dtype))
                assert bad == 0, ("mismatching elements", C, K, str(dtype), (relu, use_res, ag, ab), bad)
                # the centre of the unclaimed 3 x 3 block: g1, b1 are the bare biases
                want = ab * inp["bb"] + (1 - ab) * inp["gb2"][:, 4, 11, C:] + (inp["res"][:, 4, 11] if use_res else 0.0)
                want = want.clamp_min(0.0) if relu else want
                assert _nbad(got[:, 4, 11], sx._once(want, dtype)) == 0, ("bias-only pixel", C, K)
                stats["runs"] += 1
        # all s == 0: one plane per pixel - the region-only gather forward reads the same bytes as region bytes
        relu, use_res, ag, ab = sx.E_COMBOS[n % len(sx.E_COMBOS)]
        inp = sx.int_inputs(C, K, BASE, gen, ag, ab)
        zero = torch.zeros_like(ps)
        hard = _decode(pk, zero, K)
        ref = sx.reference(inp, hard, relu, use_res)
        _exact_eighths(ref)
        got = run_pair(device, inp, pk, zero, relu, use_res)
        assert _nbad(got, sx._once(ref["out"], F32)) == 0, ("s == 0", C, K)
        gather = sx.run(device, inp, hard, "region_only", relu, use_res, bwd=False)["out"]
        assert torch.equal(got, gather), ("s == 0 against the region-only gather forward", C, K)
        # malformed input: the offending term is dropped, nothing else
        mk, ms = pk.clone(), ps.clone()
        hand = mask.clone()
        spots = (((1, 2), 0, -0.25), ((8, 32), K - 1, 0.25), ((7, 31), K + 3, 0.25), ((0, 0), K + 3, -0.5))
        for (y, x), k, s in spots:
            mk[:, y, x], ms[:, y, x] = k, s
            hand[:, :, y, x] = 0.0
            if k < K:
                hand[:, k, y, x] = 1.0 - abs(s)
        assert torch.equal(_decode(mk, ms, K), hand), "pair_planes: a malformed term must be absent, the other kept"
        ref = sx.reference(inp, hand, relu, use_res)
        _exact_eighths(ref)
        got = run_pair(device, inp, mk, ms, relu, use_res)
        assert _nbad(got, sx._once(ref["out"], F32)) == 0, ("malformed pairs", C, K)
        stats["malformed"] += 1
    return stats


def _producer_pairs(device, B, K, H, W, width, gen):
    d = torch.rand(B, H, W, generator=gen).to(device)
    planes, pk, ps = ops.depth_to_masks_soft(d, K, width, False, pair=True)
    return planes.cpu(), pk.cpu(), ps.cpu()


def pair_launch_plan(B, H, W, C, residual):
    """sean_fwd_pair_impl's launch arithmetic restated: (workgroups per slice, base, rem) - the first ``rem`` workgroups
    take base + 1 consecutive (sample, tile) pairs, the others base."""
    tiles = B * (-(-W // 32)) * (-(-H // 8))
    slices = -(-C // 64)
    nwg = max(1, min((512 if residual else 768) // slices, tiles))
    return nwg, tiles // nwg, tiles % nwg


# (C, K, (B, H, W), runs on the emulator)
U_CASES = ((64, 10, BASE, True), (128, 7, (1, 5, 40), True), (64, 16, BASE, False), (128, 7, (258, 3, 5), False))


def check_forward_bound(device):
    """Gate U.  _spread_inputs data, pairs from the real producer on random depth maps at width 1 and 0.125:
    |kernel - float64| <= n 2^-24 M per element of out, M = reference()'s M_out on the decoded planes and n = 20 + 16:
    18 products and the bias on the g1 path (the fused multiply-adds only remove roundings), one rounding for 1 - |s|, and
    the 16 that sean_exact_checks._bound_counts charges from g1 to out.  Counted from csrc/sean.hip, not tuned.
    (258, 3, 5) at C = 128 with a residual (MI355X only): one tile per sample, 258 tiles over 512 / 2 = 256 workgroups per
    slice, so workgroups 0 and 1 take two tiles each - two SAMPLES, with a different D - asserted from pair_launch_plan.
    Printed, not gated: the same figure for the general forward (ops.sean_fwd, mode "none") on the decoded planes, and how
    many elements of the two kernels' outputs differ in bits."""
    n_bound = 20 + 16
    worst = worst_gen = 0.0
    differ = total = runs = 0
    for ci, (C, K, shape, on_emu) in enumerate(U_CASES):
        if device == "cpu" and not on_emu:
            continue
        B, H, W = shape
        gen = torch.Generator().manual_seed(9400 + ci)
        for wi, width in enumerate((1.0, 0.125)):
            relu, use_res = (ci + wi) % 2 == 0, wi == 0 or B > 2
            if B > 2:
                nwg, base, rem = pair_launch_plan(B, H, W, C, use_res)
                assert (-(-W // 32)) * (-(-H // 8)) == 1 and base == 1 and rem >= 2, (nwg, base, rem)
                # workgroup 0 owns (sample, tile) pairs 0 and 1 = samples 0 and 1: D is restaged inside its loop
            planes, pk, ps = _producer_pairs(device, B, K, H, W, width, gen)
            mask = _decode(pk, ps, K)
            assert torch.equal(mask, planes.to(F64))
            inp = sx._spread_inputs(C, K, shape, gen)
            if B > 2:
                assert not torch.equal(inp["D"][0], inp["D"][1])
            ref = sx.reference(inp, mask, relu, use_res)
            bound = (n_bound * U * ref["M_out"]).clamp_min(1e-300)
            got = run_pair(device, inp, pk, ps, relu, use_res)
            ratio = float(((got.to(F64) - ref["out"]).abs() / bound).max())
            gen_out = sx.run(device, inp, mask, "none", relu, use_res, bwd=False)["out"]
            worst_gen = max(worst_gen, float(((gen_out.to(F64) - ref["out"]).abs() / bound).max()))
            worst = max(worst, ratio)
            differ += int((_bits(got) != _bits(gen_out)).sum())
            total += got.numel()
            runs += 1
            assert ratio <= 1.0, ("per-element bound", C, K, shape, width, "n", n_bound, "worst error / bound", ratio)
    print("pair forward  worst error / bound = %.4f   (general forward: %.4f)   elements that differ in bits from the "
          "general forward: %d of %d" % (worst, worst_gen, differ, total))
    return dict(runs=runs, worst=round(worst, 4), general=round(worst_gen, 4), differ=differ, of=total)


def check_forward_amax(device):
    """The fused maximum (fp32) is bit for bit max |out| of the tensor that came back, and out is that of the plain
    form.  C = 64, K = 16, 2 x 9 x 33 with all but K isolated pixels unclaimed: clamped lanes beyond the last column and
    row gather other rows than the pixels whose t they read, so a maximum over every lane exceeds max |out| here."""
    C, K = 64, 16
    B, H, W = BASE
    gen = torch.Generator().manual_seed(9500)
    r = sx.isolated_regions(B, K, H, W)
    pk = r.to(torch.uint8)
    ps = _valid_sign(pk, torch.where(r < K, torch.tensor(0.25), torch.tensor(0.0)) * (1 - 2 * (r % 2)).float(), K)
    assert int((pk == K).sum()) == B * (H * W - K) and int((ps != 0).sum()) > 0
    inp = sx._spread_inputs(C, K, BASE, gen)
    n = 0
    for relu, use_res in ((True, True), (False, False)):
        plain = run_pair(device, inp, pk, ps, relu, use_res)
        fused, amax = run_pair(device, inp, pk, ps, relu, use_res, amax=True)
        assert torch.equal(plain, fused), "fused-amax form differs"
        assert amax == float(fused.abs().max()), ("fused amax", amax, float(fused.abs().max()))
        n += 1
    return dict(runs=n)


def check_forward_refusals(device):
    """C % 4 != 0 and K > 16: DASR_E_UNSUPPORTED before any launch; NULL side-cars: DASR_E_NULL."""
    lib, st, p = _lib.get(), _lib.stream(), ops._p
    B, H, W = 1, 3, 5

    def rc(C=8, K=3, k=True, s=True):
        z = lambda *shape: torch.zeros(shape, device=device)
        out = torch.full((B, H, W, C), -7.0, device=device)
        pk = torch.zeros((B, H, W), dtype=torch.uint8, device=device)
        t, mean, var, gb2, ps, D, bias, alpha = (z(B, H, W, C), z(B, C), z(B, C) + 1, z(B, H, W, 2 * C), z(B, H, W),
                                                 z(B, 2, 9, K, C), z(C), z(1))
        code = lib.dasr_sean_fwd_pair(p(t), p(mean), p(var), p(gb2), _lib.ptr(pk, dtype=torch.uint8) if k else None,
                                      p(ps) if s else None, p(D), p(bias), p(bias), p(alpha), p(alpha), None, p(out), None,
                                      0, B, H, W, C, K, ops.IN_EPS, st)
        return code, bool((out == -7.0).all())          # (the read-back waits for the launch: the inputs are still alive)

    assert rc(C=6) == (E_UNSUPPORTED, True) and rc(K=17) == (E_UNSUPPORTED, True)
    assert rc(k=False) == (E_NULL, True) and rc(s=False) == (E_NULL, True)
    code, untouched = rc()
    assert code == 0 and not untouched
    return dict(ok=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. MaskPack.resized
# ---------------------------------------------------------------------------------------------------------------------
def check_resize(device):
    """A pair pack at 9 x 33 resized to 18 x 66 and 36 x 132, and one at 18 x 66 down to 9 x 33: the resized pair decodes
    to exactly ops.resize_nearest_nchw of the planes (the rule is pointwise), and the pack stays a pair pack."""
    K = 10
    gen = torch.Generator().manual_seed(9600)
    n = 0
    for (h, w), targets in (((9, 33), ((18, 66), (36, 132))), ((18, 66), ((9, 33),))):
        d = torch.rand(2, h, w, generator=gen).to(device)
        planes, pk, ps = ops.depth_to_masks_soft(d, K, 1.0, False, pair=True)
        with _counting(ops, "mask_compress") as c:
            pack = graph.MaskPack(planes, pair=(pk, ps))
            assert pack.region is None and pack.flag is None and pack.pair_k is pk and pack.pair_s is ps
            for H, W in targets:
                r = pack.resized(H, W)
                want = ops.resize_nearest_nchw(planes, H, W)
                assert r.region is None and r.flag is None and tuple(r.pair_k.shape) == tuple(r.pair_s.shape) == (2, H, W)
                assert _same_bits(r.planes, want) and _same_bits(prep.pair_planes(r.pair_k, r.pair_s, K), want), (h, w, H, W)
                assert pack.resized(H, W) is r
                n += 1
            assert c["mask_compress"] == 0
    return dict(runs=n)


# ---------------------------------------------------------------------------------------------------------------------
# 6. - 7. the whole net
# ---------------------------------------------------------------------------------------------------------------------
def _names(log, prefix):
    return [L.name for L in log.launches if L.name.startswith(prefix)]


def _audited(device, fn):
    """fn() under tests/stream_audit.audit on the MI355X (the emulator has one stream: fn() alone); (result, log)."""
    if device != "cuda":
        return fn(), None
    from tests.stream_audit import audit
    torch.cuda.synchronize()
    with audit() as log:
        out = fn()
    torch.cuda.synchronize()
    assert log.launches and log.unresolved == 0
    assert log.reports == [], "\n".join(log.reports)
    return out, log


def check_whole_net_forward(device):
    """The net of soft_prep_checks.check_whole_net_forward at K = 10 and 16, and an x8 net whose last two blocks are depth
    blocks (they run at 2x and 4x the mask size: the resized packs), on prep.depth_to_soft_masks(pair=True) masks against
    the float64-free CPU oracle at that check's gate, 2e-4.  Every SEAN forward is ops.sean_fwd_pair, no compression pass
    runs; on the MI355X the launch log says the same and the stream audit is clean.  Printed: the distance to the
    general-path forward (graph.FORCE_GENERAL_SEAN)."""
    out = {}
    for name, kw, K, (B, h, w) in (("K10", dict(which_ResBlk_depth=[0, 1], nb=4, scale=2), 10, (2, 8, 12)),
                                   ("K16", dict(which_ResBlk_depth=[0, 1], nb=4, scale=2), 16, (2, 8, 12)),
                                   ("x8_tail", dict(which_ResBlk_depth=[0, 2, 3], nb=4, scale=8), 10, (1, 4, 6))):
        cfg = O.make_cfg(depth_latent_ch=32, depthRangeNum=K, **kw)
        net = DepthNet(depth_latent_ch=32, depthRangeNum=K, **kw)
        synth.closed_form_fill_(net.state_dict().items())
        net = net.to(device)
        lq, _, dm, _ = synth.closed_form_batch(1, B, h, w, kw["scale"], K)
        lq_d, dm_d = lq.to(device), dm.to(device)
        mk = prep.depth_to_soft_masks(dm_d, K, width=1.0, pair=True)
        assert graph.attached_pair(mk) is not None and float((mk > 0).sum(dim=1).float().mean()) > 1.0
        n_depth = 2 * len([i for i in kw["which_ResBlk_depth"] if i != kw["nb"] - 3])

        def forward():
            with torch.no_grad():
                return net(lq_d, dm_d, mk)

        with _counting(ops, "sean_fwd_pair", "sean_fwd", "mask_compress") as c:
            sr, log = _audited(device, forward)
        assert (c["sean_fwd_pair"], c["sean_fwd"], c["mask_compress"]) == (n_depth, 0, 0), (name, c)
        if log is not None:
            fwd = _names(log, "dasr_sean_fwd")
            assert len(fwd) == n_depth and all(nm.startswith("dasr_sean_fwd_pair") for nm in fwd), fwd
            assert not _names(log, "dasr_mask_compress")
            if name == "x8_tail":
                assert _names(log, "dasr_resize_nearest_u8"), "the resized packs were not used"
        with torch.no_grad():
            ref = O.depthnet_forward(_oracle_sd(net), cfg, lq, dm, mk.cpu())
            graph.FORCE_GENERAL_SEAN = True
            try:
                with _counting(ops, "sean_fwd_pair") as c:
                    general = net(lq_d, dm_d, mk)
                assert c["sean_fwd_pair"] == 0
            finally:
                graph.FORCE_GENERAL_SEAN = False
        err = (sr.cpu() - ref).abs().max().item()
        out[name] = (err, (sr - general).abs().max().item())
        print("pair whole-net forward %s: max error against the oracle %.3g, distance to the general path %.3g" % ((name,) + out[name]))
        assert err <= 2e-4, (name, err)
    return out


TRAIN_CASE = dict(scale=2, which=[0, 1, 2, 3], L=16, nb=4, B=1, H=8, W=12)
N_SEAN = 6                         # blocks 0, 2 and 3 run (block nb - 3 is constructed but never called), two SEANs each


def check_training_step(device):
    """Training on prep.depth_to_soft_masks(pair=True) masks.  (a) forward and every parameter gradient against the CPU
    oracle with parity_checks._compare_with_oracle at its own gates (2e-4, 2e-5), the helper check_soft_masks_whole_net
    uses, unchanged: it is handed the planes on the CPU, for the oracle, whose ``.to(device)`` gives the stamped device
    tensor.  (b) one Trainer step: the SEAN forwards are the pair kernel, the backwards ops.sean_bwd on the planes with
    region = flag = None; on the MI355X the same from the launch log (dasr_sean_bwd* without a region argument) under a
    clean stream audit."""
    K = 10
    net, cfg = build_net(TRAIN_CASE, device)
    lq, gt, dm, _ = synth.closed_form_batch(2, 1, 8, 12, 2)
    mk_d = prep.depth_to_soft_masks(dm.to(device), K, width=1.0, pair=True)
    mk = mk_d.cpu()
    mk.to = lambda *a, **k: mk_d                       # (instance attribute: _compare_with_oracle's mk.to(device))
    with _counting(ops, "sean_fwd_pair", "sean_fwd") as c:
        err, rel = _compare_with_oracle(net, cfg, lq, dm, mk, device)
    assert c["sean_fwd_pair"] == N_SEAN and c["sean_fwd"] == 0, c
    print("pair training: forward max error %.3g, gradient relative L2 %.3g" % (err, rel))

    net, _ = build_net(TRAIN_CASE, device)
    tr = harness.Trainer(net)
    seen = []
    keep = ops.sean_bwd

    def bwd(*a, **k):
        seen.append((a[7], a[8]))                       # (region, flag)
        return keep(*a, **k)

    def step():
        masks = prep.depth_to_soft_masks(dm.to(device), K, width=1.0, pair=True)
        return tr.optimize_parameters(lq.to(device), gt.to(device), dm.to(device), masks)

    ops.sean_bwd = bwd
    try:
        with _counting(ops, "sean_fwd_pair", "sean_fwd", "mask_compress") as c:
            log_t, log = _audited(device, step)
    finally:
        ops.sean_bwd = keep
    assert (c["sean_fwd_pair"], c["sean_fwd"], c["mask_compress"]) == (N_SEAN, 0, 0), c
    assert len(seen) == N_SEAN and all(r is None and f is None for r, f in seen), seen
    assert all(math.isfinite(float(v)) for v in log_t.values()), log_t
    if log is not None:
        fwd, bw = _names(log, "dasr_sean_fwd"), [L for L in log.launches if L.name.startswith("dasr_sean_bwd")]
        assert len(fwd) == N_SEAN and all(nm.startswith("dasr_sean_fwd_pair") for nm in fwd), fwd
        assert len(bw) == N_SEAN and not any(a.name in ("region", "onehot_flag") for L in bw for a in L.args)
        assert not _names(log, "dasr_mask_compress")
    return dict(err=err, rel=rel, l_all=float(log_t["l_all"]))


def check_graphed_trainer_pair(device):
    """MI355X: a captured Trainer step on pair masks.  The captured forward reads the CAPTURED masks' side-cars, so a replay
    on another mask tensor must bring its pair along: five steps on five different depth maps give the losses of an eager
    trainer on the same batches (the gate of soft_loss_checks.check_graphed_trainer_soft, 3e-3), and the captured side-cars
    hold the last step's pair afterwards.  Masks without a pair are refused by a step captured with one."""
    K = 10
    frames, depths = sp._fixture_frames(2)
    flags = np.array([1, 2], dtype=np.uint8)
    case = dict(name="x4_nb4_dgb", scale=4, which=[0, 1], L=32, nb=4, B=2, H=12, W=12)
    from dasr_amd import data
    losses = {}
    for use_graph in (False, True):
        net, _ = build_net(case, device)
        tr = harness.Trainer(net, K, use_graph=use_graph)
        mk = data.BatchMaker(4, K, device=device)
        out = []
        for step in range(5):
            lq, gt, depth, _ = mk.make(np.roll(frames, step, axis=1), np.roll(depths, step, axis=2), flags)
            masks = prep.depth_to_soft_masks(depth, K, width=1.0, pair=True)
            out.append(float(tr.optimize_parameters(lq, gt, depth, masks)["l_all"]))
        losses[use_graph] = out
    assert tr._graph is not None
    pk, ps = graph.attached_pair(tr._static[3])
    want = graph.attached_pair(masks)
    assert torch.equal(pk, want[0]) and _same_bits(ps, want[1]) and pk is not want[0]
    le, lg = losses[False], losses[True]
    assert all(math.isfinite(v) for v in le + lg), (le, lg)
    assert all(abs(a - b) <= 3e-3 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    assert sp._raises(ValueError, tr.optimize_parameters, lq, gt, depth, prep.depth_to_soft_masks(depth, K, width=1.0))
    print("captured trainer on pair masks: losses eager", le, "captured", lg)
    return dict(eager=le, captured=lg)


# ---------------------------------------------------------------------------------------------------------------------
# 8. video (MI355X), the switches
# ---------------------------------------------------------------------------------------------------------------------
def check_switches(device):
    """soft_pair without soft_masks raises ValueError; soft_pair=False is the call without the keyword (the defaults check
    of soft_prep_checks.check_defaults_unchanged restated for the new argument)."""
    lin = torch.nn.Linear(1, 1)
    assert sp._raises(ValueError, FrameUpscaler, lin, soft_pair=True)
    assert sp._raises(ValueError, validate.validate_u8, lin, [], 4, soft_pair=True)
    assert sp._raises(ValueError, validate.test_u8, lin, [], 4, soft_pair=True)
    assert FrameUpscaler(lin, soft_masks=0.5, soft_pair=True).soft_pair is True
    case = sp.X4 if device == "cuda" else sp.TINY_X8
    net, _ = build_net(case, device)
    h, w, s = case["H"], case["W"], case["scale"]
    f, d = sp._frames(h, w, 1, 0)
    for soft in (None, 0.5):
        ups = [FrameUpscaler(net, use_graph=False, soft_masks=soft),
               FrameUpscaler(net, use_graph=False, soft_masks=soft, soft_pair=False)]
        with _counting(ops, "sean_fwd_pair") as c:
            a, b = (u.upscale(f, d) for u in ups)
        assert c["sean_fwd_pair"] == 0 and np.array_equal(a, b) and a.shape == (1, s * h, s * w, 3)
        slots = [next(iter(u._shapes.values())).slots[0] for u in ups]
        assert sorted(vars(slots[0])) == sorted(vars(slots[1])) and ups[0].soft_pair is False
    gt = torch.from_numpy(np.random.default_rng(5).random(size=(1, 3, s * h, s * w), dtype=np.float32))
    items = [(f, gt, d)]
    assert validate.validate_u8(net, items, s) == validate.validate_u8(net, items, s, soft_pair=False)
    assert validate.validate_u8(net, items, s, soft_masks=0.5) == validate.validate_u8(net, items, s, soft_masks=0.5, soft_pair=False)
    r0, r1 = validate.test_u8(net, items, s), validate.test_u8(net, items, s, soft_pair=False)
    assert r0 == r1 and r0["n"] == 1
    return dict(ok=True)


def check_upscaler_pair(device):
    """FrameUpscaler(soft_masks=1.0, soft_pair=True) on the frames of check_upscaler_soft, fp32, bf16 and the fp32
    self-ensemble: eager and captured give the same bytes, also after a re-capture forced by load_state_dict; against
    soft_pair=False every byte differs by at most 1 (the float outputs agree far below 1 / 255: only rounding boundaries
    can flip; the count is printed)."""
    out = {}
    seq = [sp._frames(12, 16, 2, 1)] + [sp._frames(12, 16, 2, 20 + i) for i in range(3)]
    for dtype, ens in (("fp32", False), ("bf16", False), ("fp32", True)):
        net, _ = build_net(sp.X4, device)
        net.set_compute_dtype(dtype)
        kw = dict(soft_masks=1.0, self_ensemble=ens)
        with _counting(ops, "sean_fwd_pair", "sean_fwd") as c:
            up_e = FrameUpscaler(net, use_graph=False, soft_pair=True, **kw)
            eager = [up_e.upscale(f, d) for f, d in seq]
        assert c["sean_fwd_pair"] > 0 and c["sean_fwd"] == 0, c
        up_g = FrameUpscaler(net, use_graph=True, soft_pair=True, **kw)
        for i, (f, d) in enumerate(seq):
            assert np.array_equal(up_g.upscale(f, d), eager[i]), (dtype, ens, i)
        assert up_g.captures == 1 and up_g.replays >= 2, (up_g.captures, up_g.replays)
        general = [FrameUpscaler(net, use_graph=False, **kw).upscale(f, d) for f, d in seq[:2]]
        diff = [np.abs(a.astype(np.int16) - b.astype(np.int16)) for a, b in zip(eager, general)]
        assert max(int(x.max()) for x in diff) <= 1, (dtype, ens, [int(x.max()) for x in diff])
        out["%s%s" % (dtype, "+ens" if ens else "")] = (sum(int((x != 0).sum()) for x in diff), sum(x.size for x in diff))
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        sd["conv_output.weight"] = sd["conv_output.weight"] * 1.5
        net.load_state_dict(sd)
        want = [FrameUpscaler(net, use_graph=False, soft_pair=True, **kw).upscale(f, d) for f, d in seq[:3]]
        for i in range(3):                                           # stale graph: two eager calls, then the re-capture
            assert np.array_equal(up_g.upscale(*seq[i]), want[i]), (dtype, ens, "after load_state_dict", i)
        assert up_g.captures == 2, up_g.captures
    print("soft_pair against the general path, bytes that differ (by 1) of all:", out)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 9. the stamp
# ---------------------------------------------------------------------------------------------------------------------
def check_stamp(device):
    """The pair stamp travels with the planes, is dropped by an in-place edit, and never reads as region bytes:
    attach_region answers False without a launch and graph.attached_region is None."""
    d = torch.tensor(sp.planted_maps((2, 5, 7), 10, False, 0), device=device)
    plain = prep.depth_to_soft_masks(d, 10, width=0.5)
    assert graph.attached_pair(plain) is None and prep.marked_soft(plain)
    for dd in (d, d[:, None]):
        m = prep.depth_to_soft_masks(dd, 10, width=0.5, pair=True)
        assert tuple(m.shape) == (2, 10, 5, 7) and _same_bits(m, plain) and prep.marked_soft(m) is True
        pk, ps = graph.attached_pair(m)
        assert pk.dtype == torch.uint8 and ps.dtype == F32 and tuple(pk.shape) == tuple(ps.shape) == (2, 5, 7)
        assert _same_bits(prep.pair_planes(pk, ps, 10), m)
        assert m._dasr_region is None and graph.attached_region(m) is None
    with _counting(ops, "mask_compress") as c:
        assert prep.attach_region(m) is False and c["mask_compress"] == 0
    assert graph.attached_region(m) is None and graph.attached_pair(m) is not None
    m.mul_(1.0)                                                 # an in-place edit drops both stamps
    assert graph.attached_pair(m) is None and prep.marked_soft(m) is False
    return dict(ok=True)
