"""The SEAN kernels of csrc/sean.hip at op level, every kernel form, behind dasr_sean_fwd / dasr_sean_bwd (and their _bf16
twins): the one-hot gather forward in three forms, the 8-wave one-hot backward that builds dD on the bf16 matrix cores, the
fp32-MFMA soft-mask forward and backward, the scalar fallback, the slab reduction and the two pass-B kernels.  Each check
takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_sean_exact.py runs every one of them on both.

The caller supplies mean and var, the alphas are inputs, (1 - alpha) x is an exact zero at alpha = 1 and the normalised
value is exactly 0 where t == mean: large parts of the result are exactly computable, the rest hangs on ONE rounding
through s(var) = dasr_double_in_scale.  Three kinds of gate (DESIGN.md 2 has the case table and the measured figures):
  E  integer data     D in [-2, 2], biases and mean in [-3, 3], gb2 / res / dout in [-4, 4], var in [0.01, 4], alphas in
                      {0, 0.5, 1}, t == mean: every gated sum has sum |term| < 2^22 in units of 1/4 (asserted from the
                      float64 terms), so fp32 is exact in ANY order - slabs, LDS and global atomics: == float64
  M  full mantissa    one term per sum: the scale probe (out == s(var) against a float32 numpy restatement, every operation
                      rounded on its own), the gamma image (out = fl32(+-2^j s (1 + g1)): one rounding), the backward on
                      `isolated` masks with 24-bit dout (every dD element is m a (dgam | g0) of ONE pixel, all 24 bits: a
                      two-piece split of G, a truncating sG store or an inexact residual fails here and passes every
                      rel_max gate), and pass B at H W = 2^n with t == mean (dt = fl32(s (dxh - S1 / N)): one rounding)
  U  derived bound    |kernel - float64| <= n 2^-24 M per ELEMENT on general data, M the float64 sum of the magnitudes of
                      the element's terms, n the roundings on the longest path (counted in _bound_counts, not tuned)
bf16 storage: the reference is float64 rounded to fp32 once and then to bf16 (the kernels compute in fp32 and round on
store); in the bf16 backward G = (a_g dgam, a_b g0) is rounded to bf16 ONCE by design before the matrix cores, so dD there
is m bf16(fl32(G)).

The dispatch of sean_fwd_impl / sean_bwd_impl, restated (fast = region bytes given and C % 4 == 0):
  fast, flag None      "region_only": k_sean_fwd_onehot (bf16: k_sean_fwd_onehot_w8 at C % 8 == 0, the 4-channel form under
                       ops.set_conv_bf16_impl(2048)) and k_sean_bwd_a_onehot<float, 1> / <bf16_t, 2> ALONE (fast_only); with
                       amax= / dgb2_amax= their AMAX = true instantiations
  fast, flag given     "compress": the one-hot AND the soft kernel are launched, the device flag lets one of them work
  no region, C % 4 == 0   "none": k_sean_fwd_soft / k_sean_bwd_a_soft (fp32 MFMA)
  C % 4 != 0           k_sean_fwd / k_sean_bwd_a (scalar, K <= 14), with or without region bytes
  dD                   slabs of sean_bwd_blocks_per_sample workgroups summed by k_sean_dD_reduce (scalar: float atomics)
  pass B               256 % (C / 4) == 0 (C = 32, 64, 128): k_sean_bwd_b_rows; else k_sean_bwd_b (float4 branch at C = 48,
                       96, scalar branch at C % 4 != 0); dt_amax= rides on either
Every form is forced by arguments (modes_of), never assumed.  Every result is read back and then poisoned (_take);
references are float64 torch / float32 numpy, never another entry point of the library.  A case whose last field is False runs on
the MI355X only."""
import numpy as np
import torch
import torch.nn.functional as F

from dasr_amd import ops
from tests.bf16_exact_checks import _ints, _nbad, _take
from tests.onehot_sean_checks import make_regions, planes_of
from tests.soft_mask_checks import make_inputs as gaussian_inputs

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS = float(np.float32(ops.IN_EPS))          # the kernels take eps as a float argument: this value, exactly
U = 2.0 ** -24
BASE = (2, 9, 33)          # one row past an 8-row tile, one column past a 32-column tile; 18 one-row backward tiles
POW2 = (2, 4, 64)          # H W = 256: S1 / N is exact (check_mantissa_pass_b)
ONEHOT_KINDS = ("blob", "hashed", "hole", "allnone", "uniform")
GRADS = ("dt", "dgb2", "dD", "dbg", "dbb", "dag", "dab", "dres")


def modes_of(C):
    """How each kernel form is reached (the module docstring has the dispatch): "region_only" the gather kernels alone,
    "compress" through the device flag, "none" the soft MFMA kernels; C % 4 != 0: the scalar kernels either way."""
    return ("region_only", "compress", "none") if C % 4 == 0 else ("compress", "none")


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------
def isolated_pixels(H, W, K):
    """K distinct pixels: an image corner, two tile corners (y = 7 | 8, x = 31 | 32, clipped into the image), the last
    column, the other corners, then a stride through the image."""
    want = [(0, 0), (7, 31), (8, 32), (H // 2, W - 1), (H - 1, W - 1), (7, 32), (8, 31), (0, W - 1), (H - 1, 0)]
    pix = []
    for y, x in want + [divmod((i * 37 + 11) % (H * W), W) for i in range(H * W)]:
        p = (min(y, H - 1), min(x, W - 1))
        if p not in pix:
            pix.append(p)
    assert len(pix) >= K, ("isolated: more regions than pixels", H, W, K)
    return pix[:K]


def isolated_regions(B, K, H, W):
    """Region integers with every region claimed by exactly ONE pixel per sample, all other pixels unclaimed (K)."""
    r = torch.full((B, H, W), K, dtype=torch.long)
    pix = isolated_pixels(H, W, K)
    for b in range(B):
        for k in range(K):
            y, x = pix[(k + 3 * b) % K]
            r[b, y, x] = k
    assert all(int((r[b] == k).sum()) == 1 for b in range(B) for k in range(K))
    return r


def regions(kind, B, K, H, W):
    return isolated_regions(B, K, H, W) if kind == "isolated" else make_regions(kind, B, K, H, W)


def interior_counts(r, K):
    """(pixel groups that take the interior-table shortcut of sean_gather_interior, groups that do not), from the region
    integers: a wave step holds four consecutive pixels x = 4 i .. 4 i + 3 of a row, and the shortcut is a vote of all of
    them: every one inside the image with nine equal neighbourhood bytes below K (K outside the image)."""
    B, H, W = r.shape
    rp = F.pad(r, (1, 1, 1, 1), value=K)
    same = torch.ones((B, H, W), dtype=torch.bool)
    for tap in range(9):
        same &= rp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W] == r
    same &= r < K
    same = F.pad(same.to(torch.uint8), (0, (-W) % 4)).reshape(B, H, -1, 4).min(-1).values > 0
    return int(same.sum()), int((~same).sum())


def onehot_mask(kind, B, K, H, W, device):
    """float64 planes [B, K, H, W] of a one-hot kind and its region integers; ops.mask_compress must return exactly them
    with a clear flag."""
    r = regions(kind, B, K, H, W)
    planes = planes_of(r, K)
    region, flag = ops.mask_compress(planes.to(device))
    assert int(flag.item()) == 0 and torch.equal(region.cpu().long(), r), ("mask_compress", kind, K)
    return planes.to(F64), r


def soft_mask(kind, B, K, H, W, gen):
    """float64 soft planes: "softint" small integers in [-2, 2] (a fifth exact zeros); "isolated" the isolated pixels with
    the values 0.5 and -2, zero elsewhere; "real" 0.7 one-hot + 0.3 uniform noise with exact zeros (gate U)."""
    if kind == "softint":
        m = _ints(gen, -2, 2, B, K, H, W)
        assert bool((m == 0).any()) or m.numel() < 8
        return m
    if kind == "isolated":
        r = isolated_regions(B, K, H, W)
        val = torch.where((torch.arange(K) % 2 == 0), torch.tensor(0.5), torch.tensor(-2.0)).view(1, K, 1, 1)
        return (planes_of(r, K) * val).to(F64)
    assert kind == "real"
    m = 0.7 * planes_of(regions("hashed", B, K, H, W), K) + 0.3 * torch.rand(B, K, H, W, generator=gen)
    m[torch.rand(B, K, H, W, generator=gen) < 0.2] = 0.0
    return m.to(F32).to(F64)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def scale32(var32):
    """dasr_double_in_scale in float32 numpy, every operation rounded on its own (correctly rounded sqrt and division)."""
    var32 = np.asarray(var32, dtype=np.float32)
    e, one = np.float32(EPS), np.float32(1.0)
    a = var32 + e
    r1 = one / np.sqrt(a)
    v2 = var32 / a
    s = r1 / np.sqrt(v2 + e)
    assert s.dtype == np.float32
    return s


def scale64(var):
    a = var + EPS
    return 1.0 / a.sqrt() / (var / a + EPS).sqrt()


def dscale64(var):
    a = var + EPS
    b = var / a + EPS
    return scale64(var) * (-0.5 / a - 0.5 * (EPS / (a * a)) / b)


def dynconv64(mask, D):
    """gamma1, beta1 without bias, NHWC [B, H, W, C]: F.conv2d of the planes with D[b] as [2C, K, 3, 3]."""
    B, K, H, W = mask.shape
    C = D.shape[-1]
    out = []
    for b in range(B):
        w = D[b].reshape(2, 3, 3, K, C).permute(0, 4, 3, 1, 2).reshape(2 * C, K, 3, 3)
        out.append(F.conv2d(mask[b:b + 1], w, padding=1))
    gb1 = torch.cat(out, 0).permute(0, 2, 3, 1)
    return gb1[..., :C], gb1[..., C:]


def dD64(mask, G, Bv):
    """dD[b, s, tap, k, c] = sum_p mask[b, k, p + tap - 1] (G | Bv)[b, p, c], and the number of non-zero terms of each."""
    B, K, H, W = mask.shape
    mp = F.pad(mask, (1, 1, 1, 1))
    dD = torch.zeros(B, 2, 9, K, G.shape[-1], dtype=mask.dtype)
    terms = torch.zeros(B, 9, K, dtype=torch.long)
    for tap in range(9):
        win = mp[:, :, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W]
        dD[:, 0, tap] = torch.einsum("bkhw,bhwc->bkc", win, G)
        dD[:, 1, tap] = torch.einsum("bkhw,bhwc->bkc", win, Bv)
        terms[:, tap] = (win != 0).sum((2, 3))
    return dD, terms


def reference(inp, mask, relu, use_res, s=None, out_in=None):
    """Everything the kernels compute, in the dtype of ``inp`` (float64; float32 for the torch restatement of gate U), from
    the formulas of csrc/sean.hip; mean, var and the alphas are inputs.  ``s``: the scale to use instead of the float64
    s(var) (gate M: the float32 restatement, as float64).  ``out_in``: the `out` the backward is given (default: this
    function's own, rounded to float32).  With float64 inputs the magnitudes ("M_*": the same sums over absolute values)
    come back as well."""
    t, gb2, D = inp["t"], inp["gb2"], inp["D"]
    B, H, W, C = t.shape
    N = H * W
    ag, ab = inp["ag"], inp["ab"]
    v = lambda x: x.reshape(B, 1, 1, C)
    s = v(scale64(inp["var"]) if s is None else s)
    ds = v(dscale64(inp["var"]))
    g1, b1 = dynconv64(mask, D)
    g1, b1 = g1 + inp["bg"], b1 + inp["bb"]
    g2, b2 = gb2[..., :C], gb2[..., C:]
    gam, bet = ag * g1 + (1 - ag) * g2, ab * b1 + (1 - ab) * b2
    xc = t - v(inp["mean"])
    xh = xc * s
    pre = xh * (1 + gam) + bet + (inp["res"] if use_res else 0.0)
    out = pre.clamp_min(0.0) if relu else pre
    r = {"out": out, "pre": pre, "s": s, "xh": xh}
    o_in = out.to(F32) if out_in is None else out_in
    g0 = torch.where(o_in > 0, inp["dout"], torch.zeros_like(inp["dout"])) if relu else inp["dout"]
    dgam = g0 * xh
    G, Bv = ag * dgam, ab * g0
    dxh = g0 * (1 + gam)
    S1, S2 = dxh.sum((1, 2), keepdim=True), (dxh * xc).sum((1, 2), keepdim=True)
    dD, terms = dD64(mask, G, Bv)
    r.update(g0=g0, dgam=dgam, dres=g0, dgb2=torch.cat(((1 - ag) * dgam, (1 - ab) * g0), -1), dD=dD, dD_terms=terms,
             dbg=G.sum((0, 1, 2)), dbb=Bv.sum((0, 1, 2)), dag=(dgam * (g1 - g2)).sum().reshape(1),
             dab=(g0 * (b1 - b2)).sum().reshape(1), dt=s * (dxh - S1 / N) + ds * (2.0 / N) * xc * S2)
    if t.dtype != F64:
        return r
    # magnitudes: the same sums over absolute values
    A = torch.abs
    mg1, mb1 = dynconv64(A(mask), A(D))
    mg1, mb1 = mg1 + A(inp["bg"]), mb1 + A(inp["bb"])
    mgam, mbet = abs(ag) * mg1 + abs(1 - ag) * A(g2), abs(ab) * mb1 + abs(1 - ab) * A(b2)
    mdxh = A(g0) * (1 + mgam)
    mS1, mS2 = mdxh.sum((1, 2), keepdim=True), (mdxh * A(xc)).sum((1, 2), keepdim=True)
    mdD, _ = dD64(A(mask), A(G), A(Bv))
    r.update(M_out=A(xh) * (1 + mgam) + mbet + (A(inp["res"]) if use_res else 0.0),
             M_dgb2=torch.cat((abs(1 - ag) * A(dgam), abs(1 - ab) * A(g0)), -1), M_dD=mdD,
             M_dbg=A(G).sum((0, 1, 2)), M_dbb=A(Bv).sum((0, 1, 2)), M_dag=(A(dgam) * (mg1 + A(g2))).sum().reshape(1),
             M_dab=(A(g0) * (mb1 + A(b2))).sum().reshape(1),
             M_dt=A(s) * (mdxh + mS1 / N) + A(ds) * (2.0 / N) * A(xc) * mS2,
             T_dab=A(g0 * (b1 - b2)), T_dD=mdD, T_b1=mb1)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def run(device, inp, mask, mode, relu, use_res, dtype=F32, out_in=None, amax=False, bwd=True):
    """dasr_sean_fwd and dasr_sean_bwd in one dispatch mode; poisoned-after-reading CPU copies {"out", GRADS...} (and, with
    ``amax``, the three fused maxima as floats).  The backward's `out` is the forward's own result, or ``out_in``."""
    dev = lambda x: x.to(F32).to(device).contiguous()
    act = lambda x: x.to(F32).to(dtype).to(device).contiguous()
    for k in ("t", "gb2", "res", "dout"):                      # activations must be numbers of their storage type
        assert torch.equal(inp[k].to(F32).to(dtype).to(F64), inp[k]), (k, dtype)
    m = dev(mask)
    region = flag = None
    if mode != "none":
        region, flag = ops.mask_compress(m)
        if mode == "region_only":
            assert int(flag.item()) == 0, "region_only vouches for one-hot masks"
            flag = None
    scal = lambda a: torch.full((1,), a, dtype=F32, device=device)
    common = (m, region, flag, dev(inp["D"]), dev(inp["bg"]), dev(inp["bb"]), scal(inp["ag"]), scal(inp["ab"]))
    t, gb2, mean, var = act(inp["t"]), act(inp["gb2"]), dev(inp["mean"]), dev(inp["var"])
    am = [ops.amax_buffer(t) for _ in range(3)] if amax else [None] * 3
    kw = {"amax": am[0]} if amax else {}
    y = ops.sean_fwd(t, mean, var, gb2, *common, act(inp["res"]) if use_res else None, relu, **kw)
    got = {}
    if bwd:
        kw = {"dt_amax": am[1], "dgb2_amax": am[2]} if amax else {}
        g = ops.sean_bwd(act(inp["dout"]), y if out_in is None else act(out_in), t, mean, var, gb2, *common, relu, True, **kw)
        got = {nm: _take(x) for nm, x in zip(GRADS, g)}
    got["out"] = _take(y)
    if amax:
        got["amax"] = tuple(ops.amax_value(a) for a in (am[:1] if not bwd else am))
    return got


def _amax_ok(got, what):
    """The fused maxima are bit for bit max |tensor| of the tensors that came back with them."""
    names = ("out", "dt", "dgb2")[:len(got["amax"])]
    want = tuple(float(got[nm].abs().max()) for nm in names)
    assert got["amax"] == want, ("fused amax", what, got["amax"], want)


def _once(x64, dtype):
    """float64 -> float32 (one rounding) -> the storage type (bf16: the kernels' second rounding, on store)."""
    return x64.to(F32).to(dtype).to(F64)


def _is32(x64):
    return torch.equal(x64.to(F32).to(F64), x64)


# ---------------------------------------------------------------------------------------------------------------------
# E. integer data
# ---------------------------------------------------------------------------------------------------------------------
def int_inputs(C, K, shape, gen, ag, ab, dout_hi=4):
    B, H, W = shape
    mean = _ints(gen, -3, 3, B, C)
    return dict(t=mean.reshape(B, 1, 1, C).expand(B, H, W, C).clone(), mean=mean,
                var=(torch.rand(B, C, generator=gen) * 3.99 + 0.01).to(F64), gb2=_ints(gen, -4, 4, B, H, W, 2 * C),
                res=_ints(gen, -4, 4, B, H, W, C), D=_ints(gen, -2, 2, B, 2, 9, K, C), bg=_ints(gen, -3, 3, C),
                bb=_ints(gen, -3, 3, C), ag=ag, ab=ab, dout=_ints(gen, -dout_hi, dout_hi, B, H, W, C))


def _exact_ok(ref):
    """Every exactly gated sum is a sum of multiples of 1/4 with sum |term| < 2^22: every partial sum, in any order, is a
    multiple of 1/4 below 2^22, a float32 number.  T_b1: beta1's own 9 K terms and its bias; T_dab: the terms g0 (b1 - b2)
    of dalpha_b, one sum over everything; T_dD: dD's sums of |m a g0| (dbias_b is a part of one of them at m = 1)."""
    for nm in ("T_dab", "T_dD", "T_b1"):
        assert torch.equal(ref[nm] * 4, (ref[nm] * 4).round()), nm
    assert float(ref["T_b1"].max()) < 2.0 ** 22
    return (float(ref["T_dab"].sum()) < 2.0 ** 22 and float(ref["T_dD"].max()) < 2.0 ** 22 and
            float(ref["M_dbb"].max()) < 2.0 ** 22)


# (relu, residual, alpha_g, alpha_b): the alphas only from {0, 0.5, 1}; cycled over the runs of a check
E_COMBOS = ((True, True, 1.0, 0.5), (False, False, 0.5, 0.0), (True, False, 0.0, 1.0), (False, True, 0.5, 0.5),
            (True, True, 0.0, 0.0), (False, False, 1.0, 1.0), (True, False, 0.5, 1.0), (False, True, 1.0, 0.5))
# (C, K, (B, H, W), one-hot kinds, soft kinds, runs on the emulator)
#   (64, 10)  the production shape, every kind          (64, 16)  SEAN_MAXK: byte 16 matches no row
#   (64, 1)   one region                                (32, 16)  half of the 64-channel slice dead
#   (96, 10)  second slice half dead, k_sean_bwd_b      (48, 10)  k_sean_bwd_b with one slice
#   (128, 7) at 1 x 5 x 40   two slices, fewer rows than a tile       (6, 3)  the scalar kernels
#   3 x 2 x 3, 1 x 1 x 1     smaller than a tile and than its halo     1 x 17 x 70  three ragged tile rows and columns
#   (32, 10) at 64 x 5 x 33  sean_bwd_blocks_per_sample = 256 / 64 = 4 workgroups per sample: the one-hot backward deals its
#                            10 one-row tiles 3, 3, 2, 2; the soft backward has 2 tiles, so two workgroups write zero slabs
E_CASES = (
    (64, 10, BASE, ONEHOT_KINDS + ("isolated",), ("softint", "isolated"), True),
    (64, 16, BASE, ("hashed", "hole"), ("softint",), True),
    (64, 1, BASE, ("hashed", "allnone"), ("softint",), True),
    (32, 16, BASE, ("hashed", "hole"), ("softint",), True),
    (96, 10, BASE, ("hashed", "uniform"), ("softint",), True),
    (48, 10, BASE, ("hashed",), ("softint",), True),
    (128, 7, (1, 5, 40), ("hashed", "hole", "isolated"), ("softint",), True),
    (6, 3, BASE, ("hashed", "hole", "isolated"), ("softint", "isolated"), True),
    (64, 10, (3, 2, 3), ("hashed",), ("softint",), True),
    (64, 10, (1, 1, 1), ("hashed", "uniform"), ("softint",), True),
    (64, 10, (1, 17, 70), ("hashed", "hole", "isolated"), ("softint",), True),
    (32, 10, (64, 5, 33), ("blob", "isolated"), ("softint",), False),         # (emulator: 10 s a run)
)


def _plan(C, onehot_kinds, soft_kinds):
    """(mask kind, is soft, mode) of a case: every one-hot kind in every mode that takes region bytes, the first one also
    through the soft kernels ("none"); every soft kind through "none", the first one also through the device flag."""
    plan = []
    for i, kind in enumerate(onehot_kinds):
        plan += [(kind, False, mode) for mode in modes_of(C) if mode != "none" or i == 0]
    for i, kind in enumerate(soft_kinds):
        plan += [(kind, True, "none")] + ([(kind, True, "compress")] if i == 0 else [])
    return plan


def _masks(device, K, shape, onehot_kinds, soft_kinds, gen):
    B, H, W = shape
    masks = {(k, False): onehot_mask(k, B, K, H, W, device)[0] for k in onehot_kinds}
    masks.update({(k, True): soft_mask(k, B, K, H, W, gen) for k in soft_kinds})
    return masks


def _int_run(device, C, K, shape, mask, mode, combo, gen, dtype, stats):
    relu, use_res, ag, ab = combo
    inp = int_inputs(C, K, shape, gen, ag, ab)
    ref = reference(inp, mask, relu, use_res)
    if not _exact_ok(ref):                                   # dalpha_b would leave the exact range: dout in {-1, 0, 1}
        inp = int_inputs(C, K, shape, gen, ag, ab, dout_hi=1)
        ref = reference(inp, mask, relu, use_res)
        stats["dout shrunk"] += 1
    assert _exact_ok(ref), ("sum |term| >= 2^22", C, K, shape)
    assert float(ref["xh"].abs().max()) == 0.0 and _is32(ref["out"])
    if relu:
        stats["relu'(0)"] += int(((ref["pre"] == 0) & (inp["dout"] != 0)).sum())
    got = run(device, inp, mask, mode, relu, use_res, dtype)
    zero = torch.zeros(())
    want = {"out": _once(ref["out"], dtype), "dres": ref["dres"], "dgb2": _once(ref["dgb2"], dtype), "dD": ref["dD"],
            "dbg": zero, "dbb": ref["dbb"], "dag": zero, "dab": ref["dab"]}
    assert float(ref["dD"][:, 0].abs().max()) == 0.0 and float(ref["dgb2"][..., :C].abs().max()) == 0.0
    bad = {nm: _nbad(got[nm], w.expand_as(got[nm])) for nm, w in want.items()}
    assert not any(bad.values()), ("mismatching elements", C, K, shape, mode, combo, str(dtype), bad)
    stats["runs"] += 1
    if mode == "region_only" and dtype == F32 and stats["runs"] % 3 == 1:      # the AMAX = true instantiations
        got = run(device, inp, mask, mode, relu, use_res, amax=True)
        bad = {nm: _nbad(got[nm], w.expand_as(got[nm])) for nm, w in want.items()}
        assert not any(bad.values()), ("fused-amax form, mismatching elements", C, K, shape, combo, bad)
        _amax_ok(got, (C, K, shape, combo))
        stats["fused-amax runs"] += 1


def _int_cases(device, cases, seed, dtype=F32, soft=True):
    stats = {"runs": 0, "fused-amax runs": 0, "relu'(0)": 0, "dout shrunk": 0, "interior groups": 0, "gather groups": 0}
    n = 0
    for ci, (C, K, shape, oh, sf, on_emu) in enumerate(cases):
        if device == "cpu" and not on_emu:
            continue
        gen = torch.Generator().manual_seed(seed + ci)
        masks = _masks(device, K, shape, oh, sf if soft else (), gen)
        for kind in oh:
            a, b = interior_counts(regions(kind, *shape[:1], K, *shape[1:]), K)
            stats["interior groups"], stats["gather groups"] = stats["interior groups"] + a, stats["gather groups"] + b
        for kind, is_soft, mode in _plan(C, oh, sf if soft else ()):
            if not soft and mode == "none":
                continue
            _int_run(device, C, K, shape, masks[(kind, is_soft)], mode, E_COMBOS[n % len(E_COMBOS)], gen, dtype, stats)
            n += 1
    assert stats["relu'(0)"] > 0, "input condition: no output that is exactly 0 meets a non-zero dout"
    assert stats["interior groups"] > 0 and stats["gather groups"] > 0, stats
    return stats


def check_int_fp32(device):
    """E on fp32 tensors, E_CASES, every mask kind in every dispatch mode of modes_of(C) (_plan): with t == mean broadcast,
    out = a_b b1 + (1 - a_b) b2 (+ res) (ReLU on and off): all 9 K taps, the zero padding, the halo, the unclaimed row K and
    the bias fold at every pixel and channel.  Backward on the same inputs: dres, the beta half of dgb2, dbias_b, dalpha_b
    (one sum over everything, through the interior table's beta rows and float atomics), the beta half of dD == float64,
    and dalpha_g, dbias_g, the gamma halves of dgb2 and dD == 0.  The ReLU backward must take relu'(0) = 0: outputs that are
    exactly 0 under a non-zero dout are counted and asserted to exist, as are wave steps that take the interior-table
    shortcut and steps that do not (from the region integers)."""
    return _int_cases(device, E_CASES, 9100)


# the bf16 forms take one-hot masks with region bytes: k_sean_fwd_onehot_w8 (C % 8 == 0), the 4-channel form, and
# k_sean_bwd_a_onehot<bf16_t, 2> (two tile rows: 9 rows = 5 tiles, the last one half)
E_CASES_BF16 = (
    (64, 10, BASE, ONEHOT_KINDS + ("isolated",), (), True),
    (96, 10, BASE, ("hashed", "uniform"), (), True),
    (32, 16, (1, 17, 70), ("hashed", "hole"), (), True),
)


def _both_bf16_forms(fn):
    """fn() with eight channels per lane (the default) and again with four (ops.set_conv_bf16_impl(2048))."""
    out = [fn()]
    ops.set_conv_bf16_impl(2048)
    try:
        out.append(fn())
    finally:
        ops.set_conv_bf16_impl(0)
    return out


def check_int_bf16(device):
    """E on bf16 tensors (E_CASES_BF16, both forward lane layouts): the gates of check_int_fp32, the reference rounded once
    to fp32 and then to bf16 (every value is a small multiple of 1/2: both roundings are exact, so is G in bf16)."""
    return _both_bf16_forms(lambda: _int_cases(device, E_CASES_BF16, 9200, BF16, soft=False))


# ---------------------------------------------------------------------------------------------------------------------
# M. full mantissa, one term per sum
# ---------------------------------------------------------------------------------------------------------------------
PROBE_VARS = (0.0, 1e-12, 1e-5, 1.0, 4.0, 1e6)


def _ulps(a32, b32):
    """Distance in float32 units in the last place between two float32 tensors of equal sign."""
    ia, ib = a32.contiguous().view(torch.int32).long(), b32.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


def probe_inputs(C, K, shape, gen):
    """t = mean + 1, D = 0, biases 0, a_g = a_b = 1, gb2 finite: out is exactly s(var)."""
    B, H, W = shape
    inp = int_inputs(C, K, shape, gen, 1.0, 1.0)
    var = torch.rand(B, C, generator=gen) * 3.99 + 0.01
    var.view(-1)[:B * C // 2 * 2:2] = torch.tensor(PROBE_VARS, dtype=F32).repeat(B * C)[:B * C // 2]
    inp.update(t=inp["t"] + 1.0, var=var.to(F64), D=torch.zeros_like(inp["D"]), bg=torch.zeros(C, dtype=F64),
               bb=torch.zeros(C, dtype=F64))
    return inp


M_FORMS = ((64, 10, BASE), (96, 10, BASE), (128, 7, (1, 5, 40)), (6, 3, BASE))


def check_scale_probe(device):
    """out == s(var) bit for bit against scale32 (float32 numpy, each operation rounded on its own) in every forward form:
    var holds 0, 1e-12, 1e-5, 1, 4 and 1e6 beside random values in [0.01, 4].  Holds on the MI355X because hipcc's default
    division and sqrtf are correctly rounded; every s-dependent gate M below rests on it.  bf16: the rounding of it."""
    worst = 0
    for ci, (C, K, shape) in enumerate(M_FORMS):
        gen = torch.Generator().manual_seed(9300 + ci)
        inp = probe_inputs(C, K, shape, gen)
        assert all(bool((inp["var"].to(F32) == torch.tensor(v, dtype=F32)).any()) for v in PROBE_VARS)
        s = torch.from_numpy(scale32(inp["var"].to(F32).numpy())).reshape(shape[0], 1, 1, C).expand(*shape, C)
        mask = onehot_mask("hashed", shape[0], K, *shape[1:], device)[0]
        for mode in modes_of(C):
            got = run(device, inp, mask, mode, False, False, bwd=False)["out"]
            d = _ulps(got, s.contiguous())
            print("scale probe C=%d K=%d %s %s: %d ulp" % (C, K, shape, mode, d))
            worst = max(worst, d)
            assert torch.equal(got, s), ("s(var) is not the float32 restatement", C, K, mode, "ulps", d)
        if C % 8 == 0:
            for got in _both_bf16_forms(lambda: run(device, inp, mask, "region_only", False, False, BF16, bwd=False)["out"]):
                assert torch.equal(got, s.to(BF16)), ("bf16 s(var)", C, K)
    return {"worst ulp distance": worst}


def mantissa_inputs(C, K, shape, gen, ag, ab, dtype=F32):
    """Integer D, biases, mean, gb2 (beta half 0 where a_b != 1 is wanted exact: see the callers); t = mean +- 2^j, j in
    -3 .. 3; var random float32 in [0.01, 4]; dout = +-(rand + 0.5), 24 bits (bf16: 8)."""
    B, H, W = shape
    inp = int_inputs(C, K, shape, gen, ag, ab)
    j = torch.randint(-3, 4, (B, H, W, C), generator=gen).to(F64)
    sign = torch.randint(0, 2, (B, H, W, C), generator=gen).to(F64) * 2 - 1
    dout = ((torch.rand(B, H, W, C, generator=gen) + 0.5) * (torch.randint(0, 2, (B, H, W, C), generator=gen) * 2 - 1))
    inp.update(t=inp["t"] + sign * 2.0 ** j, var=(torch.rand(B, C, generator=gen) * 3.99 + 0.01).to(F32).to(F64),
               dout=dout.to(F32).to(dtype).to(F64))
    return inp


def _s32(inp):
    return torch.from_numpy(scale32(inp["var"].to(F32).numpy())).to(F64)


M_GAMMA_CASES = (
    (64, 10, BASE, ONEHOT_KINDS, ("softint",), True),
    (64, 16, BASE, ("hashed",), ("softint",), True),
    (96, 10, BASE, ("hashed", "uniform"), ("softint",), True),
    (128, 7, (1, 5, 40), ("hashed",), ("softint",), True),
    (6, 3, BASE, ("hashed",), ("softint",), True),
    (64, 10, (1, 17, 70), ("hole",), ("softint",), True),
)


def _gamma_cases(device, cases, seed, dtype=F32, soft=True):
    n = 0
    for ci, (C, K, shape, oh, sf, on_emu) in enumerate(cases):
        if device == "cpu" and not on_emu:
            continue
        gen = torch.Generator().manual_seed(seed + ci)
        masks = _masks(device, K, shape, oh, sf if soft else (), gen)
        for kind, is_soft, mode in _plan(C, oh, sf if soft else ()):
            if not soft and mode == "none":
                continue
            inp = mantissa_inputs(C, K, shape, gen, 1.0, 0.0, dtype)
            inp["gb2"][..., C:] = 0.0
            relu = n % 2 == 0
            ref = reference(inp, masks[(kind, is_soft)], relu, False, s=_s32(inp))
            # xh = +-2^j s32 and 1 + g1 (an integer) are exact, their product is exact in float64: ONE rounding to float32
            assert _is32(ref["xh"]) and int((ref["out"] != 0).sum()) > ref["out"].numel() // 4
            got = run(device, inp, masks[(kind, is_soft)], mode, relu, False, dtype, bwd=False)["out"]
            bad = _nbad(got, _once(ref["out"], dtype))
            assert bad == 0, ("gamma image mismatching elements", C, K, shape, kind, mode, str(dtype), bad)
            if mode == "region_only" and dtype == F32:                       # k_sean_fwd_onehot<..., AMAX = true>
                fused = run(device, inp, masks[(kind, is_soft)], mode, relu, False, amax=True, bwd=False)
                assert torch.equal(fused["out"], got), ("fused-amax forward differs", C, K, shape, kind)
                _amax_ok(fused, (C, K, shape, kind))
            n += 1
    return {"runs": n}


def check_mantissa_gamma_image(device):
    """M forward, M_GAMMA_CASES in every dispatch mode: t - mean = +-2^j, a_g = 1, a_b = 0, the beta half of gb2 zero: out =
    fl32(xh (1 + g1)) with xh = +-2^j s32 exact and g1 an integer - the full 24 bits of s through the gather / MFMA / scalar
    gamma path, ONE rounding (a fused multiply-add with the zero beta term rounds the same).  Rests on check_scale_probe."""
    return _gamma_cases(device, M_GAMMA_CASES, 9400)


def check_mantissa_gamma_image_bf16(device):
    """The gamma image on bf16 tensors, both forward lane layouts: float64 -> fp32 -> bf16."""
    cases = tuple(c for c in M_GAMMA_CASES if c[0] % 8 == 0)[:3]
    return _both_bf16_forms(lambda: _gamma_cases(device, cases, 9450, BF16, soft=False))


# isolated masks need K <= H W pixels; (32, 10) at 64 x 5 x 33: four workgroups per sample, uneven tiles, zero slabs
M_BWD_CASES = (
    (64, 10, BASE, True), (64, 16, BASE, True), (32, 16, BASE, True), (96, 10, BASE, True), (48, 10, BASE, True),
    (128, 7, (1, 5, 40), True), (6, 3, BASE, True), (64, 10, (1, 17, 70), True), (32, 10, (64, 5, 33), False),
)


def _bwd_cases(device, cases, seed, dtype=F32, soft=True):
    n = 0
    for ci, (C, K, shape, on_emu) in enumerate(cases):
        if device == "cpu" and not on_emu:
            continue
        B, H, W = shape
        gen = torch.Generator().manual_seed(seed + ci)
        hard, r = onehot_mask("isolated", B, K, H, W, device)
        claimed = {(int(y), int(x)) for y, x in (r[0] < K).nonzero().tolist()}
        if H >= 9 and W >= 33:
            assert (0, 0) in claimed and (7, 31) in claimed and (8, 32) in claimed and any(x == W - 1 for _, x in claimed)
        plan = [(hard, m) for m in modes_of(C) if m != "none"]
        if soft:
            plan += [(soft_mask("isolated", B, K, H, W, gen), "none"), (hard, "none")]
        for mask, mode in plan:
            for ag, ab in ((1.0, 1.0), (0.5, 0.5)):
                inp = mantissa_inputs(C, K, shape, gen, ag, ab, dtype)
                relu = n % 2 == 0
                out_in = _ints(gen, -1, 2, B, H, W, C)                    # the backward's `out`: a quarter each <, == 0
                ref = reference(inp, mask, relu, False, s=_s32(inp), out_in=out_in)
                assert int(ref["dD_terms"].max()) <= 1 and int(ref["dD_terms"].sum()) >= 4 * K, "one pixel per dD element"
                dgam = ref["dgam"].to(F32).to(F64)                       # fl32(g0 xh): the product is exact in float64
                G = _once(ag * dgam, dtype)                              # bf16: rounded once for the matrix cores
                Bv = _once(ab * ref["g0"], dtype)
                want = {"dres": ref["dres"], "dD": dD64(mask, G, Bv)[0],
                        "dgb2": _once(torch.cat(((1 - ag) * dgam, (1 - ab) * ref["g0"]), -1), dtype)}
                assert _is32(want["dD"]) and int((want["dD"] != 0).sum()) >= 4 * K * C
                got = run(device, inp, mask, mode, relu, False, dtype, out_in=out_in)
                bad = {nm: _nbad(got[nm], w) for nm, w in want.items()}
                assert not any(bad.values()), ("full-mantissa backward mismatching elements", C, K, shape, mode, ag,
                                               str(dtype), bad)
                if mode == "region_only" and dtype == F32 and ag == 0.5:     # k_sean_bwd_a_onehot<float, 1, AMAX = true>
                    fused = run(device, inp, mask, mode, relu, False, out_in=out_in, amax=True)
                    bad = {nm: _nbad(fused[nm], w) for nm, w in want.items()}
                    assert not any(bad.values()), ("fused-amax backward mismatching elements", C, K, shape, bad)
                    _amax_ok(fused, (C, K, shape))
                n += 1
    return {"runs": n}


def check_mantissa_backward(device):
    """M backward, M_BWD_CASES on `isolated` masks (one-hot in the gather modes and through the soft kernels; soft with the
    values 0.5 and -2) at alphas 1 and 0.5, 24-bit dout, a given `out` with zeros and negatives under ReLU:  dgam = fl32(g0
    xh);  dgb2 == ((1 - a_g) dgam, (1 - a_b) g0);  every dD[s, tap, k, c] == m a (dgam | g0) of its single contributing
    pixel (asserted: at most one term per element), all 24 bits, through the three-piece bf16 split, sG, the matrix cores,
    the slabs and their reduction (the scalar kernel: LDS and global atomics onto zero).  Claimed pixels include an image
    corner, tile corners and the last column (asserted)."""
    return _bwd_cases(device, M_BWD_CASES, 9500)


def check_mantissa_backward_bf16(device):
    """The same on bf16 tensors (k_sean_bwd_a_onehot<bf16_t, 2>; 8-bit dout): dgb2 is float64 -> fp32 -> bf16 and dD is m
    bf16(fl32(a (dgam | g0))): G is rounded to bf16 once by design."""
    cases = tuple(c for c in M_BWD_CASES if c[0] % 8 == 0 and c[2] != (64, 5, 33))[:4]
    return _bwd_cases(device, cases, 9550, BF16, soft=False)


def check_mantissa_pass_b(device):
    """M for pass B at H W = 256 (POW2), t == mean, integer data: dxh and S1 are exact, S1 / N is exact (N = 2^8) and the S2
    term is an exact zero, so dt = fl32(s32 (dxh - S1 / N)): ONE rounding whether or not the compiler fuses anything.
    C = 32, 64, 128: k_sean_bwd_b_rows; 48, 96: the float4 branch of k_sean_bwd_b; 6: its scalar branch; with dt_amax= as
    well (bitwise the same dt, and the maximum of it)."""
    n = 0
    for ci, (C, K) in enumerate(((32, 16), (64, 10), (128, 7), (48, 10), (96, 10), (6, 3))):
        gen = torch.Generator().manual_seed(9600 + ci)
        B, H, W = POW2
        mask = onehot_mask("hashed", B, K, H, W, device)[0]
        for mode in modes_of(C):
            relu, use_res, ag, ab = E_COMBOS[n % len(E_COMBOS)]
            inp = int_inputs(C, K, POW2, gen, ag, ab)
            inp["var"] = inp["var"].to(F32).to(F64)
            ref = reference(inp, mask, relu, use_res, s=_s32(inp))
            assert float(ref["xh"].abs().max()) == 0.0 and int((ref["dt"] != 0).sum()) > ref["dt"].numel() // 2
            want = ref["dt"].to(F32)
            got = run(device, inp, mask, mode, relu, use_res)
            bad = _nbad(got["dt"], want)
            assert bad == 0, ("pass B mismatching elements", C, K, mode, bad)
            if mode == "region_only":
                fused = run(device, inp, mask, mode, relu, use_res, amax=True)
                assert torch.equal(fused["dt"], got["dt"]) and fused["amax"][1] == float(want.abs().max()), (C, K)
            n += 1
    return {"runs": n}


def check_mantissa_table(device):
    """M for the rows that feed dxhat and the forward with all 24 bits: the per-region table of sean_gather_interior, the
    gather, the bias fold of sean_stage_D, the soft MFMA chain and the scalar loop.  One-hot `uniform` and `blob` masks at
    POW2 (wave steps that take the table are asserted to exist), t == mean, a_g = a_b = 1.  D is arbitrary float32 with ONE
    non-zero tap per channel (tap = c % 9, whatever the region), the biases are arbitrary float32: g1 = fl32(bias_g + D[tap,
    r(p + tap), c]) and b1 likewise are one term plus the bias - ONE rounding in any summation order.  Then out == b1
    exactly, and with dout = +-2^j at one pixel per (b, c): dxh = +-2^j fl32(1 + g1), S1 is that one value, S1 / 256 is
    exact, dt = fl32(s32 fl32(dxh - S1 / 256)) - each operation rounded on its own in float32 numpy, and no fused
    multiply-add the compiler may form changes any of them (its addend is an exact zero or its product is exact)."""
    n = interior = 0
    B, H, W = POW2
    for ci, (C, K) in enumerate(((64, 10), (96, 10), (32, 16), (128, 7), (6, 3))):
        gen = torch.Generator().manual_seed(9650 + ci)
        for kind in ("uniform", "blob"):
            mask, r = onehot_mask(kind, B, K, H, W, device)
            interior += interior_counts(r, K)[0]
            for mode in modes_of(C):
                inp = int_inputs(C, K, POW2, gen, 1.0, 1.0)
                keep = (torch.arange(9).view(9, 1, 1) == (torch.arange(C) % 9).view(1, 1, C)).to(F64)
                sign = lambda *s: (torch.randint(0, 2, s, generator=gen) * 2 - 1).to(F64)
                val = sign(B, 1, C) * 2.0 ** torch.randint(-3, 4, (B, 1, C), generator=gen).to(F64)
                dout = torch.zeros(B, H * W, C, dtype=F64).scatter_(1, torch.randint(0, H * W, (B, 1, C), generator=gen), val)
                inp.update(var=inp["var"].to(F32).to(F64), D=torch.randn(B, 2, 9, K, C, generator=gen).to(F64) * keep,
                           bg=torch.randn(C, generator=gen).to(F64), bb=torch.randn(C, generator=gen).to(F64),
                           dout=dout.reshape(B, H, W, C))
                g1c, b1c = dynconv64(mask, inp["D"])
                assert float(dynconv64(mask, (inp["D"] != 0).to(F64))[0].max()) <= 1.0, "one term per (pixel, channel)"
                f = lambda x: x.to(F32).numpy()
                assert _is32(g1c) and _is32(b1c) and int((g1c != 0).sum()) > g1c.numel() // 2
                g1, b1 = f(inp["bg"]) + f(g1c), f(inp["bb"]) + f(b1c)                  # float32: one rounding each
                dxh = f(inp["dout"]) * (np.float32(1.0) + g1)                          # (+-2^j: exact)
                S1 = dxh.astype(np.float64).sum((1, 2), keepdims=True).astype(np.float32)   # (one non-zero term)
                dt = scale32(f(inp["var"]))[:, None, None, :] * (dxh - S1 * np.float32(1.0 / (H * W)))
                assert dt.dtype == np.float32 and int((dt != 0).sum()) > dt.size // 2
                got = run(device, inp, mask, mode, False, False)
                bad = {"out": _nbad(got["out"], torch.from_numpy(b1)), "dt": _nbad(got["dt"], torch.from_numpy(dt))}
                assert not any(bad.values()), ("full-mantissa table mismatching elements", C, K, kind, mode, bad)
                n += 1
    assert interior > 0, "input condition: no wave step takes the interior table"
    return {"runs": n, "interior groups": interior}


# ---------------------------------------------------------------------------------------------------------------------
# fused amax, powers of two
# ---------------------------------------------------------------------------------------------------------------------
def general_inputs(C, K, shape, gen, bf_valued=False):
    """The Gaussian inputs of soft_mask_checks.make_inputs with mean and var of t (float64 statistics rounded to fp32)."""
    B, H, W = shape
    g = gaussian_inputs(C, K, gen, B, H, W, bf_valued=bf_valued)
    t = g["t"].to(F64)
    inp = {k: g[k].to(F64) for k in ("t", "gb2", "res", "D", "bg", "bb", "dout")}
    inp.update(mean=t.mean((1, 2)).to(F32).to(F64), var=t.var((1, 2), unbiased=False).to(F32).to(F64),
               ag=float(g["ag"].item()), ab=float(g["ab"].item()))
    return inp


def check_amax_forms(device):
    """The AMAX = true instantiations (amax=, dt_amax=, dgb2_amax= with flag None: k_sean_fwd_onehot<..., true>,
    k_sean_bwd_a_onehot<float, 1, true>, pass B with a maximum): every tensor bitwise that of the plain form (atomically
    summed ones: on the emulator), every maximum bitwise max |tensor| of the returned tensor.  Gaussian data; (128, 7): two
    slices; (96, 10): dead lanes that shadow channel 0; 64 x 5 x 33: idle workgroups commit too."""
    n = 0
    for ci, (C, K, shape) in enumerate(((64, 10, BASE), (96, 10, BASE), (128, 7, (1, 5, 40)), (64, 10, (1, 17, 70)),
                                        (32, 10, (64, 5, 33)))):
        if device == "cpu" and shape == (64, 5, 33):          # MI355X only (emulator: 10 s a run)
            continue
        gen = torch.Generator().manual_seed(9700 + ci)
        inp = general_inputs(C, K, shape, gen)
        mask = onehot_mask("hashed", shape[0], K, *shape[1:], device)[0]
        for relu, use_res in ((True, True), (False, False)):
            plain = run(device, inp, mask, "region_only", relu, use_res)
            fused = run(device, inp, mask, "region_only", relu, use_res, amax=True)
            for nm in ("out", "dgb2", "dD", "dres") + (GRADS if device == "cpu" else ()):
                assert torch.equal(plain[nm], fused[nm]), ("fused-amax form differs", nm, C, K, shape)
            _amax_ok(fused, (C, K, shape))
            n += 1
    return {"runs": n}


def check_pow2_scaling(device):
    """dout scaled by 2^-20 and by 2^12 scales dres, dgb2 and dD (slabs summed in a fixed order; not the scalar kernel's
    atomically summed dD on the GPU) bit for bit in every form, and on the emulator every other gradient too.  Gaussian
    data, fp32 in every mode and bf16 in the gather mode."""
    n = 0
    for ci, (C, K, shape) in enumerate(((64, 10, BASE), (96, 10, BASE), (6, 3, BASE), (32, 10, (64, 5, 33)))):
        if device == "cpu" and shape == (64, 5, 33):          # MI355X only (emulator: 10 s a run)
            continue
        gen = torch.Generator().manual_seed(9800 + ci)
        B, H, W = shape
        hard = onehot_mask("hashed", B, K, H, W, device)[0]
        soft = soft_mask("real", B, K, H, W, gen)
        forms = [(hard, m, F32) for m in modes_of(C)] + [(soft, "none", F32)]
        forms += [(hard, "region_only", BF16)] if C % 8 == 0 else []
        for mask, mode, dtype in forms:
            inp = general_inputs(C, K, shape, gen, bf_valued=dtype == BF16)
            base = run(device, inp, mask, mode, True, True, dtype)
            for e in (-20, 12):
                scaled = run(device, dict(inp, dout=inp["dout"] * 2.0 ** e), mask, mode, True, True, dtype)
                names = ["dres", "dgb2"] + (["dD"] if C % 4 == 0 or device == "cpu" else [])
                names += [g for g in GRADS if g not in names] if device == "cpu" else []
                for nm in names:
                    want = (base[nm].to(F64) * 2.0 ** e).to(base[nm].dtype)
                    assert torch.equal(scaled[nm], want), ("not scaled bit for bit", nm, e, C, K, shape, mode, str(dtype))
                n += 1
    return {"runs": n}


# ---------------------------------------------------------------------------------------------------------------------
# U. the derived per-element bound
# ---------------------------------------------------------------------------------------------------------------------
def _bound_counts(C, K, shape, onehot, terms):
    """n per quantity: the roundings on the longest path, counted from csrc/sean.hip without any fused multiply-add (a
    fused one only removes roundings).  A sum of N terms in any order counts N (the any-order bound of
    fp32_exact_checks.check_bound); s(var) counts 6 (two square roots and three divisions / additions propagated).
      g1, b1   one-hot: bias + 9 rows = 10 terms; soft / scalar: 9 K products + bias = 9 K + 1       -> n1
      gam, bet (1 - a) 1, two products 2, one addition 1                                              -> n1 + 4
      xh       t - mean 1, s 6, product 1                                                             -> 8
      out      gam + 1 addition (1 + gam) + product + addition of bet + residual: (n1 + 4) + 4, xh 8  -> n1 + 16
      dgam     g0 xh                                                                                   -> 9
      dgb2     (1 - a) 1 and the product 1 on dgam                                                     -> 11
      G        a dgam                                                                                  -> 10
      dD       G 10, the product with the mask 1, T terms: the pixels whose mask value is not zero for this (tap, k),
               counted from the mask (``terms``: dD_terms of reference()), three exact pieces each in the one-hot fp32
               form (the pieces are exact, their products with 0 / 1 are exact, the matrix cores add 3 T terms), the
               slabs                                                                                  -> 11 + (3 | 1) T + slabs
      dbias    G 10 (beta: a g0, 1), B H W terms                                                       -> 10 | 1 + B H W
      dalpha   dgam 9, g1 - g2: n1 + 1, product 1, B H W C terms                                       -> n1 + 11 + B H W C
      dxh      g0 (1 + gam): (n1 + 4) + 1 + 1                                                         -> n1 + 6
      S1       dxh, H W terms                                                                          -> n1 + 6 + H W
      S2       dxh, t - mean 1, product 1, H W terms                                                   -> n1 + 8 + H W
      dt       first term: S1, 1 / N 1, S1 / N 1, the difference 1, s 6, product 1, the sum 1          -> n1 + H W + 17
               second term: s' (s 6, a 1, a a 1, two divisions and a product in each of two parts 6, their sum 1,
               the product with s 1 = 16), 1 / N 1, three products 3, S2, the sum 1: n1 + 8 + H W + 21 -> n1 + H W + 29"""
    B, H, W = shape
    n1 = 10 if onehot else 9 * K + 1
    slabs = min(max(256 // B, 1), -(-W // 32) * -(-H // 4))
    return {"out": n1 + 16, "dgb2": 11, "dD": (11 + (3 if onehot else 1) * terms + slabs).to(F64).reshape(B, 1, 9, K, 1), "dbg": 10 + B * H * W,
            "dbb": 1 + B * H * W, "dag": n1 + 11 + B * H * W * C, "dab": n1 + 11 + B * H * W * C, "dt": n1 + H * W + 29}


# the emulator runs one case per kernel form (the others repeat a form at another C, K: about a second a run there)
U_CASES = (
    (64, 10, BASE, True), (64, 16, BASE, False), (64, 1, BASE, False), (32, 16, BASE, False), (96, 10, BASE, True),
    (48, 10, BASE, False), (128, 7, (1, 5, 40), True), (6, 3, BASE, True), (64, 10, (3, 2, 3), True),
    (64, 10, (1, 17, 70), False), (32, 10, (64, 5, 33), False),
)


def _spread_inputs(C, K, shape, gen):
    """General data whose magnitude changes with the channel over 2^-6 .. 2^6 (an error in a small-magnitude channel is
    judged against that channel), mean and var given freely (not the statistics of t)."""
    B, H, W = shape
    rn = lambda *s: torch.randn(*s, generator=gen)
    e = 2.0 ** ((torch.arange(C) * 5) % 13 - 6).to(F32)
    f = lambda x: x.to(F32).to(F64)
    return dict(t=f(rn(B, H, W, C) * e), mean=f(rn(B, C) * e * 0.5), var=f((torch.rand(B, C, generator=gen) + 0.05) * e * e),
                gb2=f(rn(B, H, W, 2 * C)), res=f(rn(B, H, W, C) * e), D=f(rn(B, 2, 9, K, C) * 0.2), bg=f(rn(C) * 0.2),
                bb=f(rn(C) * e), ag=0.625, ab=0.25, dout=f(rn(B, H, W, C)))


def check_bound(device):
    """U on U_CASES, in every dispatch mode, on two data sets: `spread` (_spread_inputs) and the Gaussian inputs of
    soft_mask_checks.make_inputs; one-hot `blob` masks on one and `hashed` masks on the other in the region modes, `real`
    soft masks in "none".
    |kernel - float64| <= n 2^-24 M in every element of out, dgb2, dD, dbias, dalpha and dt, n from _bound_counts, M from
    reference() (for dt: |s| (|dxh| + |S1| / N) + |s'| (2 / N) |t - mean| |S2|, both sums over absolute values).  The
    backward is given the float64 output rounded to fp32 as its `out`, so relu' is the reference's.  Prints and returns
    the worst error / bound per quantity beside the same figure for the float32 torch restatement of reference()."""
    worst, worst32 = {}, {}
    for ci, (C, K, shape, on_emu) in enumerate(U_CASES):
        if device == "cpu" and not on_emu:
            continue
        B, H, W = shape
        gen = torch.Generator().manual_seed(9900 + ci)
        soft = soft_mask("real", B, K, H, W, gen)
        for di, make in enumerate((_spread_inputs, general_inputs)):
            inp = make(C, K, shape, gen)
            hard = onehot_mask(("blob", "hashed")[(ci + di) % 2], B, K, H, W, device)[0]   # (blob: the interior table)
            for mask, mode in [(hard, m) for m in modes_of(C) if m != "none"] + [(soft, "none")]:
                relu, use_res = (ci + di) % 2 == 0, di == 0
                ref = reference(inp, mask, relu, use_res)
                out_in = ref["out"].to(F32).to(F64)
                ref32 = reference({k: (v.to(F32) if torch.is_tensor(v) else v) for k, v in inp.items()}, mask.to(F32),
                                  relu, use_res, out_in=out_in.to(F32))
                got = run(device, inp, mask, mode, relu, use_res, out_in=out_in)
                counts = _bound_counts(C, K, shape, mode != "none" and C % 4 == 0, ref["dD_terms"])
                for nm, n in counts.items():
                    bound = n * U * ref["M_" + nm]
                    err = (got[nm].to(F64) - ref[nm]).abs()
                    ratio = float((err / bound.clamp_min(1e-300)).max())
                    worst[nm] = max(worst.get(nm, 0.0), ratio)
                    worst32[nm] = max(worst32.get(nm, 0.0), float(((ref32[nm].to(F64) - ref[nm]).abs() /
                                                                    bound.clamp_min(1e-300)).max()))
                    assert bool((err <= bound).all()), ("per-element bound", nm, C, K, shape, mode, "n", n if isinstance(n, int) else "per element", "elements over",
                                                        int((err > bound).sum()), "worst error / bound", ratio)
    for nm in worst:
        print("sean bound  %-5s worst error / bound = %.4f   (float32 torch: %.4f)" % (nm, worst[nm], worst32[nm]))
    return {nm: (round(worst[nm], 4), round(worst32[nm], 4)) for nm in worst}
