"""The bf16 path at op level, as sharp as arithmetic allows: the 3x3 trunk convolutions (csrc/conv_bf16_mfma.hip, the
persistent LDS-DMA form csrc/conv_bf16_v2.hip), the 9x9 output convolution (csrc/conv9_bf16_mfma.hip), the data movers and
weight re-layouts of csrc/s2d.hip, the elementwise / cast / layout / clamp / resize kernels of csrc/edge.hip and the
activation backward of csrc/conv_direct.hip.  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_bf16_exact.py runs every one of them on both.

Four kinds of gate, none of them a max-norm figure per tensor:
  integer data      operands are small integers, so every product and partial sum is an integer below 2^24 and the fp32
                    accumulation is exact in ANY order: bf16 outputs must equal the float64 result rounded once, fp32
                    outputs the float64 result itself, in every element
  planted taps      one 1.0 in the input and a kernel whose entries name their own index: the output is an image of the
                    kernel, compared exactly
  float64 bound     a derived per-element bound on Gaussian and on all-positive operands (check_conv_bound)
  powers of two     scaling operands by powers of two scales every output bit for bit
Data movement and single-operation kernels are compared with torch.equal.  Inputs come from seeded torch.Generators on the
CPU; every check restores ops.set_conv_bf16_impl(0)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from dasr_amd import ops
from tests.parity_checks import nchw, nhwc

BF16 = torch.bfloat16
F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_LRELU = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU

# ops.set_conv_bf16_impl values (csrc/conv_bf16_v2.hip): 1 = the first kernel everywhere; 0 = the persistent kernel, 4 waves
# at these sizes; 2 + 32 = 8 waves / 16-row tiles and ONE workgroup per XCD (every workgroup walks a list of items);
# 2 + 16 = 4 waves / 8-row tiles, one workgroup per XCD (MI355X only)
IMPLS = {"cpu": (1, 0, 2 + 32), "cuda": (1, 0, 2 + 32, 2 + 16)}

# (Cin, Cout, B, H, W, bias, act, residual, ps_r)
#   (32, 32, 1, 1, 1)     one pixel; Cout % 64 != 0: the first kernel in every impl
#   (32, 64, 2, 9, 33)    a ragged second tile row and column of 8-row tiles; one channel chunk; NT = 2
#   (64, 32, 1, 7, 31)    a single ragged tile; two chunks; the dgrad is the persistent kernel (produces 64 channels)
#   (64, 128, 1, 17, 34)  ragged rows of 8- and 16-row tiles (17 = 2 * 8 + 1 = 16 + 1), two tile columns; NT = 4
#   (96, 64, 3, 8, 32)    three chunks; exact 8-row tile; three samples: the item list crosses the batch boundary
#   (128, 64, 1, 16, 32)  four chunks; exact 16-row tile
#   (32, 288, 1, 3, 5)    PixelShuffle(3): the first kernel's forward; Cout = 9 * 32
CONV_CASES = (
    (32, 32, 1, 1, 1, True, ACT_RELU, True, 1),
    (32, 64, 2, 9, 33, False, ACT_NONE, False, 1),
    (64, 32, 1, 7, 31, True, ACT_LRELU, False, 1),
    (64, 128, 1, 17, 34, True, ACT_LRELU, False, 2),
    (96, 64, 3, 8, 32, True, ACT_RELU, True, 1),
    (128, 64, 1, 16, 32, True, ACT_LRELU, False, 1),
    (32, 288, 1, 3, 5, True, ACT_LRELU, False, 3),
)


def _with_impl_restored(fn):
    def wrapped(device):
        try:
            return fn(device)
        finally:
            ops.set_conv_bf16_impl(0)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


def _bf(x):
    """The value a bf16 tensor holds, in float64."""
    return x.to(torch.float32).to(BF16).to(F64)


def _once(x64):
    """float64 -> bf16 with ONE rounding (torch casts float64 through float32 first: exact here only because every value
    that takes this road is asserted to be representable in float32)."""
    x32 = x64.to(torch.float32)
    assert torch.equal(x32.to(F64), x64), "reference value is not a float32: the cast to bf16 would round twice"
    return x32.to(BF16)


def _poison(t):
    """Overwrite a result that has been read back: the allocator hands the block to the next result of that size, and a
    kernel that skipped a store would otherwise find the previous - often identical - values already in place."""
    if t.dtype == torch.uint8:
        t.fill_(0xA5)
    else:
        t.fill_(float("nan"))


def _take(t):
    """A result as a CPU copy; the tensor it came in is poisoned."""
    c = t.detach().cpu().clone()
    _poison(t)
    return c


def _same(got, want, poison=True):
    """Bit-for-bit equality of two tensors that hold no NaN (-0 and +0 differ).  ``got``, a kernel's result, is poisoned
    after it has been read (``poison=False``: it is used again)."""
    dev = got.detach()
    got = dev.cpu().clone()
    if poison:
        _poison(dev)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, want.dtype, got.shape, want.shape)
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[got.element_size()]
    return torch.equal(got.contiguous().view(it), want.contiguous().view(it))


def _nbad(got, want):
    return int((got.detach().cpu().to(F64) != want.to(F64)).sum())


def _v2_expected(impl, red, prod, ps_r=1, residual=False, accumulate=False):
    """conv_bf16_v2_supported (csrc/conv_bf16_v2.hip) in the kernel's terms: reduction / produced channels."""
    return ((impl & 3) != 1 and red % 32 == 0 and prod % 64 == 0 and
            (ps_r == 1 or (ps_r == 2 and not residual and not accumulate)))


def _counted(expect_v2, fn):
    """Run one op and assert, from the launch counter, which of the two kernels carried it."""
    n0 = ops.conv_bf16_v2_launches()
    out = fn()
    n = ops.conv_bf16_v2_launches() - n0
    assert n == int(bool(expect_v2)), ("persistent-kernel launches", n, "expected", int(bool(expect_v2)))
    return out


def _ref_fwd(x, w, bias, res, act, ps_r, pad=1, exact_lrelu=True):
    """float64 NCHW reference of conv + bias -> PixelShuffle -> + residual -> activation.  LeakyReLU is one fp32 multiply
    fp32(v) * fp32(0.2), as the kernels' epilogue has it (``exact_lrelu``: v must be a float32 value)."""
    v = F.conv2d(x, w, bias, padding=pad)
    if ps_r > 1:
        v = F.pixel_shuffle(v, ps_r)
    if res is not None:
        v = v + res
    if act == ACT_RELU:
        v = v.clamp_min(0.0)
    elif act == ACT_LRELU:
        v32 = v.to(torch.float32)
        assert not exact_lrelu or torch.equal(v32.to(F64), v)
        v = torch.where(v32 > 0, v32, v32 * torch.tensor(0.2, dtype=torch.float32)).to(F64)
    return v


def _pack(w_oihw, device, dtype=BF16):
    """OIHW float64 -> the packed kernel (HWIO + per-tap transpose) on ``device``."""
    return ops.pack_hwio(w_oihw.permute(2, 3, 1, 0).contiguous().to(torch.float32).to(dtype).to(device))


def _dev(x_nchw, device, dtype=BF16):
    return nhwc(x_nchw).to(torch.float32).to(dtype).to(device)


def _ref_grads(x, w, dy, pad=1):
    """float64 (dx, dw OIHW, db) of the pure convolution."""
    xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bt = torch.zeros(w.shape[0], dtype=F64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(xt, wt, bt, padding=pad), (xt, wt, bt), dy)


def _trunk_ops(device, impl, x, w, bias, res, act, ps_r, dy, base, fwd=True, dgrad=True):
    """y, dx, dx accumulated onto ``base``, dw, db of one 3x3 layer from the bf16 entry points (all arguments float64 NCHW /
    OIHW holding bf16 values), with the kernel that carried each asserted from the launch counter.  ``fwd`` / ``dgrad``
    False: that part is not run and comes back as None."""
    cout, cin = w.shape[0], w.shape[1]
    xd, wp, dyd = _dev(x, device), _pack(w, device), _dev(dy, device)
    bd = None if bias is None else bias.to(torch.float32).to(device)
    rd = None if res is None else _dev(res, device)
    y = dx = acc = None
    if fwd:
        y = _counted(_v2_expected(impl, cin, cout, ps_r, res is not None),
                     lambda: ops.conv2d_fwd(xd, wp, bd, rd, 1, 1, False, act, ps_r))
        assert y.dtype == BF16
    if dgrad:
        dx = _counted(_v2_expected(impl, cout, cin), lambda: ops.conv2d_dgrad(dyd, wp, xd.shape, out_dtype=BF16))
        acc = _dev(base, device).clone()
        _counted(_v2_expected(impl, cout, cin, accumulate=True), lambda: ops.conv2d_dgrad(dyd, wp, xd.shape, out=acc))
        assert dx.dtype == BF16 and acc.dtype == BF16
    dw, db = ops.conv2d_wgrad(xd, dyd, (3, 3, cin, cout))
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    return tuple(None if t is None else _take(t) for t in (y, dx, acc, dw, db))


@_with_impl_restored
def check_conv_integer_exact(device):
    """A.1: ops.conv2d_fwd / conv2d_dgrad (plain and ``out=`` accumulating) / conv2d_wgrad on bf16 tensors holding integers:
    x, w, dy in [-2, 2], bias in [-3, 3], residual and accumulate base in [-4, 4], over CONV_CASES with their epilogues, in
    every impl of IMPLS.  y and dx must equal the float64 reference rounded once to bf16, dw and db the float64 sums, in
    every element.  The accumulating dgrad is pinned to "add in fp32, round once": bf16(dx + base).  A second operand set
    (x, w, dy in [0, 2]: y and dx up to 36 K, where a bf16 ulp is 2 to 32 - in the signed set nearly every sum is below 256
    and needs no rounding at all) exercises the rounding of every output and makes the accumulate model differ from "round
    dx, add, round again" - asserted as a condition on the inputs - so the pin tells the two apart."""
    n_cases = n_two_models = 0
    for impl in IMPLS[device]:
        ops.set_conv_bf16_impl(impl)
        for ci, (cin, cout, B, H, W, has_bias, act, has_res, ps) in enumerate(CONV_CASES):
            for positive in (False, True):
                gen = torch.Generator().manual_seed(9100 + 2 * ci + positive)
                x = _ints(gen, 0 if positive else -2, 2, B, cin, H, W)
                w = _ints(gen, 0 if positive else -2, 2, cout, cin, 3, 3)
                dy = _ints(gen, 0 if positive else -2, 2, B, cout, H, W)
                bias = _ints(gen, -3, 3, cout) if has_bias else None
                res = _ints(gen, -4, 4, B, cout // (ps * ps), H * ps, W * ps) if has_res else None
                base = _ints(gen, -4, 4, B, cin, H, W)
                y_ref = _once(_ref_fwd(x, w, bias, res, act, ps))
                gx, gw, gb = _ref_grads(x, w, dy)
                dx_ref, acc_ref = _once(gx), _once(gx + base)
                two_roundings = (dx_ref.to(F64) + base).to(torch.float32).to(BF16)
                n_two_models += int((two_roundings != acc_ref).sum())
                y, dx, acc, dw, db = _trunk_ops(device, impl, x, w, bias, res, act, ps, dy, base)
                bad = {"y": _nbad(nchw(y), y_ref), "dx": _nbad(nchw(dx), dx_ref), "dx_acc": _nbad(nchw(acc), acc_ref),
                       "dw": _nbad(dw.permute(3, 2, 0, 1), gw), "db": _nbad(db, gb)}
                tag = (impl, cin, cout, B, H, W, act, ps, "positive" if positive else "signed")
                assert not any(bad.values()), ("mismatching elements", tag, bad)
                assert _same(nchw(y), y_ref) and _same(nchw(dx), dx_ref) and _same(nchw(acc), acc_ref), ("sign of zero", tag)
                n_cases += 1
    assert n_two_models > 0, "input condition: the two rounding models of the accumulating dgrad never differ"
    return {"cases": n_cases, "elements where rounding dx before the add would differ": n_two_models}


def _tap_kernel(cout, cin, k=3):
    """w[co, ci, kh, kw] = 1 + kh * k + kw + 16 * ((ci + 3 co) % 8) for k = 3 (at most 121: a bf16 value); the 9x9 form
    1 + kh * 9 + kw + 128 * ((ci + co) % 2) (at most 209)."""
    co, ci = torch.arange(cout).reshape(-1, 1, 1, 1), torch.arange(cin).reshape(1, -1, 1, 1)
    kh, kw = torch.arange(k).reshape(1, 1, -1, 1), torch.arange(k).reshape(1, 1, 1, -1)
    w = 1 + kh * k + kw + (16 * ((ci + 3 * co) % 8) if k == 3 else 128 * ((ci + co) % 2))
    w = w.to(F64)
    assert torch.equal(_bf(w), w)
    return w


# impulse pixels (y, x) of the planted-tap checks at H = 17, W = 34.  Sample 0: the four corners.  Sample 1: both sides of
# the seam between the two 32-column tiles (x = 31 | 32) on both sides of the seams between tile rows of 8 rows (y = 7 | 8,
# 15 | 16) and of 16 rows (y = 15 | 16)
TAP_PIXELS = (((0, 0), (0, 33), (16, 0), (16, 33)), ((7, 31), (8, 32), (15, 32), (16, 31)))


def _impulses(C, H, W, channels, shift):
    """One 1.0 per pixel of TAP_PIXELS; the pixels of a sample take consecutive entries of ``channels``, from ``shift``."""
    t = torch.zeros(len(TAP_PIXELS), C, H, W, dtype=F64)
    for b, pixels in enumerate(TAP_PIXELS):
        for pi, (py, px) in enumerate(pixels):
            t[b, channels[(pi + shift) % len(channels)], py, px] = 1.0
    return t


@_with_impl_restored
def check_conv_planted_taps(device):
    """A.2: an input of isolated 1.0s and the kernel of _tap_kernel: around every impulse the output is a readable image of
    the kernel, and it must equal the float64 reference exactly.  64 -> 128 channels at 17 x 34, the impulses at TAP_PIXELS
    (corners in sample 0, tile seams in sample 1), each in the first or in the last channel of a 32-channel chunk (two runs:
    every pixel meets two channels).  The same for the dgrad (plain, and accumulating onto zeros) with dy as the impulses,
    and for the weight gradient with x the impulses and dy all ones, and the reverse."""
    cin, cout, H, W = 64, 128, 17, 34
    B = len(TAP_PIXELS)
    w = _tap_kernel(cout, cin)
    ones_x, ones_dy = torch.ones(B, cin, H, W, dtype=F64), torch.ones(B, cout, H, W, dtype=F64)
    base = torch.zeros(B, cin, H, W, dtype=F64)
    n = 0
    for impl in IMPLS[device]:
        ops.set_conv_bf16_impl(impl)
        for shift in (0, 1):
            x = _impulses(cin, H, W, (0, 31, 63, 32), shift)
            dy = _impulses(cout, H, W, (31, 63, 95, 127, 0, 64), shift)
            y_ref = _once(_ref_fwd(x, w, None, None, ACT_NONE, 1))
            _, gw_x, gb_x = _ref_grads(x, w, ones_dy)         # x the impulses, dy all ones
            gx_dy, gw_dy, gb_dy = _ref_grads(ones_x, w, dy)   # dy the impulses, x all ones
            dx_ref = _once(gx_dy)
            y, _, _, dw_x, db_x = _trunk_ops(device, impl, x, w, None, None, ACT_NONE, 1, ones_dy, base, dgrad=False)
            _, dx, acc, dw_dy, db_dy = _trunk_ops(device, impl, ones_x, w, None, None, ACT_NONE, 1, dy, base, fwd=False)
            bad = {"y": _nbad(nchw(y), y_ref), "dx": _nbad(nchw(dx), dx_ref), "dx_acc": _nbad(nchw(acc), dx_ref),
                   "dw (x impulses)": _nbad(dw_x.permute(3, 2, 0, 1), gw_x), "db (dy ones)": _nbad(db_x, gb_x),
                   "dw (dy impulses)": _nbad(dw_dy.permute(3, 2, 0, 1), gw_dy), "db (dy impulses)": _nbad(db_dy, gb_dy)}
            assert not any(bad.values()), ("planted taps", impl, shift, bad)
            n += 1
    return {"runs": n}


def _bound_inputs(gen, positive, cin, cout, B, H, W):
    rn = (lambda *s: torch.rand(*s, generator=gen)) if positive else (lambda *s: torch.randn(*s, generator=gen))
    x = _bf(rn(B, cin, H, W))
    w = _bf(rn(cout, cin, 3, 3) * (1.0 / math.sqrt(9 * cin)))
    bias = (rn(cout) * 0.1).to(F64)                        # fp32 parameter
    dy = _bf(rn(B, cout, H, W))
    return x, w, bias, dy


@_with_impl_restored
def check_conv_bound(device):
    """A.3: a per-element float64 bound.  Operands are rounded to bf16, the reference is float64 on the same rounded values;
    two operand sets, Gaussian (scaled as check_bf16_conv_variants scales them) and all-positive (``rand``: post-ReLU
    activations, where nothing cancels and one dropped term out of n costs about 1 / n of the magnitude term).  Epilogue:
    bias, no activation, the PixelShuffle of CONV_CASES.  Per element:
      y, dx    |got - ref| <= 2^-8 |ref| + (1 + 2^-8) * gamma * conv(|a|, |b|, |bias|),  gamma = (9 K + 2) * 2^-24
               K = reduction channels.  The exact sum s of 9 K products (+ bias) is accumulated in fp32 in some order: each
               of at most 9 K + 1 additions (and the exact bf16 x bf16 products: none) rounds by at most 2^-24 relative, so
               the accumulator errs by at most gamma * sum|terms| to first order; the store rounds once more, by at most half
               a bf16 ulp <= 2^-8 |v| of the value v it rounds, |v| <= |ref| + accumulator error
      dw, db   |got - ref| <= n * 2^-24 * conv(|x|, |dy|),  n = B * H * W <= 1024 terms, fp32 throughout
    The gate takes no margin on top of the bound.  Returns the worst error / bound per tensor and impl.
    Measured worst error / bound (Gaussian / positive), the same for every impl to three digits - emulator: y 0.964 / 0.992,
    dx 0.953 / 0.986, dw 0.090 / 0.109, db < 0.001 / 0.003; MI355X (impl 0, 1, 18, 34): y 0.964 / 0.992, dx 0.953 / 0.986,
    dw 0.093 / 0.109, db < 0.001 / 0.003.  (y and dx sit at the rounding term: a value just above a power of two that lands
    half a bf16 ulp away.)"""
    worst = {}
    for impl in IMPLS[device]:
        ops.set_conv_bf16_impl(impl)
        for ci, (cin, cout, B, H, W, _, _, _, ps) in enumerate(CONV_CASES):
            n = B * H * W
            assert n <= 1024
            for positive in (False, True):
                gen = torch.Generator().manual_seed(9300 + 2 * ci + positive)
                x, w, bias, dy = _bound_inputs(gen, positive, cin, cout, B, H, W)
                base = torch.zeros(B, cin, H, W, dtype=F64)
                y_ref = _ref_fwd(x, w, bias, None, ACT_NONE, ps)
                y_mag = _ref_fwd(x.abs(), w.abs(), bias.abs(), None, ACT_NONE, ps)
                gx, gw, gb = _ref_grads(x, w, dy)
                mx, mw, mb = _ref_grads(x.abs(), w.abs(), dy.abs())
                y, dx, _, dw, db = _trunk_ops(device, impl, x, w, bias, None, ACT_NONE, ps, dy, base)
                bounds = {
                    "y": (nchw(y), y_ref, 2.0 ** -8 * y_ref.abs() + (1 + 2.0 ** -8) * (9 * cin + 2) * 2.0 ** -24 * y_mag),
                    "dx": (nchw(dx), gx, 2.0 ** -8 * gx.abs() + (1 + 2.0 ** -8) * (9 * cout + 2) * 2.0 ** -24 * mx),
                    "dw": (dw.permute(3, 2, 0, 1), gw, n * 2.0 ** -24 * mw),
                    "db": (db, gb, n * 2.0 ** -24 * mb),
                }
                for nm, (got, ref, bound) in bounds.items():
                    err = (got.detach().cpu().to(F64) - ref).abs()
                    ok = err <= bound
                    ratio = (err / bound.clamp_min(1e-300)).max().item()
                    key = "%s impl %d %s" % (nm, impl, "positive" if positive else "gauss")
                    worst[key] = max(worst.get(key, 0.0), ratio)
                    assert bool(ok.all()), ("per-element bound", nm, impl, (cin, cout, B, H, W), positive,
                                            "elements over", int((~ok).sum()), "worst error / bound", ratio)
    for k in sorted(worst):
        print("conv bound  %-28s worst error / bound = %.3f" % (k, worst[k]))
    return {k: round(v, 4) for k, v in worst.items()}


@_with_impl_restored
def check_conv_pow2_equivariance(device):
    """A.4: (x 2^a, w 2^b, bias 2^(a+b), residual 2^(a+b), dy 2^a) for (a, b) in (40, 20), (-40, -20), (60, -60): y (bias +
    residual + LeakyReLU) and dx must scale by 2^(a+b), dw by 2^(2a), db by 2^a, bit for bit - a power of two changes no
    rounding while nothing leaves the normal range (dy is drawn with standard deviation 1/8 so that dw 2^120 stays below
    2^127).  At (64, 64, 2, 9, 33) and (128, 128, 1, 8, 35), every impl of IMPLS."""
    n = 0
    for impl in IMPLS[device]:
        ops.set_conv_bf16_impl(impl)
        for si, (cin, cout, B, H, W) in enumerate(((64, 64, 2, 9, 33), (128, 128, 1, 8, 35))):
            gen = torch.Generator().manual_seed(9400 + si)
            x, w, bias, dy = _bound_inputs(gen, False, cin, cout, B, H, W)
            dy = _bf(dy * 0.125)
            bias = bias.to(torch.float32).to(F64)
            res = _bf(torch.randn(B, cout, H, W, generator=gen))
            base = torch.zeros(B, cin, H, W, dtype=F64)
            y0, dx0, _, dw0, db0 = [t.detach().cpu().to(F64) for t in
                                    _trunk_ops(device, impl, x, w, bias, res, ACT_LRELU, 1, dy, base)]
            assert float(dw0.abs().max()) < 2.0 ** 6 and float(y0.abs().max()) > 0
            for a, b in ((40, 20), (-40, -20), (60, -60)):
                sa, sb, sab = 2.0 ** a, 2.0 ** b, 2.0 ** (a + b)
                y, dx, _, dw, db = _trunk_ops(device, impl, x * sa, w * sb, bias * sab, res * sab, ACT_LRELU, 1, dy * sa, base)
                bad = {"y": _nbad(y, y0 * sab), "dx": _nbad(dx, dx0 * sab), "dw": _nbad(dw, dw0 * (sa * sa)),
                       "db": _nbad(db, db0 * sa)}
                assert not any(bad.values()), ("power-of-two equivariance", impl, (cin, cout, B, H, W), (a, b), bad)
                n += 1
    return {"runs": n}


# ---- B: the 9x9 output convolution of the bf16 path (bf16 x, fp32 kernel and image side) ---------------------------------
# forward tiles are 8 rows x 56 columns of y, dgrad / wgrad tiles 8 x 64 (Q_TH, Q_TQ - 8, Q_TQ of csrc/conv9_bf16_mfma.hip)
CONV9_SHAPES = ((1, 1, 1, (0,)), (1, 9, 9, (0,)), (2, 11, 70, (0,)), (2, 19, 60, (0, 2)))     # (B, H, W, impls)


def _conv9_ops(device, x, w, bias, dy, base):
    cin, cout = 32, 3
    xd = _dev(x, device)
    wp = _pack(w, device, torch.float32)
    dyd = _dev(dy, device, torch.float32)
    bd = None if bias is None else bias.to(torch.float32).to(device)
    y = ops.conv2d_fwd(xd, wp, bd, pad=4)
    dx = ops.conv2d_dgrad(dyd, wp, xd.shape, pad=4, out_dtype=BF16)
    acc = _dev(base, device).clone()
    ops.conv2d_dgrad(dyd, wp, xd.shape, pad=4, out=acc)
    dw, db = ops.conv2d_wgrad(xd, dyd, (9, 9, cin, cout), pad=4)
    assert y.dtype == torch.float32 and dx.dtype == BF16 and acc.dtype == BF16
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    return tuple(_take(t) for t in (y, dx, acc, dw, db))


def _conv9_compare(device, tag, x, w, bias, dy, base):
    y_ref = _ref_fwd(x, w, bias, None, ACT_NONE, 1, pad=4)
    gx, gw, gb = _ref_grads(x, w, dy, pad=4)
    y, dx, acc, dw, db = _conv9_ops(device, x, w, bias, dy, base)
    bad = {"y": _nbad(nchw(y), y_ref), "dx": _nbad(nchw(dx), _once(gx)), "dx_acc": _nbad(nchw(acc), _once(gx + base)),
           "dw": _nbad(dw.permute(3, 2, 0, 1), gw), "db": _nbad(db, gb)}
    assert not any(bad.values()), ("9x9 mismatching elements", tag, bad)


@_with_impl_restored
def check_conv9_exact(device):
    """B: A.1 and A.2 for ops.conv2d_fwd(pad=4) / conv2d_dgrad(pad=4, out_dtype=bf16) (plain and ``out=``) /
    conv2d_wgrad(pad=4) at 32 -> 3 channels: bf16 x, fp32 w and dy, all integers in [-2, 2] (81 * 32 terms), bias in
    [-3, 3], accumulate base in [-4, 4].  y, dw, db must be exact, dx exact after one rounding (accumulating: bf16(dx +
    base)).  CONV9_SHAPES; the last with impl 0 and with impl 2 (three workgroups walk the tile list).  Then planted taps
    at (2, 11, 70) and (2, 19, 60): impulses of 1.0 in the image corners (sample 0) and on both sides of the tile seams
    (sample 1: rows 7 | 8 and, at H = 19, 15 | 16; columns 55 | 56 of the forward's tiles and 63 | 64 of the gradients',
    where W reaches them),
    channels 0 and 31, against the kernel of _tap_kernel; for the gradients dy carries the impulses."""
    n = 0
    for si, (B, H, W, impls) in enumerate(CONV9_SHAPES):
        gen = torch.Generator().manual_seed(9500 + si)
        x, w, dy = _ints(gen, -2, 2, B, 32, H, W), _ints(gen, -2, 2, 3, 32, 9, 9), _ints(gen, -2, 2, B, 3, H, W)
        bias, base = _ints(gen, -3, 3, 3), _ints(gen, -4, 4, B, 32, H, W)
        for impl in impls:
            ops.set_conv_bf16_impl(impl)
            _conv9_compare(device, ("integers", impl, B, H, W), x, w, bias, dy, base)
            n += 1
    w = _tap_kernel(3, 32, 9)
    for (B, H, W, impls) in CONV9_SHAPES[2:]:
        corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
        seams = [(7, 55), (8, 56), (7, min(63, W - 2)), (8, min(64, W - 1))] + ([(15, 20), (16, 21)] if H > 16 else [])
        for shift in (0, 1):
            x, dy = torch.zeros(B, 32, H, W, dtype=F64), torch.zeros(B, 3, H, W, dtype=F64)
            for b, pixels in enumerate((corners, seams)):
                for pi, (py, px) in enumerate(pixels):
                    x[b, (0, 31)[(pi + shift) % 2], py, px] = 1.0
                    dy[b, (pi + shift) % 3, py, px] = 1.0
            for impl in impls:
                ops.set_conv_bf16_impl(impl)
                _conv9_compare(device, ("x impulses, dy ones", impl, B, H, W, shift), x, w, None, torch.ones_like(dy),
                               torch.zeros_like(x))
                _conv9_compare(device, ("dy impulses, x ones", impl, B, H, W, shift), torch.ones_like(x), w, None, dy,
                               torch.zeros_like(x))
                n += 2
    return {"runs": n}


# =====================================================================================================================
# C. data movers, casts, elementwise, layout, resize: bit for bit
# =====================================================================================================================
E_SHAPE_TEXT = "inconsistent or non-positive sizes"        # dasr_error_string(DASR_E_SHAPE)


def _refused(fn, text=E_SHAPE_TEXT):
    try:
        fn()
    except RuntimeError as e:
        assert text in str(e), str(e)
        return True
    raise AssertionError("the call was not refused")


def _same_nan(got, want):
    """Equality in which NaN equals NaN (whatever its payload) and nothing else."""
    dev = got.detach()
    got = dev.cpu().clone()
    dev.fill_(0.5)                                     # (see _poison; NaN is a legitimate value here)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(torch.where(gn, torch.zeros_like(got), got),
                                               torch.where(wn, torch.zeros_like(want), want))


# (B, H, W, C, valid_hw)
S2D_SHAPES = ((2, 5, 7, 8, None), (1, 6, 8, 32, (5, 7)), (1, 1, 1, 4, None), (1, 1, 259, 128, None),
              (2, 3, 258, 128, (3, 257)), (1, 7, 9, 12, (0, 0)), (1, 2, 259, 256, (2, 258)))


def _s2d_reference(x, valid_hw):
    """x'[i][j][(2 py + px) C + c] = x[2 i + py][2 j + px][c], zero beyond (Hv, Wv) and beyond an odd edge (the definition
    in the header of csrc/s2d.hip), as an index map."""
    B, H, W, C = x.shape
    Hv, Wv = valid_hw if valid_hw is not None else (H, W)
    Hs, Ws = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros(B, 2 * Hs, 2 * Ws, C, dtype=x.dtype)
    xp[:, :Hv, :Wv] = x[:, :Hv, :Wv]
    return xp.reshape(B, Hs, 2, Ws, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hs, Ws, 4 * C).contiguous()


def _d2s_reference(dy, x_shape, valid_hw):
    B, H, W, C = x_shape
    Hv, Wv = valid_hw if valid_hw is not None else (H, W)
    Hs, Ws = (H + 1) // 2, (W + 1) // 2
    full = dy.reshape(B, Hs, Ws, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hs, 2 * Ws, C)
    out = torch.zeros(B, H, W, C, dtype=dy.dtype)
    out[:, :Hv, :Wv] = full[:, :Hv, :Wv]
    return out


def check_space_to_depth(device):
    """ops.space_to_depth2 (fp32 and bf16 input) and ops.depth_to_space2_bwd (fp32 and bf16 dx, plain and ``out=``
    accumulating: one fp32 add, one rounding) against the index map of the csrc/s2d.hip header, torch.equal.  S2D_SHAPES:
      (2, 5, 7, 8)            odd H and W: a zero row and column at the edge
      (1, 6, 8, 32, (5, 7))   valid extents inside an even image
      (1, 1, 1, 4)            one pixel
      (1, 1, 259, 128), (2, 3, 258, 128, (3, 257))   Ws * C = 16640 / 16512 threads of work per row > 64 blocks x 256: the
                              forward's grid-stride loop makes a second trip
      (1, 7, 9, 12, (0, 0))   nothing valid: all zeros, and a zero gradient
      (1, 2, 259, 256, (2, 258))   W * C / 4 = 16576 > 64 x 256: the adjoint's loop makes a second trip
    Refusals with the ABI's shape error: C % 4 != 0, valid_hw beyond (H, W), B * ceil(H / 2) > 65535 (adjoint: B * H)."""
    n = 0
    for si, (B, H, W, C, valid) in enumerate(S2D_SHAPES):
        gen = torch.Generator().manual_seed(9600 + si)
        x = torch.randn(B, H, W, C, generator=gen)
        Hs, Ws = (H + 1) // 2, (W + 1) // 2
        for dt in (torch.float32, BF16):
            got = ops.space_to_depth2(x.to(dt).to(device), valid)
            assert got.dtype == BF16 and _same(got, _s2d_reference(x.to(BF16), valid)), ("space_to_depth2", S2D_SHAPES[si], dt)
            n += 1
        dy = torch.randn(B, Hs, Ws, 4 * C, generator=gen).to(BF16)
        want = _d2s_reference(dy, (B, H, W, C), valid)
        for dt in (torch.float32, BF16):
            got = ops.depth_to_space2_bwd(dy.to(device), (B, H, W, C), dt, valid_hw=valid)
            assert _same(got, want.to(dt)), ("depth_to_space2_bwd", S2D_SHAPES[si], dt)
            base = torch.randn(B, H, W, C, generator=gen).to(dt)
            acc = base.to(device).clone()
            r = ops.depth_to_space2_bwd(dy.to(device), (B, H, W, C), dt, out=acc, valid_hw=valid)
            assert r is acc and _same(acc, (base.float() + want.float()).to(dt)), ("depth_to_space2_bwd out=", S2D_SHAPES[si], dt)
            n += 2
    small = torch.zeros(1, 2, 2, 6).to(device)
    assert _refused(lambda: ops.space_to_depth2(small))
    assert _refused(lambda: ops.depth_to_space2_bwd(torch.zeros(1, 1, 1, 24, dtype=BF16).to(device), (1, 2, 2, 6), BF16))
    ok = torch.zeros(1, 2, 2, 4).to(device)
    dok = torch.zeros(1, 1, 1, 16, dtype=BF16).to(device)
    for bad in ((3, 2), (2, 3), (-1, 2)):
        assert _refused(lambda: ops.space_to_depth2(ok, bad))
        assert _refused(lambda: ops.depth_to_space2_bwd(dok, (1, 2, 2, 4), BF16, valid_hw=bad))
    tall = torch.zeros(1, 2 * 65536, 1, 4).to(device)                      # B * ceil(H / 2) = 65536
    assert _refused(lambda: ops.space_to_depth2(tall))
    assert _refused(lambda: ops.depth_to_space2_bwd(torch.zeros(1, 32768, 1, 16, dtype=BF16).to(device), (1, 65536, 1, 4), BF16))
    return {"compared": n}


S2_KH = {(0, 1): 0, (1, 0): 1, (1, 1): 2}      # (tap row r of W', input phase py) -> kh of the stride-2 kernel
T2_KH = {(0, 1): 1, (1, 1): 2, (1, 2): 0}      # (output phase a, tap row r of W') -> kh of the transposed kernel


def _expand_s2_reference(w):
    """W'[r][s][(2 py + px) Cin + c][co] = w[kh(r, py)][kw(s, px)][c][co], zero elsewhere (numpy, HWIO in and out)."""
    _, _, Cin, Cout = w.shape
    e = np.zeros((3, 3, 4 * Cin, Cout), dtype=w.dtype)
    live = np.zeros((3, 3, 4 * Cin, Cout), dtype=bool)
    for (r, py), kh in S2_KH.items():
        for (s, px), kw in S2_KH.items():
            q = 2 * py + px
            e[r, s, q * Cin:(q + 1) * Cin] = w[kh, kw]
            live[r, s, q * Cin:(q + 1) * Cin] = True
    return e, live


def _expand_t2_reference(w):
    """W'[r][s][ci][4 co + 2 a + b] = w[kh(a, r)][kw(b, s)][ci][co], zero elsewhere."""
    _, _, Cin, Cout = w.shape
    e = np.zeros((3, 3, Cin, 4 * Cout), dtype=w.dtype)
    live = np.zeros((3, 3, Cin, 4 * Cout), dtype=bool)
    for (a, r), kh in T2_KH.items():
        for (b, s), kw in T2_KH.items():
            e[r, s, :, 2 * a + b::4] = w[kh, kw]
            live[r, s, :, 2 * a + b::4] = True
    return e, live


def _collapse_reference(dwe, Cin, Cout, transposed):
    dw = np.zeros((3, 3, Cin, Cout), dtype=dwe.dtype)
    if transposed:
        for (a, r), kh in T2_KH.items():
            for (b, s), kw in T2_KH.items():
                dw[kh, kw] = dwe[r, s, :, 2 * a + b::4]
    else:
        for (r, py), kh in S2_KH.items():
            for (s, px), kw in S2_KH.items():
                q = 2 * py + px
                dw[kh, kw] = dwe[r, s, q * Cin:(q + 1) * Cin]
    return dw


def _both_halves(packed, want_hwio, what):
    """Both halves of a packed kernel (2, 3, 3, I, O): HWIO, and memory that holds every tap transposed ([tap][O][I])."""
    _, _, _, I, O = packed.shape
    assert _same(packed[0], want_hwio, poison=False), (what, "HWIO half")
    assert _same(packed[1].reshape(3, 3, O, I), want_hwio.permute(0, 1, 3, 2).contiguous(), poison=False), (what, "transposed half")


def check_weight_expand_collapse(device):
    """ops.weight_expand_s2 / weight_collapse_s2 / weight_expand_t2 / weight_collapse_t2 against the index tables of the
    csrc/s2d.hip header written out in numpy (S2_KH, T2_KH), torch.equal on both halves of the packed result; (Cin, Cout) =
    (32, 64), (4, 4), (64, 32), (128, 16).  The expanded taps that carry nothing are exactly zero (27 of the 36 slots per channel pair, in
    both forms), collapse(expand(w).float()) is bf16(w), the transposed
    form's bias expands to bias[n >> 2], and the collapsed bias gradient is (e0 + e1) + (e2 + e3) in that order.
    Then the function: a stride-2 F.conv2d and F.conv_transpose2d in float64 on integer data (x, w in [-2, 2], bias in
    [-3, 3]) equal the stride-1 forms built from these pieces - space_to_depth2 + expanded kernel, expanded kernel +
    PixelShuffle(2) - through ops.conv2d_fwd, exactly, for odd and even H, W."""
    n = 0
    for si, (Cin, Cout) in enumerate(((32, 64), (4, 4), (64, 32), (128, 16))):
        gen = torch.Generator().manual_seed(9700 + si)
        w = torch.randn(3, 3, Cin, Cout, generator=gen)
        bias = torch.randn(Cout, generator=gen)
        wp = ops.pack_hwio(w.to(device))
        wb = w.to(BF16)
        # ---- stride 2
        e_ref, live = _expand_s2_reference(wb.float().numpy())
        e = ops.weight_expand_s2(wp)
        assert e.dtype == BF16 and tuple(e.shape) == (2, 3, 3, 4 * Cin, Cout)
        _both_halves(e, torch.from_numpy(e_ref).to(BF16), ("expand_s2", Cin, Cout))
        assert int(live.sum()) == 9 * Cin * Cout and bool((e[0].float().cpu().numpy()[~live] == 0).all())
        assert _same(ops.weight_collapse_s2(e[0].float().contiguous(), Cin, Cout), wb.float()), ("collapse(expand) s2", Cin, Cout)
        dwe = torch.randn(3, 3, 4 * Cin, Cout, generator=gen)
        assert _same(ops.weight_collapse_s2(dwe.to(device), Cin, Cout),
                     torch.from_numpy(_collapse_reference(dwe.numpy(), Cin, Cout, False))), ("collapse_s2", Cin, Cout)
        # ---- transposed, stride 2
        t_ref, tlive = _expand_t2_reference(wb.float().numpy())
        t, b4 = ops.weight_expand_t2(wp, bias.to(device))
        assert t.dtype == BF16 and tuple(t.shape) == (2, 3, 3, Cin, 4 * Cout)
        _both_halves(t, torch.from_numpy(t_ref).to(BF16), ("expand_t2", Cin, Cout))
        assert int(tlive.sum()) == 9 * Cin * Cout and bool((t[0].float().cpu().numpy()[~tlive] == 0).all())
        assert _same(b4, bias[torch.arange(4 * Cout) >> 2]), ("expand_t2 bias", Cin, Cout)
        t0, none = ops.weight_expand_t2(wp, None)
        assert none is None and _same(t0, t.cpu().clone())
        dwe = torch.randn(3, 3, Cin, 4 * Cout, generator=gen)
        dbe = torch.randn(4 * Cout, generator=gen)
        dw, db = ops.weight_collapse_t2(dwe.to(device), dbe.to(device), Cin, Cout)
        assert _same(dw, torch.from_numpy(_collapse_reference(dwe.numpy(), Cin, Cout, True))), ("collapse_t2", Cin, Cout)
        assert _same(db, (dbe[0::4] + dbe[1::4]) + (dbe[2::4] + dbe[3::4])), ("collapse_t2 bias", Cin, Cout)
        dw2, db2 = ops.weight_collapse_t2(t[0].float().contiguous(), None, Cin, Cout)
        assert db2 is None and _same(dw2, wb.float()), ("collapse(expand) t2", Cin, Cout)
        n += 1
    # ---- the function the pieces exist for
    for si, (Cin, Cout, B, H, W) in enumerate(((32, 64, 2, 5, 7), (32, 64, 1, 6, 8), (64, 32, 1, 4, 5), (32, 64, 1, 3, 4))):
        gen = torch.Generator().manual_seed(9750 + si)
        x, bias = _ints(gen, -2, 2, B, Cin, H, W), _ints(gen, -3, 3, Cout)
        xd = _dev(x, device)
        bd = bias.float().to(device)
        w = _ints(gen, -2, 2, Cout, Cin, 3, 3)
        want = _once(F.conv2d(x, w, bias, stride=2, padding=1))
        y = _take(ops.conv2d_fwd(ops.space_to_depth2(xd), ops.weight_expand_s2(_pack(w, device, torch.float32)), bd))
        assert _nbad(nchw(y), want) == 0 and _same(nchw(y), want), ("stride-2 conv", Cin, Cout, H, W)
        wt = _ints(gen, -2, 2, Cin, Cout, 3, 3)                             # ConvTranspose2d: [Cin][Cout][kh][kw]
        want = _once(F.conv_transpose2d(x, wt, bias, stride=2, padding=1))
        wtp = ops.pack_hwio(wt.permute(2, 3, 0, 1).contiguous().float().to(device))
        w4, b4 = ops.weight_expand_t2(wtp, bd)
        y = _take(ops.conv2d_fwd(xd, w4, b4, ps_r=2))
        assert tuple(y.shape) == (B, 2 * H, 2 * W, Cout)
        y = nchw(y)[:, :, :2 * H - 1, :2 * W - 1].contiguous()
        assert _nbad(y, want) == 0 and _same(y, want), ("transposed stride-2 conv", Cin, Cout, H, W)
        n += 2
    return {"compared": n}


CAST_SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.00390625, 1.01171875, -1.00390625, -1.01171875,
                 3.4e38, -3.4e38, 1e-40, -1e-40)
EW_SIZES = (4, 1028, 4 * ((1 << 21) // 4 + 3))         # the last: > 2048 blocks x 256 threads x 4 elements


def check_elementwise_and_casts(device):
    """ops.add, ops.accumulate_, ops.cast_to_bf16, ops.cast_to_f32, ops.copy_ against torch: one fp32 operation and at most
    one rounding per element, so torch.equal.  Sizes n = 4, 1028 and 2097164 (above 2048 blocks x 256 threads x 4 elements:
    the grid-stride loop takes a second trip); the fp32 add / accumulate also n = 1 and 524293 (one element per thread).
    accumulate_: fp32 += fp32, bf16 += bf16, fp32 += bf16; bf16 += fp32 does not exist and raises TypeError.  The cast
    input holds CAST_SPECIALS: +-0, +-inf, NaN (stays NaN), the RNE ties 1.00390625 (down to 1.0) and 1.01171875 (up to
    1.015625), 3.4e38 (rounds to inf) and an fp32 subnormal; -0 and +0 are told apart.  n % 4 != 0 is refused by the bf16
    entry points."""
    n_cmp = 0
    sp = torch.tensor(CAST_SPECIALS, dtype=torch.float32)
    assert float(torch.tensor(1.00390625).to(BF16)) == 1.0 and float(torch.tensor(1.01171875).to(BF16)) == 1.015625
    assert bool(torch.isinf(torch.tensor(3.4e38).to(BF16)))
    for si, n in enumerate(EW_SIZES + (1, 524288 + 5)):
        gen = torch.Generator().manual_seed(9800 + si)
        a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        assert _same(ops.add(a.to(device), b.to(device)), a + b), ("add fp32", n)
        d = a.to(device).clone()
        assert ops.accumulate_(d, b.to(device)) is d and _same(d, a + b), ("accumulate_ fp32", n)
        d2 = torch.empty(n).to(device)
        assert ops.copy_(d2, a.to(device)) is d2 and _same(d2, a), ("copy_ fp32", n)
        n_cmp += 3
        if n % 4:
            continue
        a16, b16 = a.to(BF16), b.to(BF16)
        assert _same(ops.add(a16.to(device), b16.to(device)), (a16.float() + b16.float()).to(BF16)), ("add bf16", n)
        d = a16.to(device).clone()
        ops.accumulate_(d, b16.to(device))
        assert _same(d, (a16.float() + b16.float()).to(BF16)), ("accumulate_ bf16 += bf16", n)
        d = a.to(device).clone()
        ops.accumulate_(d, b16.to(device))
        assert _same(d, a + b16.float()), ("accumulate_ fp32 += bf16", n)
        d2 = torch.empty(n, dtype=BF16).to(device)
        ops.copy_(d2, a16.to(device))
        assert _same(d2, a16), ("copy_ bf16", n)
        c = a.clone()
        pos = torch.randperm(n, generator=gen)[:min(n, sp.numel())]
        c[pos] = sp[:pos.numel()]
        c[-1] = sp[2]                                                       # the last element of the last group
        got = ops.cast_to_bf16(c.to(device))
        want = c.to(BF16)
        assert got.dtype == BF16 and torch.equal(torch.isnan(got.cpu()), torch.isnan(want)), ("cast_to_bf16 NaN", n)
        keep = ~torch.isnan(want)
        assert torch.equal(got.cpu().view(torch.int16)[keep], want.view(torch.int16)[keep]), ("cast_to_bf16", n)
        back = ops.cast_to_f32(want.to(device))
        assert back.dtype == torch.float32 and torch.equal(torch.isnan(back.cpu()), torch.isnan(want)), ("cast_to_f32 NaN", n)
        assert torch.equal(back.cpu().view(torch.int32)[keep], want.float().view(torch.int32)[keep]), ("cast_to_f32", n)
        n_cmp += 6
    try:
        ops.accumulate_(torch.zeros(4, dtype=BF16).to(device), torch.zeros(4).to(device))
        raise AssertionError("bf16 += fp32 was accepted")
    except TypeError:
        pass
    z6, z6b = torch.zeros(6).to(device), torch.zeros(6, dtype=BF16).to(device)
    assert _refused(lambda: ops.add(z6b, z6b)) and _refused(lambda: ops.accumulate_(z6b.clone(), z6b))
    assert _refused(lambda: ops.accumulate_(z6.clone(), z6b))
    assert _refused(lambda: ops.cast_to_bf16(z6)) and _refused(lambda: ops.cast_to_f32(z6b))
    return {"compared": n_cmp}


# (B, Ho, Wo, Cout, ps_r): the kernel forms of conv_epilogue_bwd_impl (csrc/conv_direct.hip)
#   ps_r 1, n % 4 == 0     k_conv_epilogue_bwd_flat4; (1, 129, 64, 256): n / 4 = 528384 > 2048 x 256, a second grid pass
#   ps_r 1, n % 4 != 0     the generic kernel; (1, 1, 174763, 3): n = 524289 > 2048 x 256
#   ps_r 2, ps_r 3         k_conv_epilogue_bwd_ps<2 | 3>; Wo * Cq = 2240 and 1056: several workgroups per row;
#                          (1, 4101, 1, 4, 2) / (1, 4099, 1, 9, 3) with a maximum wanted (fp32): the row grid is capped at
#                          4096 and the kernel's two-rows-per-trip loop runs, the second row missing in its last trip
EPILOGUE_SHAPES = ((2, 5, 7, 8, 1), (1, 129, 64, 256, 1), (1, 3, 5, 3, 1), (1, 1, 174763, 3, 1), (2, 3, 5, 8, 2),
                   (1, 2, 70, 128, 2), (1, 4101, 1, 4, 2), (2, 3, 5, 18, 3), (1, 2, 33, 288, 3), (1, 4099, 1, 9, 3))


def check_epilogue_bwd(device):
    """ops.conv2d_epilogue_bwd, fp32 (with the max |.| buffer the fp32 path asks for) and bf16, against dy * (y > 0 ? 1 :
    slope) - one fp32 multiply, one rounding for bf16 - taken through the inverse PixelShuffle map (F.pixel_unshuffle),
    torch.equal.  ReLU and LeakyReLU, ps_r 1, 2, 3, EPILOGUE_SHAPES; y holds exact zeros (the slope side)."""
    n = 0
    for si, (B, Ho, Wo, Cout, ps) in enumerate(EPILOGUE_SHAPES):
        gen = torch.Generator().manual_seed(9900 + si)
        shp = (B, Ho * ps, Wo * ps, Cout // (ps * ps))
        dy, y = torch.randn(shp, generator=gen), torch.randn(shp, generator=gen)
        y[torch.rand(shp, generator=gen) < 0.1] = 0.0
        for act in (ACT_RELU, ACT_LRELU):
            slope = torch.tensor(0.0 if act == ACT_RELU else 0.2, dtype=torch.float32)
            for dt in (torch.float32, BF16):
                dyt, yt = dy.to(dt), y.to(dt)
                g = (dyt.float() * torch.where(yt.float() > 0, torch.ones((), dtype=torch.float32), slope)).to(dt)
                want = nhwc(F.pixel_unshuffle(nchw(g.float()), ps)).to(dt) if ps > 1 else g
                amax = ops.amax_buffer(dyt.to(device)) if dt == torch.float32 else None
                got = ops.conv2d_epilogue_bwd(dyt.to(device), yt.to(device), Ho, Wo, Cout, act, ps, amax=amax)
                assert tuple(got.shape) == (B, Ho, Wo, Cout)
                assert _same(got, want.contiguous()), ("epilogue_bwd", EPILOGUE_SHAPES[si], act, dt)
                if amax is not None:
                    assert ops.amax_value(amax) == float(want.abs().max()), ("epilogue_bwd max |.|", EPILOGUE_SHAPES[si], act)
                n += 1
    return {"compared": n}


LAYOUT_SHAPES = tuple((B, C, H, W) for B, (H, W) in ((2, (1, 1)), (2, (7, 9))) for C in (1, 3, 5)) + ((1, 3, 419, 419),)


def check_layout_and_clamp(device):
    """ops.nchw_to_nhwc / nhwc_to_nchw against permute().contiguous(), ops.clamp_to_nchw against torch.clamp and
    ops.clamp_to_nchw_bwd against its autograd, torch.equal with NaN == NaN.  C = 1, 3, 5 at 1 x 1 and 7 x 9, and
    (1, 3, 419, 419) = 526683 elements > 2048 x 256: a second trip of the grid-stride loop.  The clamped tensor holds
    values exactly at lo and hi (the gradient passes on the closed interval), +-inf (clamp to hi / lo, no gradient) and NaN:
    torch.clamp keeps NaN and sends no gradient through it, and so must the kernels."""
    n = 0
    for si, (B, C, H, W) in enumerate(LAYOUT_SHAPES):
        gen = torch.Generator().manual_seed(10000 + si)
        x = torch.randn(B, C, H, W, generator=gen)
        assert _same(ops.nchw_to_nhwc(x.to(device)), nhwc(x)), ("nchw_to_nhwc", LAYOUT_SHAPES[si])
        xl = torch.randn(B, H, W, C, generator=gen)
        assert _same(ops.nhwc_to_nchw(xl.to(device)), nchw(xl)), ("nhwc_to_nchw", LAYOUT_SHAPES[si])
        for lo, hi in ((0.0, 1.0), (-0.5, 0.25)):
            y = (torch.randn(B, H, W, C, generator=gen) * 0.6 + 0.3)
            flat = y.view(-1)
            sp = torch.tensor([lo, hi, float("nan"), float("inf"), float("-inf"), -0.0], dtype=torch.float32)
            k = min(flat.numel(), sp.numel())
            pos = torch.randperm(flat.numel(), generator=gen)[:k]
            flat[pos] = sp[torch.arange(k) if flat.numel() >= sp.numel() else torch.tensor([2 * (si % 3)] * k)]
            dout = torch.randn(B, C, H, W, generator=gen)
            yt = y.clone().requires_grad_(True)
            ref = nchw(torch.clamp(yt, lo, hi))
            ref.backward(dout)
            got = ops.clamp_to_nchw(y.to(device), lo, hi)
            assert _same_nan(got, ref.detach()), ("clamp_to_nchw", LAYOUT_SHAPES[si], lo, hi)
            gy = ops.clamp_to_nchw_bwd(dout.to(device), y.to(device), lo, hi)
            assert _same_nan(gy, yt.grad), ("clamp_to_nchw_bwd", LAYOUT_SHAPES[si], lo, hi)
            n += 2
    yn = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.5]).reshape(1, 2, 2, 1)
    got = ops.clamp_to_nchw(yn.to(device), 0.0, 1.0).cpu().reshape(-1)
    assert bool(torch.isnan(got[0])) and got[1:].tolist() == [1.0, 0.0, 0.5], got
    assert ops.clamp_to_nchw_bwd(torch.ones(1, 1, 2, 2).to(device), yn.to(device), 0.0, 1.0).cpu().reshape(-1).tolist() == [0.0, 0.0, 0.0, 1.0]
    return {"compared": n}


RESIZE_PAIRS = ((1, 4), (3, 10), (10, 3), (5, 7), (7, 5), (127, 64), (64, 127), (13, 100), (100, 13), (33, 97), (255, 85),
                (85, 255))


def check_resize_nearest(device):
    """ops.resize_nearest_nchw / ops.resize_nearest_u8 against F.interpolate(mode="nearest"), torch.equal.  Every (in, out)
    pair of RESIZE_PAIRS once for the rows, with another pair (five further on) for the columns; the identity returns its
    argument; the u8 form refuses H > 65535 and B > 65535 with the ABI's shape error."""
    n = 0
    for i, (h, H) in enumerate(RESIZE_PAIRS):
        w, W = RESIZE_PAIRS[(i + 5) % len(RESIZE_PAIRS)]
        gen = torch.Generator().manual_seed(10100 + i)
        x = torch.randn(2, 3, h, w, generator=gen)
        assert _same(ops.resize_nearest_nchw(x.to(device), H, W), F.interpolate(x, (H, W), mode="nearest")), ("nchw", h, w, H, W)
        r = torch.randint(0, 256, (3, h, w), generator=gen).to(torch.uint8)
        want = F.interpolate(r.float().unsqueeze(1), (H, W), mode="nearest").squeeze(1).to(torch.uint8)
        assert _same(ops.resize_nearest_u8(r.to(device), H, W), want), ("u8", h, w, H, W)
        n += 2
    xd, rd = torch.randn(1, 2, 5, 7).to(device), torch.zeros(2, 5, 7, dtype=torch.uint8).to(device)
    assert ops.resize_nearest_nchw(xd, 5, 7) is xd and ops.resize_nearest_u8(rd, 5, 7) is rd
    one = torch.zeros(1, 1, 1, dtype=torch.uint8).to(device)
    assert _refused(lambda: ops.resize_nearest_u8(one, 65536, 1))
    assert _refused(lambda: ops.resize_nearest_u8(torch.zeros(65536, 1, 1, dtype=torch.uint8).to(device), 1, 2))
    return {"compared": n}


# =====================================================================================================================
# D. non-finite values reach the caller
# =====================================================================================================================
def _tiny_net(device, dtype):
    from dasr_amd import synth
    from tests.parity_checks import build_net
    net, _ = build_net(dict(scale=2, which=[0, 1, 2, 3], L=16, nb=4, B=1, H=8, W=12), device)
    net.set_compute_dtype(dtype)
    lq, gt, dm, mk = synth.closed_form_batch(2, 1, 8, 12, 2)
    soft = 0.7 * mk + 0.3 * synth.hash_uniform(mk.numel(), "soft").reshape(mk.shape).float()
    return net, [t.to(device) for t in (lq, gt, dm, soft)]


def _nan_bias_(net):
    with torch.no_grad():
        net.conv_output.bias[0] = float("nan")


def check_nan_bias_reaches_caller(device):
    """A diverged model must look diverged.  On the tiny x2 net of check_soft_masks_whole_net (scale 2, which = [0, 1, 2, 3],
    L = 16, nb = 4, 1 x 8 x 12), fp32 and bf16 activations, with and without autograd, conv_output.bias[0] = NaN: output
    plane 0 is NaN in every pixel and planes 1 and 2 hold none; one harness.Trainer step logs a non-finite pixel loss -
    eager, and on the MI355X also captured (three eager steps, the capture, one replay).
    (torch.clamp, the last operation of the reference's forward, keeps NaN; a clamp built on fmaxf / fminf returned ``lo``
    for it: plane 0 came back as exact zeros and the loss stayed finite.)"""
    from dasr_amd import harness
    n = 0
    for dtype in (torch.float32, BF16):
        for grad in (False, True):
            net, (lq, gt, dm, mk) = _tiny_net(device, dtype)
            _nan_bias_(net)
            with torch.set_grad_enabled(grad):
                sr = net(lq, dm, mk).detach().cpu()
            assert tuple(sr.shape) == (1, 3, 16, 24)
            assert bool(torch.isnan(sr[:, 0]).all()), ("NaN bias: plane 0", dtype, grad, int(torch.isnan(sr[:, 0]).sum()))
            assert not bool(torch.isnan(sr[:, 1:]).any()), ("NaN bias: planes 1, 2", dtype, grad)
            n += 1
        for use_graph in ((False, True) if device != "cpu" else (False,)):
            net, (lq, gt, dm, mk) = _tiny_net(device, dtype)
            _nan_bias_(net)
            tr = harness.Trainer(net, use_graph=use_graph)
            for _ in range(5 if use_graph else 1):
                log = tr.optimize_parameters(lq, gt, dm, mk)
            assert not use_graph or tr._graph is not None
            l_pix = float(log["l_pix"])
            assert not math.isfinite(l_pix), ("Trainer step with a NaN bias", dtype, use_graph, l_pix)
            n += 1
    return {"runs": n}


def check_nan_lr_pixel_reaches_caller(device):
    """The same net with one NaN LR pixel (lq[0, 1, 3, 5]): the output must contain NaN, as the reference's does (conv,
    LeakyReLU, instance norm, F.relu and torch.clamp all propagate it), fp32 and bf16 activations, with and without autograd.
    (With the clamp alone keeping NaN, 0 of 1152 outputs were NaN: the NaN spread as it should - 288 of conv1's outputs,
    every value of the head's feature map, of each block's instance-norm statistics and of the trunk - up to the ReLU that
    ends a residual block, where the SEAN forward kernels of csrc/sean.hip computed ``o > 0.f ? o : 0.f`` after adding the
    residual, which sends NaN to 0.  Every path from the LR image to the output crosses the ReLU that ends block nb - 1.
    They compute ``o <= 0.f ? 0.f : o`` now: NaN stays, every other input gives the same bits.)"""
    counts = {}
    for dtype in (torch.float32, BF16):
        for grad in (False, True):
            net, (lq, gt, dm, mk) = _tiny_net(device, dtype)
            lq = lq.clone()
            lq[0, 1, 3, 5] = float("nan")
            with torch.set_grad_enabled(grad):
                sr = net(lq, dm, mk).detach().cpu()
            counts["%s grad=%d" % (str(dtype).replace("torch.", ""), grad)] = (int(torch.isnan(sr).sum()), sr.numel())
    print("NaN outputs of one NaN LR pixel:", counts)
    assert all(c > 0 for c, _ in counts.values()), ("a NaN LR pixel left no NaN in the output", counts)
    return counts
