"""The small kernels around the convolutions at op level against float64, at the shapes where they leave the first tile, the
first loop trip or the first workgroup pass: csrc/dynk.hip, csrc/instnorm.hip, csrc/weights.hip, csrc/conv_c1.hip and
csrc/pool.hip.  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_small_kernels.py
runs every one of them on both.

Every reference is plain torch in float64 (einsum / F.conv2d / torch._weight_norm + autograd) on the same fp32 inputs (the
bf16 flavours: on the same bf16-rounded inputs); inputs come from a seeded torch.Generator on the CPU.  Each check also
computes the quantity with torch in fp32 and prints that error ("torch32") beside the kernel's: the reference's own fp32
error, printed and not gated."""
import torch
import torch.nn.functional as F

from dasr_amd import _lib, ops
from tests.parity_checks import rel_max

BF16 = torch.bfloat16
EPS32 = 1.19e-7

# (B, K, L, C): what each reaches is in check_dynk_shapes
DYNK_SHAPES = ((4, 16, 33, 64), (3, 11, 65, 36), (1, 1, 1, 4), (2, 10, 32, 11), (2, 3, 97, 43), (5, 10, 48, 20),
               (7, 10, 256, 8), (32, 10, 32, 64))
DYNK_NAMES = ("stp", "D", "dst", "dA_w", "dA_b", "dWg", "dWb")


def _fmt(errs):
    return " ".join("%s=%.2e" % kv for kv in errs.items())


def _worst(worst, errs):
    for nm, e in errs.items():
        worst[nm] = max(worst.get(nm, 0.0), e)


def dynk_inputs(B, K, L, C, seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return dict(st=rn(B, K, L), A_w=rn(K, K, 1, 1) * 0.3, A_b=rn(K) * 0.1, Wg=rn(C, L, 3, 3), Wb=rn(C, L, 3, 3),
                dD=rn(B, 2, 9, K, C), base=rn(B, K, L))


def dynk_reference(inp, dtype):
    """(stp, D, dst, dA_w, dA_b, dWg, dWb) of the two einsums and their autograd in ``dtype``."""
    B, K, L = inp["st"].shape
    C = inp["Wg"].shape[0]
    d = [inp[k].to(dtype).clone().requires_grad_(True) for k in ("st", "A_w", "A_b", "Wg", "Wb")]
    stp = d[2].reshape(1, K, 1) + torch.einsum("kj,bjl->bkl", d[1].reshape(K, K), d[0])
    W2 = torch.stack((d[3], d[4])).reshape(2, C, L, 9)
    D = torch.einsum("sclt,bkl->bstkc", W2, stp)
    D.backward(inp["dD"].to(dtype))
    return (stp.detach(), D.detach()) + tuple(x.grad for x in d)


def dynk_kernels(inp, device):
    """The same seven tensors from dasr_dynk_fwd / dasr_dynk_bwd; dst is what the backward ADDED to a random base."""
    dev = lambda k: inp[k].to(device)
    stp, D = ops.dynk_fwd(dev("st"), dev("A_w"), dev("A_b"), dev("Wg"), dev("Wb"))
    dst = dev("base").clone()
    dWg, dWb, dA_w, dA_b = ops.dynk_bwd(dev("dD"), dev("st"), stp, dev("A_w"), dev("Wg"), dev("Wb"), dst)
    added = (dst.double().cpu() - inp["base"].double()).float()
    return stp, D, added, dA_w, dA_b, dWg, dWb


def check_dynk_shapes(device):
    """dasr_dynk_fwd / dasr_dynk_bwd against float64 einsums, the gradient of the depth matrix added onto a random base.
    Gate: rel_max <= 1e-5 on each of stp, D, dst, dA_w, dA_b, dWg, dWb (the gate of check_dynk_odd_latent).  DYNK_SHAPES:
      (4, 16, 33, 64)   L = 1 (mod 32); M = 64 is two full M tiles; K = 16 is the soft-mask maximum
      (3, 11, 65, 36)   L = 1 and B*K = 33 = 1 (mod 32); ragged M tile; N = 648 is no multiple of 32
      (1, 1, 1, 4)      every bound equal to 1
      (2, 10, 32, 11), (2, 3, 97, 43)   3*C = 33 and 129 (the dstp contraction); C % 4 != 0
      (5, 10, 48, 20)   ragged M (50), ragged L trip (48), ragged N (360)
      (7, 10, 256, 8)   eight L trips; B*K = 70 is three K trips of dW
      (32, 10, 32, 64)  the batch-32 training shape: ten M tiles, B*K = 320 is ten full trips
    With the contraction loops started at the lane half (`for (l0 = lane >> 5; l0 < L; l0 += 32)`) the two halves of a wave
    made different trip counts at a bound of 32 n + 1: on the emulator D came out with rel_max 4.3 / 4.1 at L = 33 / 65,
    dWg / dWb with 4.0 / 4.3 at B*K = 33 and 1.0 / 0.73 at (1, 1, 1, 4), and the dstp kernel stopped at a divergent
    barrier at 3*C = 33 and 129.
    Measured worst rel_max, emulator: stp 1.3e-7, D 4.2e-7, dst 3.0e-7, dA_w 2.9e-7, dA_b 3.6e-7, dWg 6.5e-7, dWb 7.0e-7
    (torch's own fp32 einsum: <= 6.5e-7 away from (1, 1, 1, 4), 1.2e-5 there); MI355X: the same seven figures to two digits."""
    worst = {}
    for si, shape in enumerate(DYNK_SHAPES):
        inp = dynk_inputs(*shape, seed=710 + si)
        ref = dynk_reference(inp, torch.float64)
        t32 = dynk_reference(inp, torch.float32)
        got = dynk_kernels(inp, device)
        errs = {nm: rel_max(a, r) for nm, a, r in zip(DYNK_NAMES, got, ref)}
        own = {nm: rel_max(a, r) for nm, a, r in zip(DYNK_NAMES, t32, ref)}
        print("dynk (B,K,L,C)=%s: %s | torch32: %s" % (shape, _fmt(errs), _fmt(own)))
        assert max(errs.values()) <= 1e-5, (shape, errs)
        _worst(worst, errs)
    return worst


# (B, H, W, C, offset, std, dtypes): x = offset + std * randn; what each reaches is in check_instnorm_shapes
BOTH_DTYPES = (torch.float32, BF16)
INSTNORM_CASES = (
    (2, 25, 41, 64, 0.0, 1.0, BOTH_DTYPES),
    (2, 25, 41, 64, 100.0, 0.01, (torch.float32,)),
    (1, 12, 25, 6, 0.0, 1.0, BOTH_DTYPES),
    (1, 12, 25, 6, 50.0, 0.05, BOTH_DTYPES),
    (1, 16, 64, 3, 0.5, 0.2, BOTH_DTYPES),
    (1, 37, 7, 5, 10.0, 0.1, BOTH_DTYPES),
    (1, 1, 17411, 64, 3.0, 1.0, BOTH_DTYPES),
    (2, 1, 1, 64, 1.0, 1.0, BOTH_DTYPES),
    (1, 3, 343, 68, -20.0, 0.1, BOTH_DTYPES),
)


def check_instnorm_shapes(device):
    """ops.instnorm_stats (fp32 and bf16 storage) against the float64 mean and biased variance of the stored values.
    INSTNORM_CASES (B, H, W, C, offset, std):
      (2, 25, 41, 64, 0, 1)        HW = 1025: a one-pixel tail chunk
      (2, 25, 41, 64, 100, 0.01)   fp32 only (in bf16 the data collapse to a constant)
      (1, 12, 25, 6, 0, 1), (1, 12, 25, 6, 50, 0.05)   C % 4 != 0 (k_instnorm_partial_c1); HW = 300 is one full chunk of
                                   256 pixels and a tail of 44
      (1, 16, 64, 3, 0.5, 0.2), (1, 37, 7, 5, 10, 0.1)  the same kernel at C = 3 and C = 5
      (1, 1, 17411, 64, 3, 1)      18 chunks: the merge kernel's `k += 16` loop makes a second trip
      (2, 1, 1, 64, 1, 1)          HW = 1: the variance must be exactly 0
      (1, 3, 343, 68, -20, 0.1)    C = 68: a second channel block of which only the first quad is live
    Gates per (b, c), with mean and std the float64 statistics of the stored values:
      mean      |d| / (|mean| + std) <= 2e-6                        (check_conv_fwd_stats)
      variance  |d| / var <= 2e-5 + eps32 * |mean| / std            (eps32 = 1.19e-7)
    The first variance term is check_conv_fwd_stats' gate for centred data; the second is the floor of any fp32 method that
    stores partial means: each carries a rounding of eps * |mean|, which enters M2 through the differences of partial means,
    which are of order std.  A one-pass E[x^2] - mean^2 errs by about eps * (|mean| / std)^2: 12, 0.12 and 5e-3 at the
    ratios 1e4, 1e3 and 200 of these cases, far outside the gate.  A channel that holds one value (HW = 1) must come out
    with variance exactly 0.
    Measured worst variance error (and its share of the gate), emulator: ratio 1e4: 1.7e-4 (0.14); ratio 1e3: 3.0e-6 in
    fp32 (0.022), 1.7e-6 in bf16 (0.009, ratio 3.5e3 after rounding); ratio 200: 2.3e-6 (0.052); ratio 100: 4.2e-7; centred
    data <= 2.6e-7; mean <= 2.3e-7 (torch's own fp32 var: <= 6e-8, mean <= 1.7e-7); MI355X: ratio 1e4: 1.7e-4 (0.14);
    ratio 1e3: 3.0e-6 / 1.7e-6; ratio 200: 2.2e-6 (0.051); centred data <= 2.6e-7; mean <= 2.3e-7."""
    out = {}
    for ci, (B, H, W, C, off, std, dtypes) in enumerate(INSTNORM_CASES):
        gen = torch.Generator().manual_seed(720 + ci)
        x32 = off + std * torch.randn(B, H, W, C, generator=gen)
        for dt in dtypes:
            x = x32.to(dt)
            xd = x.double().reshape(B, H * W, C)
            mt, vt = xd.mean(1), xd.var(1, unbiased=False)
            st = vt.sqrt()
            mean, var = ops.instnorm_stats(x.to(device))
            assert mean.dtype == torch.float32 and var.dtype == torch.float32
            assert tuple(mean.shape) == (B, C) == tuple(var.shape)
            gm, gv = mean.double().cpu(), var.double().cpu()
            xf = x.float().reshape(B, H * W, C)
            tm, tv = xf.mean(1).double(), xf.var(1, unbiased=False).double()
            em = ((gm - mt).abs() / (mt.abs() + st)).max().item()
            tem = ((tm - mt).abs() / (mt.abs() + st)).max().item()
            const = vt == 0
            # a channel that holds one value: exactly 0, and out of the relative comparison
            assert bool((gv[const] == 0).all()), ("variance of a constant channel", (B, H, W, C, off, std), dt)
            if H * W == 1:
                assert bool(const.all())
            live = ~const
            ev = tev = margin = 0.0
            ratio = 0.0
            if bool(live.any()):
                gate = 2e-5 + EPS32 * mt[live].abs() / st[live]
                rv = (gv[live] - vt[live]).abs() / vt[live]
                ev, tev = rv.max().item(), ((tv[live] - vt[live]).abs() / vt[live]).max().item()
                margin = (rv / gate).max().item()
                ratio = (mt[live].abs() / st[live]).max().item()
            errs = {"mean": em, "var": ev, "var/gate": margin}
            print("instnorm %dx%dx%dx%d offset=%g std=%g %s (|mean|/std <= %.3g): %s | torch32: mean=%.2e var=%.2e" %
                  (B, H, W, C, off, std, str(dt).replace("torch.", ""), ratio, _fmt(errs), tem, tev))
            assert em <= 2e-6, ((B, H, W, C, off, std), dt, errs)
            assert margin <= 1.0, ((B, H, W, C, off, std), dt, errs)
            out[(B, H, W, C, off, std, str(dt))] = errs
    return out


# (dim 0 of v, dim 1 of v, k, transposed): v is [O, I, k, k], or [I, O, k, k] for a transposed convolution; the norm groups
# are the slices along dim 0 and R = dim 1 * k * k.  What each reaches is in check_weight_norm_shapes.
WEIGHT_SHAPES = ((3, 1280, 1, False), (3, 1281, 1, False), (2, 2816, 1, False), (2, 2817, 1, False), (4, 320, 3, False),
                 (5, 142, 3, False), (320, 3, 3, True), (5, 36, 9, False), (40, 5, 9, True))


def check_weight_norm_shapes(device):
    """ops.weight_pack + ops.weight_pack_bwd against float64 torch._weight_norm(v, g, 0) and its autograd, with a random
    HWIO dw and g = rand + 0.5.  WEIGHT_SHAPES (dim 0, dim 1, k, transposed):
      (3, 1280, 1, F), (3, 1281, 1, F)   R = 1280 / 1281: the last R of the backward's NR = 5 form, the first of NR = 11
      (2, 2816, 1, F), (2, 2817, 1, F)   R = 2816 / 2817: the last of NR = 11, the first of NR = 0 (two passes over memory)
      (4, 320, 3, F)                      R = 2880: NR = 0 with a 3x3 kernel
      (5, 142, 3, F)                      R = 1278
      (320, 3, 3, T)                      transposed: 320 norm groups of R = 27
      (5, 36, 9, F), (40, 5, 9, T)        9x9
    Both halves of the packed buffer (w[0] HWIO; w[1] viewed as [kh, kw, O, I] and transposed back), dv and dg: rel_max <=
    2e-5 (check_conv_variants' tolerance for v.grad / g.grad); with g = None dv is the permuted dw bit for bit.  (R = 1 is
    left out: dv is mathematically 0 there and both implementations return rounding noise.)
    Measured worst, emulator: w 1.0e-7, wT 1.0e-7, dv 1.3e-7, dg 1.8e-7 (torch fp32 itself <= 4.4e-7); MI355X:
    w 1.2e-7, wT 1.2e-7, dv 1.3e-7, dg 1.5e-7."""
    worst = {}
    for si, (n0, n1, k, tr) in enumerate(WEIGHT_SHAPES):
        gen = torch.Generator().manual_seed(730 + si)
        v = torch.randn(n0, n1, k, k, generator=gen)
        g = torch.rand(n0, 1, 1, 1, generator=gen) + 0.5
        I, O = (n0, n1) if tr else (n1, n0)
        dw = torch.randn(k, k, I, O, generator=gen)
        to_hwio = (lambda w: w.permute(2, 3, 0, 1)) if tr else (lambda w: w.permute(2, 3, 1, 0))

        def reference(dtype):
            vv, gg = v.to(dtype).requires_grad_(True), g.to(dtype).requires_grad_(True)
            w = to_hwio(torch._weight_norm(vv, gg, 0))
            (w * dw.to(dtype)).sum().backward()
            return w.detach(), vv.grad, gg.grad
        w_ref, dv_ref, dg_ref = reference(torch.float64)
        w_t32, dv_t32, dg_t32 = reference(torch.float32)
        vd, gd, dwd = v.to(device), g.to(device), dw.contiguous().to(device)
        w, inv = ops.weight_pack(vd, gd, tr)
        assert tuple(w.shape) == (2, k, k, I, O)
        dv, dg = ops.weight_pack_bwd(dwd, vd, gd, inv, tr)
        errs = {"w": rel_max(w[0], w_ref), "wT": rel_max(w[1].reshape(k, k, O, I).permute(0, 1, 3, 2), w_ref),
                "dv": rel_max(dv, dv_ref), "dg": rel_max(dg, dg_ref)}
        own = {"w": rel_max(w_t32, w_ref), "dv": rel_max(dv_t32, dv_ref), "dg": rel_max(dg_t32, dg_ref)}
        print("weight_norm v=%dx%dx%dx%d transposed=%d R=%d: %s | torch32: %s" %
              (n0, n1, k, k, tr, n1 * k * k, _fmt(errs), _fmt(own)))
        assert max(errs.values()) <= 2e-5, ((n0, n1, k, tr), errs)
        # no weight norm: the kernel is the permuted v, its gradient the permuted dw, bit for bit
        w0, inv0 = ops.weight_pack(vd, None, tr)
        assert inv0 is None and torch.equal(w0[0].cpu(), to_hwio(v))
        assert torch.equal(w0[1].reshape(k, k, O, I).permute(0, 1, 3, 2).cpu(), to_hwio(v))
        dv0, dg0 = ops.weight_pack_bwd(dwd, vd, None, None, tr)
        want = dw.permute(2, 3, 0, 1) if tr else dw.permute(3, 2, 0, 1)
        assert dg0 is None and torch.equal(dv0.cpu(), want), ("dv without weight norm", (n0, n1, k, tr))
        _worst(worst, errs)
    return worst


# (B, H, W, Cin, Cout, act): what each reaches is in check_c1_conv_shapes
C1_SHAPES = (
    (2, 300, 5, 1, 16, ops.ACT_RELU),
    (2, 520, 3, 1, 16, ops.ACT_RELU),
    (3, 700, 3, 1, 8, ops.ACT_LRELU),
    (1, 4, 150, 3, 32, ops.ACT_LRELU),
    (1, 9, 70, 3, 64, ops.ACT_LRELU),
    (1, 3, 37, 1, 128, ops.ACT_RELU),
    (1, 5, 9, 1, 1024, ops.ACT_RELU),
    (2, 6, 7, 3, 256, ops.ACT_NONE),
    (1, 2, 1, 1, 4, ops.ACT_RELU),
)


def _act(y, act):
    return F.relu(y) if act == ops.ACT_RELU else (F.leaky_relu(y, 0.2) if act == ops.ACT_LRELU else y)


def _c1_wgrad_reference(x, dy, y_saved, act, Cout, dtype):
    """dw (HWIO) and db of conv3x3(x) for the output gradient dy * act'(y_saved), in ``dtype``: the derivative is decided by
    the sign of the saved activation the kernel was given (1 where y > 0, else the slope: 0 / 0.2 / 1)."""
    slope = {ops.ACT_RELU: 0.0, ops.ACT_LRELU: 0.2, ops.ACT_NONE: 1.0}[act]
    dconv = dy.to(dtype) * torch.where(y_saved > 0, 1.0, slope).to(dtype)
    Cin = x.shape[3]
    wt = torch.zeros(Cout, Cin, 3, 3, dtype=dtype, requires_grad=True)
    bt = torch.zeros(Cout, dtype=dtype, requires_grad=True)
    yy = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), wt, bt, padding=1)
    gw, gb = torch.autograd.grad(yy, (wt, bt), dconv.permute(0, 3, 1, 2))
    return gw.permute(2, 3, 1, 0), gb


def check_c1_conv_shapes(device):
    """The 3x3 convolution of a 1- or 3-channel image (csrc/conv_c1.hip): ops.conv2d_fwd (fp32, and out_dtype = bfloat16)
    and ops.conv2d_wgrad_act (fp32 and bf16 dy / y) against float64 F.conv2d.  The activation derivative of the weight
    gradient is decided by the saved activation the kernel is given (the kernel's own forward output).  C1_SHAPES
    (B, H, W, Cin, Cout, act):
      (2, 300, 5, 1, 16, ReLU)    600 rows > the fp32 weight gradient's 512 workgroups: several rows per workgroup, the
                                  next row's loads prefetched
      (2, 520, 3, 1, 16, ReLU)    1040 rows > the bf16 weight gradient's 1024 workgroups
      (3, 700, 3, 1, 8, LReLU)    2100 rows > the forward's 2048 workgroups
      (1, 4, 150, 3, 32, LReLU)   W past one trip of NPX * npl pixels
      (1, 9, 70, 3, 64, LReLU)
      (1, 3, 37, 1, 128, ReLU)
      (1, 5, 9, 1, 1024, ReLU)    nq = 256: one pixel lane
      (2, 6, 7, 3, 256, none)     HASY = false
      (1, 2, 1, 1, 4, ReLU)       W = 1
    Gates: fp32 y, dw, db rel_max <= 2e-5 (check_conv_variants for Cin * k * k < 600); bf16 y within 2^-8 of the largest
    value; dw / db from bf16 dy / y against float64 of the same rounded operands <= 1e-5 (check_bf16_conv_variants).
    dasr_conv2d_wgrad_act_fused is asserted for every shape (the fused kernel, not epilogue + generic weight gradient).
    Measured worst, emulator: y 1.7e-7, dw 1.0e-6, db 4.7e-7, y_bf16 3.3e-3, dw_bf16 7.2e-7, db_bf16 2.9e-7 (torch fp32
    itself <= 7.0e-7); MI355X (the sums meet in float atomics; one run): y 1.7e-7, dw 7.2e-7,
    db 6.6e-7, y_bf16 3.3e-3, dw_bf16 1.5e-6, db_bf16 2.8e-7."""
    worst = {}
    lib = _lib.get()
    for si, (B, H, W, Cin, Cout, act) in enumerate(C1_SHAPES):
        gen = torch.Generator().manual_seed(740 + si)
        rn = lambda *s: torch.randn(*s, generator=gen)
        x, w, bias, dy = rn(B, H, W, Cin), rn(3, 3, Cin, Cout) * 0.4, rn(Cout) * 0.2, rn(B, H, W, Cout)
        assert lib.dasr_conv2d_wgrad_act_fused(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, 0) == 1, (B, H, W, Cin, Cout)

        def forward(dtype):
            y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(3, 2, 0, 1), bias.to(dtype), padding=1)
            return _act(y, act).permute(0, 2, 3, 1)
        y_ref, y_t32 = forward(torch.float64), forward(torch.float32)
        xd, wp, bd = x.to(device), ops.pack_hwio(w.to(device)), bias.to(device)
        # ---- fp32
        y = ops.conv2d_fwd(xd, wp, bd, act=act)
        assert y.dtype == torch.float32 and tuple(y.shape) == (B, H, W, Cout)
        dw, db = ops.conv2d_wgrad_act(xd, dy.to(device), y, (3, 3, Cin, Cout), act)
        dw_ref, db_ref = _c1_wgrad_reference(x, dy, y.cpu(), act, Cout, torch.float64)
        dw_t32, db_t32 = _c1_wgrad_reference(x, dy, y.cpu(), act, Cout, torch.float32)
        errs = {"y": rel_max(y, y_ref), "dw": rel_max(dw, dw_ref), "db": rel_max(db, db_ref)}
        own = {"y": rel_max(y_t32, y_ref), "dw": rel_max(dw_t32, dw_ref), "db": rel_max(db_t32, db_ref)}
        # ---- bf16 activation out; bf16 dy and saved activation in
        y16 = ops.conv2d_fwd(xd, wp, bd, act=act, out_dtype=BF16)
        assert y16.dtype == BF16 and tuple(y16.shape) == (B, H, W, Cout)
        dy16 = dy.to(BF16)
        dw16, db16 = ops.conv2d_wgrad_act(xd, dy16.to(device), y16, (3, 3, Cin, Cout), act)
        assert dw16.dtype == torch.float32 and db16.dtype == torch.float32
        dw16_ref, db16_ref = _c1_wgrad_reference(x, dy16.float(), y16.float().cpu(), act, Cout, torch.float64)
        errs.update({"y_bf16": rel_max(y16.float(), y_ref), "dw_bf16": rel_max(dw16, dw16_ref),
                     "db_bf16": rel_max(db16, db16_ref)})
        print("c1 conv %dx%dx%d %d->%d act=%d: %s | torch32: %s" % (B, H, W, Cin, Cout, act, _fmt(errs), _fmt(own)))
        assert max(errs["y"], errs["dw"], errs["db"]) <= 2e-5, ((B, H, W, Cin, Cout, act), errs)
        assert errs["y_bf16"] <= 2.0 ** -8, ((B, H, W, Cin, Cout, act), errs)
        assert max(errs["dw_bf16"], errs["db_bf16"]) <= 1e-5, ((B, H, W, Cin, Cout, act), errs)
        _worst(worst, errs)
    return worst


# (B, K, L, h, w, H, W): what each reaches is in check_region_pool_shapes
POOL_SHAPES = ((2, 10, 256, 9, 7, 9, 7), (1, 16, 48, 5, 6, 17, 21), (3, 7, 33, 1, 1, 4, 4), (2, 10, 32, 16, 20, 128, 160),
               (1, 10, 5, 17, 3, 17, 3))


def check_region_pool_shapes(device):
    """ops.region_pool_fwd / ops.region_pool_bwd on one-hot-or-empty planes made of random region integers 0 .. K (K =
    unclaimed).  POOL_SHAPES (B, K, L, h, w, H, W):
      (2, 10, 256, 9, 7, 9, 7)         same size (the mask is copied); hw = 63 is a ragged 16-pixel trip; L = 256
      (1, 16, 48, 5, 6, 17, 21)        x4 in both directions
      (3, 7, 33, 1, 1, 4, 4)           h = w = 1: the `out == 1` scale of align_corners; six of seven regions empty per sample
      (2, 10, 32, 16, 20, 128, 160)    the x8 ratio of the mask to the e5 feature map
      (1, 10, 5, 17, 3, 17, 3)
    maskr must equal F.interpolate(mask, (h, w), mode="bilinear", align_corners=True) >= 0.5 bit for bit - a condition on
    the inputs is asserted first: no float64-interpolated value lies within 1e-6 of 0.5 (none does with these seeds).  At
    least one case contains empty regions, whose pooled row must be exactly 0.  out and dfeat against float64 at that
    maskr: rel_max <= 2e-6 (check_region_pool's gate).
    Measured worst, emulator: out 1.9e-7, dfeat 3.6e-8, 22 empty regions (3 at 5x6, 19 at 1x1) (torch fp32 itself <=
    1.9e-7); MI355X: the same."""
    worst = {}
    n_empty = 0
    for si, (B, K, L, h, w, H, W) in enumerate(POOL_SHAPES):
        gen = torch.Generator().manual_seed(750 + si)
        r = torch.randint(0, K + 1, (B, H, W), generator=gen)
        mask = F.one_hot(r, K + 1)[..., :K].permute(0, 3, 1, 2).float().contiguous()
        feat, dout = torch.randn(B, h, w, L, generator=gen), torch.randn(B, K, L, generator=gen)
        v64 = F.interpolate(mask.double(), (h, w), mode="bilinear", align_corners=True)
        near = int(((v64 - 0.5).abs() < 1e-6).sum())
        assert near == 0, ("input condition: interpolated mask values at the 0.5 threshold", (B, K, L, h, w, H, W), near)
        want = (F.interpolate(mask, (h, w), mode="bilinear", align_corners=True) >= 0.5).float()
        assert torch.equal(want, (v64 >= 0.5).float())
        out, maskr, area = ops.region_pool_fwd(feat.to(device), mask.to(device))
        assert torch.equal(maskr.cpu(), want), ("maskr", (B, K, L, h, w, H, W))
        assert torch.equal(area.cpu(), want.sum((2, 3))), ("area", (B, K, L, h, w, H, W))
        dfeat = ops.region_pool_bwd(dout.to(device), maskr, area, feat.shape)

        def reference(dtype):
            m = want.to(dtype).reshape(B, K, h * w)
            inv = 1.0 / (m.sum(2) + 1e-10)
            o = torch.einsum("bkp,bpl->bkl", m, feat.to(dtype).reshape(B, h * w, L)) * inv[..., None]
            df = torch.einsum("bkp,bkl->bpl", m, dout.to(dtype) * inv[..., None]).reshape(B, h, w, L)
            return o, df
        (o_ref, df_ref), (o_t32, df_t32) = reference(torch.float64), reference(torch.float32)
        empty = want.sum((2, 3)) == 0
        n_empty += int(empty.sum())
        assert bool((out.cpu()[empty] == 0).all()), ("pooled row of an empty region", (B, K, L, h, w, H, W))
        errs = {"out": rel_max(out, o_ref), "dfeat": rel_max(dfeat, df_ref)}
        own = {"out": rel_max(o_t32, o_ref), "dfeat": rel_max(df_t32, df_ref)}
        print("region_pool (B,K,L,h,w,H,W)=%s empty=%d near-0.5=%d: %s | torch32: %s" %
              ((B, K, L, h, w, H, W), int(empty.sum()), near, _fmt(errs), _fmt(own)))
        assert max(errs.values()) <= 2e-6, ((B, K, L, h, w, H, W), errs)
        _worst(worst, errs)
    assert n_empty > 0
    worst["empty_regions"] = n_empty
    return worst
