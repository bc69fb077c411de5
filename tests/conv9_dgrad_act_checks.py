"""Checks of the 9x9 fp16 x 2 split dgrad with the producer's activation / PixelShuffle(2) backward in its epilogue
(k_conv9_dgrad_split<true>, dasr_conv9_dgrad_act_split2, csrc/conv9_split.hip) and of the plain form that shares its source.
The kernel walks 8 x 16 pixel tiles with 256 threads, wave w on tile rows 2w, 2w+1; what can go wrong is the pixel map of the
2 x 16 M-tile, the swizzled LDS images, a ragged tile row or column, the un-shuffle address, the sign read from x_act at
zeros, the maximum a workgroup leaves behind, and - `impl & 3 == 2`, three workgroups - the persistent loop with the next
tile's loads in flight.  Per case:
  * check_bits: the fused launch EQUALS dasr_conv2d_epilogue_bwd of the plain dgrad (the K order per element is the same and
    the epilogue only multiplies by a power of two and by 1 / 0.2 / 0), max |dprev| is exact, word 0 of the amax buffer is
    the launched workgroup count;
  * check_float64: against torch's float64 convolution gradient, derivative and pixel_unshuffle, the gate of
    check_conv9_split (error <= 1.25x the exact-fp32 kernels' + 1e-7 on the hardware, 3x + 2e-7 on the emulator);
  * check_plain (cases a, d): the plain and the accumulating dgrad under the same gates.
check_refused: odd H, ps_r = 3 and Cin = 64 are refused.  check_net: the whole x8 net, one training backward with
graph.FUSE_C9_DGRAD_ACT on and one with it off.
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_conv9_dgrad_act.py runs them."""
import functools

import torch
import torch.nn.functional as F

from dasr_amd import ops, synth
from tests.parity_checks import ZERO_GRAD_KEYS, build_net, nchw, nhwc

F64 = torch.float64
CIN = 32
_A = dict(B=2, H=18, W=36, cout=3)          # two full tile rows plus a ragged one, a ragged tile column, two samples
CASES = {
    "a": dict(_A, impl=0, act=ops.ACT_LRELU),
    "b": dict(B=1, H=10, W=66, cout=3, impl=0, act=ops.ACT_LRELU),      # one ragged tile row, many tile columns
    "c": dict(B=1, H=12, W=34, cout=1, impl=0, act=ops.ACT_LRELU),
    "d": dict(_A, impl=2, act=ops.ACT_LRELU),                           # three workgroups, six tiles each
    "e-lrelu": dict(_A, impl=0, act=ops.ACT_LRELU, zeros=True, sd=2e-6, sx=37.0),
    "e-relu": dict(_A, impl=0, act=ops.ACT_RELU, zeros=True, sd=2e-6, sx=37.0),
}
CHECKS = ("check_bits", "check_float64")
PLAIN_CASES = ("a", "d")


def launched_workgroups(case):
    """Tiles of 8 x 16 pixels; a persistent grid of at most two workgroups per CU (512), three under `impl & 3 == 2`."""
    c = CASES[case]
    tiles = c["B"] * ((c["H"] + 7) // 8) * ((c["W"] + 15) // 16)
    return min(tiles, 3 if c["impl"] & 3 == 2 else 512)


def act_grad(x_act, act):
    neg = {ops.ACT_RELU: 0.0, ops.ACT_LRELU: 0.2, ops.ACT_NONE: 1.0}[act]
    return torch.where(x_act > 0, torch.ones_like(x_act), torch.full_like(x_act, neg))


@functools.lru_cache(maxsize=None)
def _operands(case):
    """CPU operands (NCHW fp32: x_act, w, dy, base) and the float64 references (dx [B,Cin,H,W], dprev [B,H/2,W/2,4Cin]),
    once per case."""
    c = CASES[case]
    B, H, W, cout = c["B"], c["H"], c["W"], c["cout"]
    gen = torch.Generator().manual_seed(40 + H + W + cout)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x_act = rn(B, CIN, H, W) * c.get("sx", 1.0)
    w = rn(cout, CIN, 9, 9) * 0.02
    dy = rn(B, cout, H, W) * c.get("sd", 1.0)
    base = rn(B, H, W, CIN) * c.get("sd", 1.0)
    if c.get("zeros"):
        u = torch.rand(x_act.shape, generator=gen)
        x_act = torch.where(u < 0.15, torch.zeros_like(x_act), x_act)
        x_act = torch.where((u >= 0.15) & (u < 0.3), -torch.zeros_like(x_act), x_act)
        assert int((x_act == 0).sum()) > 100 and bool(torch.signbit(x_act[x_act == 0]).any())
    x64 = x_act.double().requires_grad_(True)
    ref = F.conv2d(x64, w.double(), None, padding=4)
    dx64, = torch.autograd.grad(ref, (x64,), dy.double())
    dprev64 = nhwc(F.pixel_unshuffle(dx64 * act_grad(x_act, c["act"]).double(), 2))
    return x_act, w, dy, base, dx64, dprev64


_runs = {}


def _run(device, case):
    """The launches of one (device, case), once: the plain split dgrad, the epilogue backward of its result, the fused
    launch and its amax buffer, the exact-fp32 pair."""
    key = (device, case)
    if key in _runs:
        return _runs[key]
    c = CASES[case]
    x_act, w, dy, _, _, _ = _operands(case)
    B, H, W = c["B"], c["H"], c["W"]
    xd, dyd = nhwc(x_act).to(device), nhwc(dy).to(device)
    wp = ops.pack_hwio(w.permute(2, 3, 1, 0).contiguous().to(device))
    wm, dm = ops.absmax(wp[0]), ops.absmax(dyd)
    ops.set_conv_bf16_impl(c["impl"])
    try:
        assert ops.conv9_dgrad_act_supported(xd.shape, c["cout"], c["act"], 2)
        dx = ops.conv9_dgrad_split2(dyd, dm, wp, wm, xd.shape)
        two = ops.conv2d_epilogue_bwd(dx, xd, H // 2, W // 2, 4 * CIN, c["act"], 2)
        buf = ops.amax_buffer(xd).fill_(float("nan"))          # (poisoned: the kernel must write every word it declares)
        fused = ops.conv9_dgrad_act_split2(dyd, dm, wp, wm, xd, c["act"], 2, amax=buf)
        dx32 = ops.conv2d_dgrad(dyd, wp, xd.shape, pad=4)
        two32 = ops.conv2d_epilogue_bwd(dx32, xd, H // 2, W // 2, 4 * CIN, c["act"], 2)
    finally:
        ops.set_conv_bf16_impl(0)
    out = dict(dx=dx.cpu(), two=two.cpu(), fused=fused.cpu(), buf=buf.cpu(), dx32=dx32.cpu(), two32=two32.cpu(),
               tagged=ops.get_amax(fused) is buf, ops=(xd, dyd, wp, wm, dm))
    return _runs.setdefault(key, out)


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def check_bits(device, case):
    r = _run(device, case)
    fused, two = r["fused"], r["two"]
    assert fused.shape == two.shape == (CASES[case]["B"], CASES[case]["H"] // 2, CASES[case]["W"] // 2, 4 * CIN)
    bad = fused != two
    assert torch.equal(fused, two), ("fused differs from dgrad + epilogue backward", case, int(bad.sum()), bad.nonzero()[:4].tolist())
    assert r["tagged"], "the result does not carry its amax buffer"
    n = int(r["buf"][:1].view(torch.int32).item())
    assert n == launched_workgroups(case), ("amax word 0", n, launched_workgroups(case))
    assert not bool(torch.isnan(r["buf"][1:1 + n]).any()), "a workgroup left its word unwritten"
    got, want = ops.amax_value(r["buf"]), fused.abs().max().item()
    assert got == want, ("max |dprev|", case, got, want)
    return dict(workgroups=n, amax=got)


def check_float64(device, case):
    r = _run(device, case)
    dprev64 = _operands(case)[5]
    fac, slack = (3.0, 2e-7) if device == "cpu" else (1.25, 1e-7)
    e_sp, e_32 = _rel(r["fused"], dprev64), _rel(r["two32"], dprev64)
    print("%s %s: fused split %.3g, exact fp32 %.3g" % (case, device, e_sp, e_32))
    assert e_sp <= fac * e_32 + slack, ("conv9 dgrad + act", case, e_sp, e_32)
    return dict(split=e_sp, fp32=e_32)


def check_plain(device, case):
    """The plain and the accumulating dgrad (same kernel source, FUSE = false) under check_conv9_split's gates."""
    r = _run(device, case)
    c = CASES[case]
    _, _, _, base, dx64, _ = _operands(case)
    fac, slack = (3.0, 2e-7) if device == "cpu" else (1.25, 1e-7)
    g_sp, g_32 = _rel(nchw(r["dx"]), dx64), _rel(nchw(r["dx32"]), dx64)
    print("%s %s: plain split %.3g, exact fp32 %.3g" % (case, device, g_sp, g_32))
    assert g_sp <= fac * g_32 + slack, ("conv9 dgrad", case, g_sp, g_32)
    xd, dyd, wp, wm, dm = r["ops"]
    accd = base.to(device).clone()
    ops.set_conv_bf16_impl(c["impl"])
    try:
        ops.conv9_dgrad_split2(dyd, dm, wp, wm, xd.shape, out=accd)
    finally:
        ops.set_conv_bf16_impl(0)
    want = nhwc(dx64) + base.double()
    g_acc = _rel(accd.cpu(), want)
    assert g_acc <= fac * g_32 + 2 * slack, ("conv9 dgrad accumulate", case, g_acc, g_32)
    return dict(split=g_sp, fp32=g_32, accumulate=g_acc)


def check_refused(device):
    z = lambda *s: torch.zeros(*s).to(device)
    wp = ops.pack_hwio(z(9, 9, 32, 3))
    wm = ops.absmax(wp[0])

    def refused(H, W, cin, ps_r, w=wp):
        dy = z(1, H, W, 3)
        try:
            ops.conv9_dgrad_act_split2(dy, ops.absmax(dy), w, wm, z(1, H, W, cin), ops.ACT_LRELU, ps_r)
        except RuntimeError:
            return True
        return False

    assert not refused(16, 16, 32, 2)
    assert refused(17, 16, 32, 2), "odd H"
    assert refused(16, 17, 32, 2), "odd W"
    assert refused(18, 18, 32, 3), "ps_r = 3"
    assert refused(16, 16, 64, 2, ops.pack_hwio(z(9, 9, 64, 3))), "Cin = 64"
    assert not ops.conv9_dgrad_act_supported((1, 17, 16, 32), 3, ops.ACT_LRELU, 2)
    assert not ops.conv9_dgrad_act_supported((1, 18, 18, 32), 3, ops.ACT_LRELU, 3)
    assert not ops.conv9_dgrad_act_supported((1, 16, 16, 64), 3, ops.ACT_LRELU, 2)
    return True


NET_CASE = dict(name="c9_dgrad_act", scale=8, which=[0, 1], L=32, nb=4, B=2, H=8, W=12)


def check_net(device, monkeypatch):
    """x8, nb = 4, two DGBs, LR 8 x 12, B = 2, every split convolution forced on: one training backward with the fused 9x9
    dgrad and one without, from the same inputs.  The fused op runs once and replaces one epilogue-backward pass; what it
    hands to upscale3's weight gradient is bit-equal to that pass's result; the parameter gradients are bit-equal on the
    emulator and within 1e-5 (relative, per tensor) on the GPU, whose bias / SEAN gradients end in float atomics.
    That bound is the project's summation-order bound and is kept as it is; it is close to the noise of this net.  upscale3's
    dconv is bit-equal, so everything behind it runs the same launches on the same bits in both runs and what is compared
    is two runs' atomics order.  Worst tensor over three GPU runs: 4.4e-7, 1.2e-6 and 1.02e-5 - the last one a miss, on the
    scalar depth-residual1.norm1.alpha_beta (one sum of dbeta * (beta1 - beta2) over the whole tensor, cancelling)."""
    from dasr_amd import graph
    monkeypatch.setattr(graph, "SPLIT_MIN_PIXELS", 0)
    net, cfg = build_net(NET_CASE, device)
    lq, gt, dm, mk = [t.to(device) for t in synth.closed_form_batch(0, NET_CASE["B"], NET_CASE["H"], NET_CASE["W"], cfg["scale"])]
    hr = (NET_CASE["B"], NET_CASE["H"] * 8 // 2, NET_CASE["W"] * 8 // 2, 4 * CIN)       # upscale3's dconv
    orig_fused, orig_epi = ops.conv9_dgrad_act_split2, ops.conv2d_epilogue_bwd
    res = {}
    for on in (True, False):
        monkeypatch.setattr(graph, "FUSE_C9_DGRAD_ACT", on)
        calls = dict(fused=0, epi=0, dconv=None)

        def fused(*a, _c=calls, **k):
            _c["fused"] += 1
            out = orig_fused(*a, **k)
            _c["dconv"] = out.detach().clone()
            return out

        def epi(*a, _c=calls, **k):
            _c["epi"] += 1
            out = orig_epi(*a, **k)
            if tuple(out.shape) == hr:
                assert _c["dconv"] is None
                _c["dconv"] = out.detach().clone()
            return out

        monkeypatch.setattr(ops, "conv9_dgrad_act_split2", fused)
        monkeypatch.setattr(ops, "conv2d_epilogue_bwd", epi)
        net.zero_grad(set_to_none=True)
        sr = net(lq, dm, mk)
        wgt = torch.cos(torch.arange(sr.numel(), dtype=torch.float32) * 0.013).reshape(sr.shape).to(device)
        (sr * wgt).sum().backward()
        res[on] = (calls, {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    (c_on, g_on), (c_off, g_off) = res[True], res[False]
    assert c_on["fused"] == 1 and c_off["fused"] == 0, (c_on, c_off)
    assert c_on["epi"] == c_off["epi"] - 1, (c_on["epi"], c_off["epi"])
    assert tuple(c_on["dconv"].shape) == hr and torch.equal(c_on["dconv"], c_off["dconv"]), "upscale3's dconv differs"
    assert g_on.keys() == g_off.keys()
    worst = 0.0
    for k, g in g_off.items():
        if device == "cpu":
            assert torch.equal(g_on[k], g), ("gradient differs", k)
        else:
            d = (g_on[k] - g).double().norm().item() / max(g.double().norm().item(), 1e-30)
            worst = max(worst, 0.0 if any(z in k for z in ZERO_GRAD_KEYS) else d)
            if d > 1e-6:
                print("gradient on / off: %s %.3g" % (k, d))
            assert d <= 1e-5 or any(z in k for z in ZERO_GRAD_KEYS), ("gradient differs", k, d)
    return dict(epilogue_bwd_on=c_on["epi"], epilogue_bwd_off=c_off["epi"], worst_rel=worst)
