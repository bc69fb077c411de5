"""Checks of the fp16 x 2 split 3x3 dgrad with the producer's activation / PixelShuffle(2) backward in its epilogue
(k_conv3x3_split_n32<2, 1, true>, dasr_conv3x3_dgrad_act_split2, csrc/conv_split_bf16.hip) and of the plain 32-produced-channel dgrad
that shares its item loop.  The kernel walks 16 x 32 pixel tiles with 512 threads, wave w on tile rows 2w, 2w + 1; what can
go wrong is the lane map of the two epilogue forms, a ragged tile row or column, the un-shuffle address, the derivative
applied before instead of after the accumulation, the sign read from x_act at zeros, the maximum a workgroup leaves behind
and - `impl & 3 == 2`, one workgroup per XCD - the persistent loop with the next item's loads in flight.  Per case:
  * check_bits: the fused launch EQUALS dasr_conv2d_epilogue_bwd of dasr_conv3x3_dgrad_split2 (flat-acc: of its accumulating
    form), max |dprev| is exact, word 0 of the amax buffer is the launched workgroup count;
  * check_float64: against torch's float64 convolution gradient x derivative (+ pixel_unshuffle), the gate of
    parity_checks.check_split_conv (error <= 1.25x the exact-fp32 kernels' + 1e-7 on the hardware, 3x + 2e-7 on the emulator;
    accumulating: + twice the slack).
check_plain_unchanged: the plain dgrad's bits on the flat and flat-walk shapes are those of the build before the fused
kernel existed (emulator: digests in tests/golden/split_dgrad_plain_digests.json, recorded with plain_digests() from that
commit).  check_refused, check_net: see there.
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_split_dgrad_act.py runs them."""
import functools
import hashlib
import json
import os

import torch
import torch.nn.functional as F

from dasr_amd import ops, synth
from tests.parity_checks import build_net, nchw, nhwc

CIN = 32                                    # produced channels of the dgrad = the layer's input channels
_S = dict(B=2, H=18, W=36, cout=32, impl=0, ps=1)     # a full tile row plus a ragged one, a ragged tile column, two samples
_W = dict(B=3, H=34, W=66, cout=32, impl=2)           # 27 items on 8 workgroups: each walks 3-4
CASES = {
    "flat-lrelu": dict(_S, act=ops.ACT_LRELU),
    "flat-relu": dict(_S, act=ops.ACT_RELU),
    "flat-wide-lrelu": dict(_S, cout=128, act=ops.ACT_LRELU),
    "flat-wide-relu": dict(_S, cout=128, act=ops.ACT_RELU),
    "flat-acc": dict(_S, act=ops.ACT_LRELU, acc=True),
    "flat-walk": dict(_W, ps=1, act=ops.ACT_LRELU),
    "ps": dict(_S, ps=2, act=ops.ACT_LRELU),
    "ps-walk": dict(_W, ps=2, act=ops.ACT_LRELU),
    "zeros-flat-lrelu": dict(_S, act=ops.ACT_LRELU, zeros=True, sd=2e-6, sx=37.0),
    "zeros-flat-relu": dict(_S, act=ops.ACT_RELU, zeros=True, sd=2e-6, sx=37.0),
    "zeros-ps-lrelu": dict(_S, ps=2, act=ops.ACT_LRELU, zeros=True, sd=2e-6, sx=37.0),
    "zeros-ps-relu": dict(_S, ps=2, act=ops.ACT_RELU, zeros=True, sd=2e-6, sx=37.0),
}
CHECKS = ("check_bits", "check_float64")
PLAIN_CASES = ("flat-lrelu", "flat-walk")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_dgrad_plain_digests.json")


def launched_workgroups(case):
    """Items of 16 x 32 pixels x 32 channels, an eighth of them (Q) per XCD; 8 x min(Q, 32) workgroups, 8 under `impl & 3 == 2`."""
    c = CASES[case]
    items = c["B"] * ((c["H"] + 15) // 16) * ((c["W"] + 31) // 32)
    return 8 if c["impl"] & 3 == 2 else 8 * min((items + 7) // 8, 32)


def act_grad(x_act, act):
    neg = {ops.ACT_RELU: 0.0, ops.ACT_LRELU: 0.2, ops.ACT_NONE: 1.0}[act]
    return torch.where(x_act > 0, torch.ones_like(x_act), torch.full_like(x_act, neg))


@functools.lru_cache(maxsize=None)
def _operands(case):
    """CPU operands (NCHW fp32: x_act, w, dy; NHWC base) and the float64 reference dprev (NHWC; flat-acc: derivative applied
    to dgrad + base), once per case."""
    c = CASES[case]
    B, H, W, cout = c["B"], c["H"], c["W"], c["cout"]
    gen = torch.Generator().manual_seed(40 + H + W + cout)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x_act = rn(B, CIN, H, W) * c.get("sx", 1.0)
    w = rn(cout, CIN, 3, 3) * 0.02
    dy = rn(B, cout, H, W) * c.get("sd", 1.0)
    base = rn(B, H, W, CIN) * c.get("sd", 1.0)
    if c.get("zeros"):
        u = torch.rand(x_act.shape, generator=gen)
        x_act = torch.where(u < 0.15, torch.zeros_like(x_act), x_act)
        x_act = torch.where((u >= 0.15) & (u < 0.3), -torch.zeros_like(x_act), x_act)
        assert int((x_act == 0).sum()) > 100 and bool(torch.signbit(x_act[x_act == 0]).any())
    x64 = x_act.double().requires_grad_(True)
    ref = F.conv2d(x64, w.double(), None, padding=1)
    dx64, = torch.autograd.grad(ref, (x64,), dy.double())
    if c.get("acc"):
        dx64 = dx64 + nchw(base).double()
    d64 = dx64 * act_grad(x_act, c["act"]).double()
    dprev64 = nhwc(F.pixel_unshuffle(d64, 2)) if c["ps"] == 2 else nhwc(d64)
    return x_act, w, dy, base, dprev64


_runs = {}


def _run(device, case):
    """The launches of one (device, case), once: the plain split dgrad (flat-acc: onto the base), the epilogue backward of its
    result, the fused launch and its amax buffer, the exact-fp32 pair."""
    key = (device, case)
    if key in _runs:
        return _runs[key]
    c = CASES[case]
    x_act, w, dy, base, _ = _operands(case)
    B, H, W, r = c["B"], c["H"], c["W"], c["ps"]
    acc = bool(c.get("acc"))
    xd, dyd = nhwc(x_act).to(device), nhwc(dy).to(device)
    wp = ops.pack_hwio(w.permute(2, 3, 1, 0).contiguous().to(device))
    ws = ops.conv3x3_split2_weights(wp)
    dm = ops.absmax(dyd)
    oshape = (B, H // r, W // r, r * r * CIN)
    ops.set_conv_bf16_impl(c["impl"])
    try:
        assert ops.conv3x3_dgrad_act_supported(xd.shape, c["cout"], c["act"], r, acc)
        dx = ops.conv3x3_dgrad_split2(dyd, dm, ws, xd.shape, out=base.to(device).clone() if acc else None)
        two = ops.conv2d_epilogue_bwd(dx, xd, oshape[1], oshape[2], oshape[3], c["act"], r)
        buf = ops.amax_buffer(xd).fill_(float("nan"))          # (poisoned: the kernel must write every word it declares)
        fused = ops.conv3x3_dgrad_act_split2(dyd, dm, ws, xd, c["act"], r, out=base.to(device).clone() if acc else None, amax=buf)
        dx32 = ops.conv2d_dgrad(dyd, wp, xd.shape, out=base.to(device).clone() if acc else None)
        two32 = ops.conv2d_epilogue_bwd(dx32, xd, oshape[1], oshape[2], oshape[3], c["act"], r)
    finally:
        ops.set_conv_bf16_impl(0)
    out = dict(dx=dx.cpu(), two=two.cpu(), fused=fused.cpu(), buf=buf.cpu(), two32=two32.cpu(), oshape=oshape,
               tagged=ops.get_amax(fused) is buf)
    return _runs.setdefault(key, out)


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def check_bits(device, case):
    r = _run(device, case)
    fused, two = r["fused"], r["two"]
    assert tuple(fused.shape) == tuple(two.shape) == r["oshape"]
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
    dprev64 = _operands(case)[4]
    fac, slack = (3.0, 2e-7) if device == "cpu" else (1.25, 1e-7)
    if CASES[case].get("acc"):
        slack *= 2
    e_sp, e_32 = _rel(r["fused"], dprev64), _rel(r["two32"], dprev64)
    print("%s %s: fused split %.3g, exact fp32 %.3g" % (case, device, e_sp, e_32))
    assert e_sp <= fac * e_32 + slack, ("3x3 dgrad + act", case, e_sp, e_32)
    return dict(split=e_sp, fp32=e_32)


def plain_digests(device):
    """sha256 of the plain dgrad's result on the flat and flat-walk shapes (uses nothing the parent build lacks)."""
    out = {}
    for case in PLAIN_CASES:
        c = CASES[case]
        x_act, w, dy, _, _ = _operands(case)
        dyd = nhwc(dy).to(device)
        ws = ops.conv3x3_split2_weights(ops.pack_hwio(w.permute(2, 3, 1, 0).contiguous().to(device)))
        ops.set_conv_bf16_impl(c["impl"])
        try:
            dx = ops.conv3x3_dgrad_split2(dyd, ops.absmax(dyd), ws, tuple(nhwc(x_act).shape))
        finally:
            ops.set_conv_bf16_impl(0)
        out[case] = hashlib.sha256(dx.cpu().contiguous().numpy().tobytes()).hexdigest()
    return out


def check_plain_unchanged(device):
    """The plain path is the same instruction stream as before the fused kernel: same bits, pinned by digests recorded from
    the parent commit with plain_digests() - on the kernel emulator and on the MI355X."""
    got = plain_digests(device)
    want = json.load(open(GOLDEN))["emulator" if device == "cpu" else "gfx950"]
    assert got == want, ("plain dgrad bits changed", got, want)
    return got


def check_refused(device):
    z = lambda *s: torch.zeros(*s).to(device)

    def refused(H, W, cin, cout, ps_r, acc=False):
        ws = ops.conv3x3_split2_weights(ops.pack_hwio(z(3, 3, cin, cout)))
        dy = z(1, H, W, cout)
        r = ps_r if ps_r in (1, 2) else 1
        out = z(1, H // r, W // r, r * r * cin) if acc else None
        try:
            ops.conv3x3_dgrad_act_split2(dy, ops.absmax(dy), ws, z(1, H, W, cin), ops.ACT_LRELU, ps_r, out=out)
        except RuntimeError:
            return True
        return False

    assert not refused(16, 32, 32, 32, 2)
    assert not refused(17, 33, 32, 32, 1, acc=True)
    assert refused(17, 32, 32, 32, 2), "odd H"
    assert refused(16, 33, 32, 32, 2), "odd W"
    assert refused(18, 36, 32, 32, 3), "ps_r = 3"
    assert refused(16, 32, 32, 32, 2, acc=True), "ps_r = 2 with accumulate"
    assert refused(16, 32, 128, 32, 1), "128 produced channels"
    assert refused(16, 32, 64, 32, 1), "64 produced channels"
    assert not ops.conv3x3_dgrad_act_supported((1, 17, 32, 32), 32, ops.ACT_LRELU, 2)
    assert not ops.conv3x3_dgrad_act_supported((1, 18, 36, 32), 32, ops.ACT_LRELU, 3)
    assert not ops.conv3x3_dgrad_act_supported((1, 16, 32, 32), 32, ops.ACT_LRELU, 2, True)
    assert not ops.conv3x3_dgrad_act_supported((1, 16, 32, 128), 32, ops.ACT_LRELU, 1)
    return True


OFF_RUNS = 5
FUSED_LAYERS = 7        # upscale1.3 (accumulating), block.0, block.2, upscale2.0 (PixelShuffle), upscale2.3 (acc.), block.0, block.2


def check_net(device, monkeypatch):
    """The x8 net of conv9_dgrad_act_checks.NET_CASE, every split convolution forced on: one training backward with
    graph.FUSE_SPLIT_DGRAD_ACT on and OFF_RUNS with it off, from the same inputs.  The fused op runs FUSED_LAYERS times and
    ops.conv2d_epilogue_bwd that many times less.  The gradients of the HR tail's parameters and of head.0 differ from the
    first flag-off run by no more than twice the flag-off path's own run-to-run spread (per tensor, L2); where the flag-off
    runs agree to the bit - every weight gradient: the data-gradient chain and the weight-gradient reductions are ordered -
    so must the fused one.  The spread is the largest difference between any two of the OFF_RUNS flag-off runs, not one
    pair's: the tensors that do move (bias gradients, summed with float atomics; conv_output.bias is complete before any
    fused layer runs) move by a random amount, one pair's difference is a single draw of it, and with it as the yardstick
    the same code misses the factor of 2 in about a third of the runs (first GPU run of this test: conv_output.bias
    9.7e-5 against 3.1e-5).  The depth branch (mlp_mask, alpha_*) is not gated: its run-to-run nondeterminism is older than
    this path."""
    from dasr_amd import graph
    from dasr_amd.graph import block_plan
    from tests.conv9_dgrad_act_checks import NET_CASE
    monkeypatch.setattr(graph, "SPLIT_MIN_PIXELS", 0)
    net, cfg = build_net(NET_CASE, device)
    lq, gt, dm, mk = [t.to(device) for t in synth.closed_form_batch(0, NET_CASE["B"], NET_CASE["H"], NET_CASE["W"], cfg["scale"])]
    orig_fused, orig_epi = ops.conv3x3_dgrad_act_split2, ops.conv2d_epilogue_bwd
    res = []
    for on in (True,) + (False,) * OFF_RUNS:
        monkeypatch.setattr(graph, "FUSE_SPLIT_DGRAD_ACT", on)
        calls = dict(fused=0, epi=0)

        def fused(*a, _c=calls, **k):
            _c["fused"] += 1
            return orig_fused(*a, **k)

        def epi(*a, _c=calls, **k):
            _c["epi"] += 1
            return orig_epi(*a, **k)

        monkeypatch.setattr(ops, "conv3x3_dgrad_act_split2", fused)
        monkeypatch.setattr(ops, "conv2d_epilogue_bwd", epi)
        net.zero_grad(set_to_none=True)
        sr = net(lq, dm, mk)
        wgt = torch.cos(torch.arange(sr.numel(), dtype=torch.float32) * 0.013).reshape(sr.shape).to(device)
        (sr * wgt).sum().backward()
        res.append((calls, {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}))
    (c_on, g_on), (c_off, g_off) = res[0], res[1]
    offs = [g for _, g in res[1:]]
    assert c_on["fused"] == FUSED_LAYERS and all(c["fused"] == 0 for c, _ in res[1:]), [c for c, _ in res]
    assert all(c_on["epi"] == c["epi"] - FUSED_LAYERS for c, _ in res[1:]), [c for c, _ in res]
    assert all(g_on.keys() == g.keys() for g in offs)
    tail = ("upscale1.", "upscale2.", "upscale3.", "conv_output.", "head.0.weight") + \
        tuple(name + "." for name, _, _ in block_plan(cfg)[-2:])
    keys = [k for k in g_off if k.startswith(tail)]
    assert len(keys) >= 20 and any(k.startswith("head.0.weight") for k in keys), keys
    worst = (0.0, 0.0, None)
    for k in keys:
        d = (g_on[k] - g_off[k]).double().norm().item()
        spread = max((offs[i][k] - offs[j][k]).double().norm().item() for i in range(OFF_RUNS) for j in range(i))
        if d > worst[0]:
            worst = (d, spread, k)
        if d > 0:
            print("gradient on / off: %s diff %.3g, off / off spread %.3g" % (k, d, spread))
        if spread == 0:
            assert torch.equal(g_on[k], g_off[k]), ("gradient differs where the flag-off runs agree", k, d)
        else:
            assert d <= 2 * spread, ("gradient differs beyond the run-to-run spread", k, d, spread)
    return dict(epilogue_bwd_on=c_on["epi"], epilogue_bwd_off=c_off["epi"], fused=c_on["fused"], worst=worst, gated=len(keys))
