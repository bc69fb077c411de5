"""Checks of the 9x9 fp16 x 2 split forward in its two-workgroups-per-CU form (k_conv9_fwd_split, csrc/conv9_split.hip) against
its first form (k_conv9_fwd_split_1wg, `impl + 8192`).  The kernel walks 8 x 24 pixel tiles (16 x 32 staged pixels, 16 channels
at a time) with 256 threads, wave w on tile rows 2w, 2w+1; what can go wrong is the staged pieces' pixel map and swizzle, the
fragment addresses of the two row M-tiles, the P image and the precomputed shift-add map, a ragged tile row or column, the
XCD-blocked tile order (8 x 8 tile blocks, 512 slots per trip) and - `impl & 3 == 2`, three workgroups - the persistent loop
with the next chunk's / tile's loads in flight.  Per case:
  * check_bits: the launch EQUALS the first form's (the order of the products of every output element is the same); case f
    (more tiles than the grid holds, ragged tile blocks) also equals the linear tile order (`impl + 4096`);
  * check_float64: against torch's float64 convolution, the gate of check_conv9_split (error <= 1.25x the exact-fp32
    kernel's + 1e-7 on the hardware, 3x + 2e-7 on the emulator);
  * check_exact (cases a - e; f is a - e's arithmetic on more tiles and is held to the first form's bits): small-integer
    operands (|x| <= 8, |w| <= 4, integer bias, times the case's scales rounded to powers of two) - every product and every
    partial sum is exact in fp16 x 2 / fp32 (81 * 32 * 8 * 4 < 2^24), so the result IS torch's float64 convolution; a zero x
    gives the bias bitwise.
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_conv9_fwd.py runs them."""
import functools

import torch
import torch.nn.functional as F

from dasr_amd import ops
from tests.parity_checks import nchw, nhwc

CIN = 32
OLD, LINEAR = 8192, 4096
_A = dict(B=2, H=18, W=50, cout=3)          # two full tile rows plus a ragged one; a ragged tile column at 24 and at 56 columns
CASES = {
    "a": dict(_A, impl=0),
    "b": dict(B=1, H=10, W=100, cout=3, impl=0),         # many tile columns
    "c": dict(B=1, H=12, W=34, cout=1, impl=0),
    "d": dict(_A, impl=2),                               # three workgroups, tile lists with loads in flight
    "e": dict(_A, impl=0, sx=37.0, sw=2e-6),             # scales far from 1
    "f": dict(B=3, H=76, W=500, cout=3, impl=0),         # 630 tiles for 512 workgroups; 3 x 2 tile blocks per sample, both ragged
}
CHECKS = ("check_bits", "check_float64")
EXACT_CASES = ("a", "b", "c", "d", "e")


def _pow2(s):
    return 2.0 ** round(torch.log2(torch.tensor(float(s))).item())


@functools.lru_cache(maxsize=None)
def _operands(case):
    """CPU operands (NCHW fp32) and the float64 references, once per case: random ones and small-integer ones."""
    c = CASES[case]
    B, H, W, cout = c["B"], c["H"], c["W"], c["cout"]
    gen = torch.Generator().manual_seed(90 + H + W + cout)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sx, sw = c.get("sx", 1.0), c.get("sw", 1.0)
    x = rn(B, CIN, H, W) * sx
    w = rn(cout, CIN, 9, 9) * 0.02 * sw
    bias = rn(cout) * 0.3 * sx * sw
    ref = F.conv2d(x.double(), w.double(), bias.double(), padding=4)
    out = dict(x=x, w=w, bias=bias, ref=ref)
    if case in EXACT_CASES:
        px, pw = _pow2(sx), _pow2(sw)
        xi = torch.randint(-8, 9, (B, CIN, H, W), generator=gen).float() * px
        wi = torch.randint(-4, 5, (cout, CIN, 9, 9), generator=gen).float() * pw
        bi = torch.randint(-50, 51, (cout,), generator=gen).float() * (px * pw)
        assert xi.abs().max().item() == 8 * px and wi.abs().max().item() == 4 * pw
        out.update(xi=xi, wi=wi, bi=bi, refi=F.conv2d(xi.double(), wi.double(), bi.double(), padding=4))
    return out


_runs = {}


def _launch(xd, wp, bd, impl):
    ops.set_conv_bf16_impl(impl)
    try:
        return ops.conv9_fwd_split2(xd, ops.absmax(xd), wp, ops.absmax(wp[0]), bd).cpu()
    finally:
        ops.set_conv_bf16_impl(0)


def _run(device, case):
    """The launches of one (device, case), once."""
    key = (device, case)
    if key in _runs:
        return _runs[key]
    c, o = CASES[case], _operands(case)
    assert ops.conv9_split_supported(c["H"], c["W"], CIN, c["cout"]) and not ops.conv9_split_supported(c["H"], c["W"], 64, c["cout"])
    pack = lambda w: ops.pack_hwio(w.permute(2, 3, 1, 0).contiguous().to(device))
    xd, wp, bd = nhwc(o["x"]).to(device), pack(o["w"]), o["bias"].to(device)
    out = dict(new=_launch(xd, wp, bd, c["impl"]), old=_launch(xd, wp, bd, c["impl"] | OLD))
    if case == "f":
        out["linear"] = _launch(xd, wp, bd, c["impl"] | LINEAR)
    out["y32"] = ops.conv2d_fwd(xd, wp, bd, pad=4).cpu()
    if case in EXACT_CASES:
        xi, wi, bi = nhwc(o["xi"]).to(device), pack(o["wi"]), o["bi"].to(device)
        out["int"] = _launch(xi, wi, bi, c["impl"])
        out["zero"] = _launch(torch.zeros_like(xi), wi, bi, c["impl"])
    return _runs.setdefault(key, out)


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def check_bits(device, case):
    r = _run(device, case)
    c = CASES[case]
    assert r["new"].shape == r["old"].shape == (c["B"], c["H"], c["W"], c["cout"])
    bad = r["new"] != r["old"]
    assert torch.equal(r["new"], r["old"]), ("the two forms differ", case, int(bad.sum()), bad.nonzero()[:4].tolist())
    if "linear" in r:
        bad = r["new"] != r["linear"]
        assert torch.equal(r["new"], r["linear"]), ("XCD-blocked and linear tile order differ", int(bad.sum()), bad.nonzero()[:4].tolist())
    return dict(tiles=c["B"] * ((c["H"] + 7) // 8) * ((c["W"] + 23) // 24))


def check_float64(device, case):
    r = _run(device, case)
    ref = _operands(case)["ref"]
    fac, slack = (3.0, 2e-7) if device == "cpu" else (1.25, 1e-7)
    e_sp, e_32 = _rel(nchw(r["new"]), ref), _rel(nchw(r["y32"]), ref)
    print("%s %s: split %.3g, exact fp32 %.3g" % (case, device, e_sp, e_32))
    assert e_sp <= fac * e_32 + slack, ("conv9 fwd", case, e_sp, e_32)
    return dict(split=e_sp, fp32=e_32)


def check_exact(device, case):
    r, o = _run(device, case), _operands(case)
    got, want = nchw(r["int"]).double(), o["refi"]
    bad = got != want
    assert torch.equal(got, want), ("small-integer operands: not exact", case, int(bad.sum()), bad.nonzero()[:4].tolist())
    zero = r["zero"]
    assert torch.equal(zero, o["bi"].expand_as(zero)), ("zero x: not the bias", case)
    return dict(max=want.abs().max().item())
