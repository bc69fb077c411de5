"""Checks of the 9x9 fp16 x 2 split weight gradient (k_conv9_wgrad_split + k_conv9_wgrad_reduce_split, csrc/conv9_split.hip):
the dy tile split once into two fp16 row images, E pieces built from aligned dwords, and the slabs summed in a fixed order.
What can go wrong is the precomputed dy element map (row, column, the division by Cout), the E piece's element offset and
parity, the k' mask, a ragged tile, the persistent loop with the next tile's loads in flight (`impl & 3 == 2`: three partial
indices with long tile lists) and the reduction's slab order.  Per case:
  * check_float64: against torch's float64 weight gradient, the gate of check_conv9_split (error <= 1.25x the exact-fp32
    kernel's + 1e-7 on the hardware, 3x + 2e-7 on the emulator);
  * check_exact: small-integer operands (|x| <= 8, |dy| <= 4: every product and every partial sum over at most 2 * 18 * 50
    pixels is exact in fp16 x 2 / fp32) give torch's float64 gradient exactly;
  * check_repeat: two launches give bitwise equal dw (no atomics in the reduction).
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_conv9_wgrad.py runs them."""
import functools

import torch
import torch.nn.functional as F

from dasr_amd import ops
from tests.parity_checks import nhwc, rel_max

CIN = 32
_A = dict(B=2, H=18, W=50, cout=3)          # two full tile rows plus a ragged one, a ragged tile column, two samples
CASES = {
    "a": dict(_A, impl=0),
    "c": dict(B=1, H=12, W=34, cout=1, impl=0),
    "d": dict(_A, impl=2),                   # three partial indices, six tiles each, loads in flight
}
CHECKS = ("check_float64", "check_exact", "check_repeat")


def _grad64(x, dy, cout):
    w = torch.zeros(cout, CIN, 9, 9, dtype=torch.float64, requires_grad=True)
    gw, = torch.autograd.grad(F.conv2d(x.double(), w, None, padding=4), (w,), dy.double())
    return gw.permute(2, 3, 1, 0).contiguous()          # HWIO


@functools.lru_cache(maxsize=None)
def _operands(case):
    c = CASES[case]
    B, H, W, cout = c["B"], c["H"], c["W"], c["cout"]
    gen = torch.Generator().manual_seed(70 + H + W + cout)
    x, dy = torch.randn(B, CIN, H, W, generator=gen), torch.randn(B, cout, H, W, generator=gen)
    xi = torch.randint(-8, 9, (B, CIN, H, W), generator=gen).float()
    di = torch.randint(-4, 5, (B, cout, H, W), generator=gen).float()
    return dict(x=x, dy=dy, ref=_grad64(x, dy, cout), xi=xi, di=di, refi=_grad64(xi, di, cout))


_runs = {}


def _launch(xd, dyd, impl):
    ops.set_conv_bf16_impl(impl)
    try:
        return ops.conv9_wgrad_split2(xd, ops.absmax(xd), dyd, ops.absmax(dyd))[0].cpu()
    finally:
        ops.set_conv_bf16_impl(0)


def _run(device, case):
    key = (device, case)
    if key in _runs:
        return _runs[key]
    c, o = CASES[case], _operands(case)
    xd, dyd = nhwc(o["x"]).to(device), nhwc(o["dy"]).to(device)
    out = dict(dw=_launch(xd, dyd, c["impl"]), again=_launch(xd, dyd, c["impl"]),
               dw32=ops.conv2d_wgrad(xd, dyd, (9, 9, CIN, c["cout"]), pad=4)[0].cpu(),
               int=_launch(nhwc(o["xi"]).to(device), nhwc(o["di"]).to(device), c["impl"]))
    return _runs.setdefault(key, out)


def check_float64(device, case):
    r, ref = _run(device, case), _operands(case)["ref"]
    fac, slack = (3.0, 2e-7) if device == "cpu" else (1.25, 1e-7)
    assert r["dw"].shape == ref.shape
    w_sp, w_32 = rel_max(r["dw"], ref), rel_max(r["dw32"], ref)
    print("%s %s: split %.3g, exact fp32 %.3g" % (case, device, w_sp, w_32))
    assert w_sp <= fac * w_32 + slack, ("conv9 wgrad", case, w_sp, w_32)
    return dict(split=w_sp, fp32=w_32)


def check_exact(device, case):
    r, want = _run(device, case), _operands(case)["refi"]
    got = r["int"].double()
    bad = got != want
    assert torch.equal(got, want), ("small-integer operands: not exact", case, int(bad.sum()), bad.nonzero()[:4].tolist())
    return dict(max=want.abs().max().item())


def check_repeat(device, case):
    r = _run(device, case)
    assert torch.equal(r["dw"], r["again"]), ("two launches differ", case, int((r["dw"] != r["again"]).sum()))
    return True
