"""Checks of the fp16 x 2 weight-gradient kernel's tile order and row ring (k_conv3x3_wgrad_split2, csrc/conv_split_bf16.hip).
A workgroup walks a contiguous run of tiles down 32-pixel column strips and keeps the x rows a tile shares with the previous
one in LDS row slots (every instantiation: TH + 2 = 4, 6 or 10 slots).  What can go wrong is a stale, misplaced, doubled or
non-zeroed row at a strip change, an image change, a ragged last tile or a ragged strip.  Per shape:
  * float64: the gates of check_split_conv (operands scaled as there) next to the exact-fp32 kernel;
  * exactness: small-integer operands, for which every piece, product and partial sum is exact - dw and dbias must EQUAL
    the float64 result, whatever the summation order;
  * repeatability: two launches give bit-equal dw, and the long walks of `impl & 2` the bits of the plain launch.
plan() recomputes the kernel's tile runs from the workspace query and asserts that the `impl & 2` cases (at most three
workgroups per channel block) really walk long runs with strip changes in them.
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_wgrad_ring.py runs them."""
import functools

import torch
import torch.nn.functional as F

from dasr_amd import _lib, ops
from tests.parity_checks import nhwc, rel_max

F64 = torch.float64
# (Cin, Cout, B, H, W), impl, the instantiation <MT, NTW> the shape must select
EMU_CASES = (((64, 64, 2, 11, 40), 2, (2, 2)),      # 24 tiles over 3 workgroups: runs of 8, odd H, W = 32 + 8, strip and image change
             ((32, 32, 1, 19, 33), 2, (1, 1)))      # TH = 8, G = 4: three tiles high with a ragged one, a strip one pixel wide
GPU_ONLY_CASES = tuple((s, impl, inst) for s, inst in (((128, 128, 2, 37, 70), (2, 2)), ((32, 128, 1, 21, 64), (1, 4)),
                                                       ((64, 32, 1, 13, 40), (2, 1)), ((32, 64, 1, 13, 40), (1, 2)))
                       for impl in (0, 2)) + (((64, 64, 8, 70, 64), 0, (2, 2)),)     # natural plan: 560 tiles > P = 512
CHECKS = ("check_float64", "check_exact", "check_repeat")


def case_id(case):
    (cin, cout, B, H, W), impl, _ = case
    return "%d-%d-%dx%dx%d-impl%d" % (cin, cout, B, H, W, impl)


def plan(case):
    """The tile runs the workgroups walk, from the shape and the workspace query: dict(th, ntiles, P, runs = [(first,
    last + 1)]) and, per run, steps = (adjacent steps: same image and strip, ty one larger - the ring keeps two rows; the
    others).  P slabs (the workspace's); `impl & 2` launches min(P, 3) workgroups, each walking a list of slabs."""
    (cin, cout, B, H, W), impl, inst = case
    mt = 2 if cin % 64 == 0 else 1
    ntw = 2 if cout % 64 == 0 else 1
    if mt == 1 and cout % 128 == 0:
        ntw = 4
    assert (mt, ntw) == inst, ((mt, ntw), inst)
    th = {4: 2, 2: 4, 1: 8}[mt * ntw]
    tiles_y, tiles_x = (H + th - 1) // th, (W + 31) // 32
    ntiles = B * tiles_y * tiles_x
    nbytes = int(_lib.get().dasr_conv3x3_wgrad_split_workspace(B, H, W, cin, cout))
    P = nbytes // (4 * (9 * cin * cout + cout))
    assert P * 4 * (9 * cin * cout + cout) == nbytes and 1 <= P <= ntiles, (P, nbytes, ntiles)
    # slab p sums the tiles [p ntiles / P, (p + 1) ntiles / P); a workgroup walks the slabs [w P / nwg, (w + 1) P / nwg)
    nwg = min(P, 3) if impl & 2 else P
    runs = [((w * P // nwg) * ntiles // P, ((w + 1) * P // nwg) * ntiles // P) for w in range(nwg)]
    # tile t = (image, strip, ty) with ty fastest: the step t -> t + 1 is adjacent unless t + 1 starts a strip
    steps = [(sum(1 for t in range(a + 1, b) if t % tiles_y != 0), sum(1 for t in range(a + 1, b) if t % tiles_y == 0)) for a, b in runs]
    return dict(th=th, ntiles=ntiles, P=P, nwg=nwg, runs=runs, steps=steps)


def check_plan(case):
    """Every `impl & 2` case has a run of at least 3 tiles with a non-adjacent step in it (and, with it, adjacent ones): the
    checks below cannot pass by never using the ring, or by never leaving a strip inside a run.
    The (32, 32, 1, 19, 33) case holds 6 tiles (three high, two strips) over min(P, 3) = 3 workgroups: no plan with three
    workgroups gives it a run of 3.  Its runs are 2 tiles long - two of them one ring step each (the second one into the
    ragged tile), the middle one across the strip change - and that is what is asserted for it."""
    pl = plan(case)
    (cin, cout, B, H, W), impl, _ = case
    if not impl & 2:
        return pl
    if case[0] == (32, 32, 1, 19, 33):
        assert pl["runs"] == [(0, 2), (2, 4), (4, 6)] and pl["steps"] == [(1, 0), (0, 1), (1, 0)], pl
        return pl
    assert any(b - a >= 3 and other >= 1 and adj >= 1 for (a, b), (adj, other) in zip(pl["runs"], pl["steps"])), pl
    return pl


def _ref_wgrad(x, dy):
    """float64 (dw [3, 3, Cin, Cout], dbias) of NCHW fp32 operands."""
    dw = F.conv2d(x.to(F64).transpose(0, 1), dy.to(F64).transpose(0, 1), padding=1).transpose(0, 1)       # [Cout, Cin, 3, 3]
    return dw.permute(2, 3, 1, 0).contiguous(), dy.to(F64).sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def _operands(case, kind):
    """(x, dy, dw64, db64): NCHW fp32 CPU operands and their float64 gradient, computed once per case and kind."""
    (cin, cout, B, H, W), impl, _ = case
    gen = torch.Generator().manual_seed(1000 + 7 * cin + cout + H + (1 if kind == "int" else 0))
    if kind == "int":
        x = torch.randint(-8, 9, (B, cin, H, W), generator=gen).float()
        dy = torch.randint(-4, 5, (B, cout, H, W), generator=gen).float()
        assert 8 * 4 * B * H * W < 2 ** 24          # every partial sum is an integer below 2^24: exact in fp32
    else:
        rn = lambda *s: torch.randn(*s, generator=gen)
        x = rn(B, cin, H, W) * (1.0 + rn(B, cin, 1, 1).abs()) * 665.6
        dy = rn(B, cout, H, W) * 3e-8
    return (x, dy) + _ref_wgrad(x, dy)


_first = {}


def _launch(device, case, kind, again=False, impl=None):
    """(dw, dbias) of the split kernel as float64-comparable CPU tensors; the first launch per (device, case, kind) is kept
    (check_repeat compares a second one with it).  impl: instead of the case's."""
    key = (device, case, kind)
    if key in _first and not again:
        return _first[key]
    x, dy = _operands(case, kind)[:2]
    xd, dyd = nhwc(x).to(device), nhwc(dy).to(device)
    ops.set_conv_bf16_impl(case[1] if impl is None else impl)
    try:
        dw, db = ops.conv3x3_wgrad_split2(xd, ops.absmax(xd), dyd, ops.absmax(dyd))
        out = (dw.cpu(), db.cpu())
    finally:
        ops.set_conv_bf16_impl(0)
    return _first.setdefault(key, out)


def check_float64(device, case):
    check_plan(case)
    (cin, cout, B, H, W), impl, _ = case
    x, dy, dw64, db64 = _operands(case, "randn")
    dw, db = _launch(device, case, "randn")
    dw32, db32 = ops.conv2d_wgrad(nhwc(x).to(device), nhwc(dy).to(device), (3, 3, cin, cout))
    fac, slack = (3.0, 2e-7) if device == "cpu" else (1.25, 1e-7)
    e_sp, e_32 = rel_max(dw, dw64), rel_max(dw32, dw64)
    b_sp, b_32 = rel_max(db, db64), rel_max(db32, db64)
    print("%s %s: dw split %.3g fp32 %.3g, dbias split %.3g fp32 %.3g" % (case_id(case), device, e_sp, e_32, b_sp, b_32))
    assert e_sp <= fac * e_32 + slack, ("dw", case, e_sp, e_32)
    assert b_sp <= 2 * b_32 + 1e-6, ("dbias", case, b_sp, b_32)
    return dict(dw=e_sp, dw32=e_32, db=b_sp, db32=b_32)


def check_exact(device, case):
    pl = check_plan(case)
    x, dy, dw64, db64 = _operands(case, "int")
    dw, db = _launch(device, case, "int")
    bad = (dw.to(F64) != dw64)
    assert not bool(bad.any()), ("dw", case, int(bad.sum()), bad.nonzero()[:4].tolist(), pl["runs"])
    assert torch.equal(db.to(F64), db64), ("dbias", case)
    return dict(runs=pl["runs"], steps=pl["steps"])


def check_repeat(device, case):
    dw0, db0 = _launch(device, case, "int")
    dw1, db1 = _launch(device, case, "int", again=True)
    assert torch.equal(dw0, dw1), ("dw differs between two launches", case, rel_max(dw1, dw0))
    assert torch.equal(db0, db1), ("dbias differs between two launches", case)
    if case[1] & 2:
        # the long walks of `impl & 2` fill the same slabs with the same sums as the plain launch: bit-equal, on real-valued
        # operands (on the integer ones any order gives the same bits)
        dw2, db2 = _launch(device, case, "randn")
        dwp, dbp = _launch(device, case, "randn", again=True, impl=case[1] & ~2)
        assert torch.equal(dw2, dwp) and torch.equal(db2, dbp), ("impl & 2 differs from the plain launch", case, rel_max(dw2, dwp))
    return True
