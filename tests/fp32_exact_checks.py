"""The exact-fp32 convolution family at op level, every kernel form: csrc/conv_mfma.hip (3x3 / stride 1 on the fp32 matrix
cores: 8-row and 16-row tiles, NT = 1 | 2, the fused dgrad_act and fwd_stats epilogues, five weight-gradient blocks),
csrc/conv_gather_mfma.hip (strided, transposed and odd-channel layers), csrc/conv9_mfma.hip (the 9x9 output convolution),
csrc/conv_direct.hip (everything else, and the bias gradient's column sum), behind dasr_conv2d_{fwd, fwd_stats, dgrad,
dgrad_act, wgrad, wgrad_act}.  Every fp16x2 / bf16x3 split gate of the suite is a multiple of this family's error, so it
is pinned here on its own.  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_fp32_exact.py runs every one of them on both.

Three kinds of gate (DESIGN.md 2 has the case table and the measured figures):
  A  integer data     x, w, dy in [-2, 2], bias in [-3, 3], residual / accumulate base in [-4, 4]: every partial sum is an
                      integer below 2^24, fp32 is exact in ANY order (slabs, atomics): every element equals float64
  B  full mantissa    24-bit operands against kernels with ONE non-zero power of two per produced channel: every output is
                      one operand times 2^e (+ bias / base: one rounding).  A kernel that dropped low mantissa bits passes A
                      (small integers are bf16 / fp16 numbers) and fails here
  C  derived bound    |kernel - float64| <= gamma_n * conv(|a|, |b|) per ELEMENT, gamma_n the any-order fp32 summation
                      bound: an error is judged against its own element's magnitude, not the tensor's maximum
The kernel FORM a case is written for is asserted, not assumed: the tile rows from ops.conv2d_fwd_tile_rows (16 for every
"16-row" case and 8 for the same shape with B - 1), the weight gradient's slab count P from dasr_conv2d_wgrad_workspace.
Every result is read back and then poisoned (_take); references are float64 torch, never another entry point of the
library.  A case with ``emu=False`` runs on the MI355X only (the emulator does about 50 M MAC/s)."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from dasr_amd import _lib, ops
from tests.bf16_exact_checks import _ints, _nbad, _poison, _ref_fwd, _ref_grads, _take
from tests.parity_checks import nchw, nhwc
from tests.split_range_checks import make_operands

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_LRELU = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU
SLOPE32 = torch.tensor(0.2, dtype=torch.float32)

# One case.  ``parts``: which of y (forward), x (dgrad, plain and accumulating), w (wgrad + bias gradient) run.
# ``rows`` / ``rows_dgrad``: tile rows asserted for the forward / for the data gradient (the form of (Cout, Cin)); 0 = not
# the MFMA 3x3 family; None = not asserted (no 3x3 / stride-1 geometry).  ``fam`` + ``P``: the weight gradient's family
# ("mfma", "gather", "conv9", "direct") and its slab count, both read from the workspace size.
Case = namedtuple("Case", "cin cout B H W k stride pad tr bias act res ps parts rows rows_dgrad fam P emu")


def case(cin, cout, B, H, W, k=3, stride=1, pad=None, tr=False, bias=True, act=ACT_NONE, res=False, ps=1, parts="yxw",
         rows=None, rows_dgrad=None, fam=None, P=None, emu=True):
    return Case(cin, cout, B, H, W, k, stride, k // 2 if pad is None else pad, tr, bias, act, res, ps, parts, rows,
                rows_dgrad, fam, P, emu)


def _on(device, cases):
    return [c for c in cases if c.emu or device != "cpu"]


def _out_hw(c):
    return ops.conv_out_hw(c.H, c.W, c.k, c.k, c.stride, c.pad, c.tr)


def _wshape(c):
    """torch's layout: OIHW, and IOHW for a ConvTranspose2d."""
    return (c.cin, c.cout, c.k, c.k) if c.tr else (c.cout, c.cin, c.k, c.k)


def _hwio(w, c):
    return (w.permute(2, 3, 0, 1) if c.tr else w.permute(2, 3, 1, 0)).contiguous()


def _dw_torch(dw_hwio, c):
    """The library's HWIO weight gradient in torch's layout of the kernel."""
    return dw_hwio.permute(2, 3, 0, 1) if c.tr else dw_hwio.permute(3, 2, 0, 1)


def _conv64(x, w, bias, c):
    if c.tr:
        return F.conv_transpose2d(x, w, bias, stride=c.stride, padding=c.pad)
    return F.conv2d(x, w, bias, stride=c.stride, padding=c.pad)


def _ref_y(x, w, bias, res, c, exact_lrelu=True):
    """float64 conv + bias -> PixelShuffle -> + residual -> activation (the epilogue of _ref_fwd; a strided or transposed
    convolution goes through it as an identity 1x1 convolution of its float64 result: times 1.0, plus zeros)."""
    if res is not None and c.ps > 1:
        res = F.pixel_shuffle(res, c.ps)       # the library takes the residual as [B, Ho, Wo, Cout], _ref_fwd shuffled
    if c.stride == 1 and not c.tr:
        return _ref_fwd(x, w, bias, res, c.act, c.ps, pad=c.pad, exact_lrelu=exact_lrelu)
    eye = torch.eye(c.cout, dtype=F64).reshape(c.cout, c.cout, 1, 1)
    return _ref_fwd(_conv64(x, w, bias, c), eye, None, res, c.act, c.ps, pad=0, exact_lrelu=exact_lrelu)


def _ref_g(x, w, dy, c, parts="xw"):
    """float64 (dx, dw in torch's layout, db) of the pure convolution; dx alone (``parts`` without w) of a stride-1 layer
    is the transposed convolution written out, so that a large data-gradient case does not pay for a weight gradient."""
    if "w" not in parts and c.stride == 1 and not c.tr:
        return F.conv_transpose2d(dy, w, None, stride=1, padding=c.pad), None, None
    if c.stride == 1 and not c.tr:
        return _ref_grads(x, w, dy, pad=c.pad)
    xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bt = torch.zeros(c.cout, dtype=F64, requires_grad=True)
    return torch.autograd.grad(_conv64(xt, wt, bt, c), (xt, wt, bt), dy)


def _d(t_nchw, device):
    return nhwc(t_nchw).to(torch.float32).to(device)


def _packed(w, c, device):
    return ops.pack_hwio(_hwio(w, c).to(torch.float32).to(device))


def _geom(c):
    Ho, Wo = _out_hw(c)
    return (c.B, c.H, c.W, c.cin, Ho, Wo, c.cout, c.k, c.k, c.stride, c.pad, int(c.tr))


def wgrad_slabs(c):
    """The weight gradient's family and slab count P, from the workspace the library asks for: bytes / (4 * slab size).
    mfma: 9 Cin Cout + Cout floats per slab (the bias partials ride along); gather: K K Cin Cout; conv9: four waves x Cin / 32
    blocks of 9 x 32 x 32 per tile strip; direct (atomics into dw): no workspace."""
    nbytes = int(_lib.get().dasr_conv2d_wgrad_workspace(*_geom(c)))
    slab = {"mfma": 9 * c.cin * c.cout + c.cout, "gather": c.k * c.k * c.cin * c.cout,
            "conv9": 4 * (c.cin // 32) * 9 * 32 * 32, "direct": 1}[c.fam]
    if c.fam == "direct":
        assert nbytes == 0, ("a workspace for the direct weight gradient", c, nbytes)
        return 0
    assert nbytes > 0 and nbytes % (4 * slab) == 0, ("workspace is no whole number of %s slabs" % c.fam, c, nbytes)
    return nbytes // (4 * slab)


def assert_form(c):
    """The kernel form the case names is the one the library runs."""
    if c.rows is not None:
        got = ops.conv2d_fwd_tile_rows(c.B, c.H, c.W, c.cin, c.cout)
        assert got == c.rows, ("forward tile rows", c, got)
        if c.rows == 16:
            assert ops.conv2d_fwd_tile_rows(c.B - 1, c.H, c.W, c.cin, c.cout) == 8, ("the B - 1 neighbour is not 8-row", c)
    if c.rows_dgrad is not None:
        got = ops.conv2d_fwd_tile_rows(c.B, c.H, c.W, c.cout, c.cin)
        assert got == c.rows_dgrad, ("dgrad tile rows", c, got)
        if c.rows_dgrad == 16:
            assert ops.conv2d_fwd_tile_rows(c.B - 1, c.H, c.W, c.cout, c.cin) == 8, ("the B - 1 neighbour is not 8-row", c)
    if c.fam is not None and "w" in c.parts:
        P = wgrad_slabs(c)
        assert c.P is None or P == c.P, ("weight-gradient slabs", c, P)


def run_ops(device, c, x, w, bias, res, dy, base):
    """y, dx, dx accumulated onto ``base``, dw (torch's layout), db of one layer from the fp32 entry points, as poisoned-
    after-reading CPU copies; parts that ``c.parts`` leaves out come back as None."""
    xd, wp, dyd = _d(x, device), _packed(w, c, device), _d(dy, device)
    bd = None if bias is None else bias.to(torch.float32).to(device)
    rd = None if res is None else _d(res, device)
    y = dx = acc = dw = db = None
    if "y" in c.parts:
        y = ops.conv2d_fwd(xd, wp, bd, rd, c.stride, c.pad, c.tr, c.act, c.ps)
    if "x" in c.parts:
        dx = ops.conv2d_dgrad(dyd, wp, xd.shape, c.stride, c.pad, c.tr)
        acc = _d(base, device).clone()
        assert ops.conv2d_dgrad(dyd, wp, xd.shape, c.stride, c.pad, c.tr, out=acc) is acc
    if "w" in c.parts:
        dw, db = ops.conv2d_wgrad(xd, dyd, (c.k, c.k, c.cin, c.cout), c.stride, c.pad, c.tr)
    y, dx, acc, dw, db = (None if t is None else _take(t) for t in (y, dx, acc, dw, db))
    return (None if y is None else nchw(y), None if dx is None else nchw(dx), None if acc is None else nchw(acc),
            None if dw is None else _dw_torch(dw, c), db)


# =====================================================================================================================
# A. integer operands: every element exact
# =====================================================================================================================
def _int_operands(c, seed):
    gen = torch.Generator().manual_seed(seed)
    Ho, Wo = _out_hw(c)
    # every partial sum of any order stays an integer below 2^24
    assert 4 * c.k * c.k * max(c.cin, c.cout) + 7 < 2 ** 24 and 4 * c.B * max(Ho * Wo, c.H * c.W) < 2 ** 24
    x, w = _ints(gen, -2, 2, c.B, c.cin, c.H, c.W), _ints(gen, -2, 2, *_wshape(c))
    dy = _ints(gen, -2, 2, c.B, c.cout, Ho, Wo)
    bias = _ints(gen, -3, 3, c.cout) if c.bias else None
    res = _ints(gen, -4, 4, c.B, c.cout, Ho, Wo) if c.res else None                # the ABI's layout: before the shuffle
    base = _ints(gen, -4, 4, c.B, c.cin, c.H, c.W)
    return x, w, dy, bias, res, base


def _int_cases(device, cases, seed0):
    """A for a list of cases: y (with its epilogue), dx, ``out=``-accumulated dx, dw, db == float64 in every element."""
    n = 0
    for i, c in enumerate(_on(device, cases)):
        assert_form(c)
        x, w, dy, bias, res, base = _int_operands(c, seed0 + i)
        y, dx, acc, dw, db = run_ops(device, c, x, w, bias, res, dy, base)
        bad = {}
        if "y" in c.parts:
            bad["y"] = _nbad(y, _ref_y(x, w, bias, res, c))
        if "x" in c.parts or "w" in c.parts:
            gx, gw, gb = _ref_g(x, w, dy, c, c.parts)
            if "x" in c.parts:
                bad["dx"], bad["dx_acc"] = _nbad(dx, gx), _nbad(acc, gx + base)
            if "w" in c.parts:
                bad["dw"], bad["db"] = _nbad(dw, gw), _nbad(db, gb)
        assert not any(bad.values()), ("mismatching elements", c, bad)
        n += 1
    return {"cases": n}


# k_conv3x3_mfma, 8-row tiles / 256 threads (rows = 8), forward and dgrad:
#   (64, 64, 2, 17, 33)    NT = 2, four chunks; ragged third tile row and second tile column; 12 pixel tiles: not a multiple
#                          of 8, the XCD-ordered grid is padded with workgroups that must leave at once
#   (128, 128, 1, 9, 33)   eight chunks, NT = 2, two N slices
#   (16, 32, 2, 8, 34)     ONE chunk (the prefetch of a next chunk never runs), NT = 1; its dgrad and wgrad are not MFMA
#   (32, 128, 2, 10, 35)   PixelShuffle(2) + LeakyReLU through the fast and the generic epilogue; the 32x128 wgrad block
#   (32, 32, 1, 8, 34)     ReLU + residual; exact tile height; the 32x32 wgrad block
#   (64, 32, ...), (32, 64, ...)   the 64x32 and 32x64 wgrad blocks (NT = 1 forward with four chunks; NT = 2 with two)
CONV3_8ROW = (
    case(64, 64, 2, 17, 33, rows=8, rows_dgrad=8, fam="mfma", P=36),
    case(128, 128, 1, 9, 33, rows=8, rows_dgrad=8, fam="mfma"),
    case(16, 32, 2, 8, 34, act=ACT_RELU, rows=8, rows_dgrad=0, fam="direct"),
    case(32, 128, 2, 10, 35, act=ACT_LRELU, ps=2, rows=8, rows_dgrad=8, fam="mfma"),
    case(32, 32, 1, 8, 34, act=ACT_RELU, res=True, rows=8, rows_dgrad=8, fam="mfma"),
    case(64, 32, 1, 9, 33, act=ACT_LRELU, rows=8, rows_dgrad=8, fam="mfma"),
    case(32, 64, 1, 9, 33, bias=False, rows=8, rows_dgrad=8, fam="mfma"),
)


def check_int_conv3_8row(device):
    """A on the 8-row forms of k_conv3x3_mfma (forward and dgrad, NT = 1 and 2) and the five blocks of
    k_conv3x3_wgrad_mfma (64x64, 64x32, 32x64, 32x128, 32x32), CONV3_8ROW.  All run on the emulator."""
    return _int_cases(device, CONV3_8ROW, 7100)


# k_conv3x3_mfma, 16-row tiles / 512 threads: H % 16 == 0 and the 16-row grid a multiple of 256 workgroups.
#   16 -> 32  at 16 x 64 x 128   NT = 1 forward: 4 x 4 x 16 tiles x 1 slice = 256; ReLU + residual, fast epilogue
#   32 -> 16  at 16 x 64 x 128   its mirror: the NT = 1 dgrad (plain and accumulating)
#   16 -> 256 at 4 x 64 x 128    NT = 2 forward: 4 x 4 x 4 tiles x 4 slices = 256, fast epilogue, PixelShuffle(2) + LeakyReLU
#   16 -> 256 at 4 x 64 x 127    the same through the generic epilogue in the last tile column (the query still says 16)
#   256 -> 16 at 4 x 64 x 128    the NT = 2 dgrad
# The emulator runs the two NT = 1 cases (12 s each); the NT = 2 ones (24 s each there) run on the MI355X only.
CONV3_16ROW = (
    case(16, 32, 16, 64, 128, act=ACT_RELU, res=True, parts="y", rows=16),
    case(32, 16, 16, 64, 128, parts="x", rows_dgrad=16),
    case(16, 256, 4, 64, 128, act=ACT_LRELU, ps=2, parts="y", rows=16, emu=False),
    case(16, 256, 4, 64, 127, act=ACT_LRELU, parts="y", rows=16, emu=False),
    case(256, 16, 4, 64, 128, parts="x", rows_dgrad=16, emu=False),
)


def check_int_conv3_16row(device):
    """A on the 16-row / 512-thread forms of k_conv3x3_mfma, CONV3_16ROW: each case asserts 16 from the query and 8 for
    its B - 1 neighbour.  Emulator: the NT = 1 forward and dgrad; MI355X: NT = 2 as well."""
    return _int_cases(device, CONV3_16ROW, 7200)


# k_conv3x3_wgrad_mfma workgroups that walk more than one pixel tile: 128 -> 256 has 2 x 4 = 8 (ci, co) groups, so P =
# 512 / 8 = 64 strips, and 2 x 33 x 33 is 2 x 17 x 2 = 68 tiles of the 64x64 block's 2 x 32 pixels: the first four strips
# take a second tile.  (P is min(512 / groups, tiles): P = 64 from the workspace says the tile count is no smaller.)
# Emulator: 13 s.
WGRAD_STRIPS = (case(128, 256, 2, 33, 33, parts="w", fam="mfma", P=64),)


def check_int_wgrad_strips(device):
    """A on the weight gradient of 128 -> 256 at 2 x 33 x 33: 68 pixel tiles on P = 64 strips (asserted from the workspace),
    and the bias partials of strips that saw two tiles."""
    return _int_cases(device, WGRAD_STRIPS, 7300)


# k_conv_gather_mfma<1 | 2> (GATHER 0 and 1, forward and dgrad) and k_conv_gather_wgrad_mfma:
#   32 -> 64 stride 2 at 2 x 9 x 11 and 2 x 8 x 10   odd and even H x W (the last window hangs over the edge or not)
#   64 -> 128 stride 2 at 1 x 9 x 11                 two K trips per tap, two N slices
#   128 -> 64 transposed at 1 x 5 x 6 and 2 x 4 x 5  Ho x Wo = 9 x 11 / 7 x 9: odd, so the four residue classes hold 30, 25,
#                                                    24, 20 pixels (B = 1): unequal, and the 32-pixel M-tiles straddle every
#                                                    class boundary
#   8 | 24 | 40 -> 32 stride 1                        partial last K trip of the forward (8, 24, 8 channels of 32)
#   32 -> 8 | 24 | 40 stride 1                        the same in the dgrad (the forward is the direct kernel)
#   32 -> 64 stride 2 at 1 x 34 x 34                  wgrad with M = 289 output pixels: P = 2 slabs of per = 145 (odd: a
#                                                    pixel pair straddles m1 in slab 0, and the last pair of slab 1 is half)
GATHER = (
    case(32, 64, 2, 9, 11, stride=2, act=ACT_LRELU, fam="gather", P=1),
    case(32, 64, 2, 8, 10, stride=2, act=ACT_LRELU, fam="gather", P=1),
    case(64, 128, 1, 9, 11, stride=2, act=ACT_RELU, fam="gather", P=1),
    case(128, 64, 1, 5, 6, stride=2, tr=True, act=ACT_LRELU, fam="gather", P=1),
    case(128, 64, 2, 4, 5, stride=2, tr=True, fam="gather", P=1),
    case(8, 32, 2, 7, 9, act=ACT_RELU, rows=0, fam="direct"),
    case(24, 32, 1, 7, 9, rows=0, fam="direct"),
    case(40, 32, 1, 5, 9, act=ACT_LRELU, rows=0, fam="direct"),
    case(32, 8, 2, 7, 9, rows=0, rows_dgrad=0, fam="direct"),
    case(32, 24, 1, 7, 9, rows=0, rows_dgrad=0, fam="direct"),
    case(32, 40, 1, 5, 9, rows=0, rows_dgrad=0, fam="direct"),
    case(32, 64, 1, 34, 34, stride=2, parts="w", fam="gather", P=2),
)


def check_int_gather(device):
    """A on the gather kernels, GATHER: stride 2 with odd and even sizes, ConvTranspose2d with unequal residue classes,
    channel counts with a partial last K trip in the forward and in the dgrad, and a weight gradient of two slabs with an
    odd slab length (P asserted from the workspace).  All run on the emulator."""
    return _int_cases(device, GATHER, 7400)


# k_conv9x9_{fwd, dgrad, wgrad}_mfma and k_conv9_wgrad_reduce: 32 -> 3 and 64 -> 1 (two ci blocks).
#   9 x 57    the forward's tiles are 56 columns: a second tile of ONE column; 9 rows: a second tile row of one row
#   10 x 66   the gradients' tiles are 64 columns: a second tile of two columns
#   2 x 40 x 65   wgrad with 2 x 5 x 2 = 20 tile strips -> 80 slabs >= 64: k_conv9_wgrad_reduce splits them over 32
#                 workgroups that meet in dw through atomics (ysplit == 32); the smaller cases (8 to 32 slabs) reduce in one.
#                 H = 40: the last tile row is full, so the last strip's four slabs (one per wave = per two tile rows) all
#                 carry data - at H = 33 the last two would be zeros and a reduction that lost them would pass
CONV9 = (
    case(32, 3, 2, 9, 57, k=9, fam="conv9", P=4),
    case(32, 3, 2, 10, 66, k=9, fam="conv9", P=8),
    case(64, 1, 1, 9, 57, k=9, fam="conv9", P=2),
    case(64, 1, 1, 10, 66, k=9, bias=False, fam="conv9", P=4),
    case(32, 3, 2, 40, 65, k=9, parts="w", fam="conv9", P=20),
)


def check_int_conv9(device):
    """A on the 9x9 kernels, CONV9; the last case's P = 20 >= 16 (from the workspace) is what takes the reduction to
    its 32-way split.  The bias gradient is conv_colsum at C = 3 and C = 1.  All run on the emulator."""
    return _int_cases(device, CONV9, 7500)


# conv_direct.hip, and conv_colsum through db (C <= 8: k_colsum_small; above: k_colsum; the gather cases above are C = 64
# and 128, the 9x9 ones C = 3 and 1):
#   5 -> 8 stride 1 and 2; 6 -> 4 transposed; 4 -> 18 PixelShuffle(3); 4 -> 16 PixelShuffle(2); 8 -> 8 ReLU + residual;
#   4 -> 3 with a 9x9 kernel; 5 -> 8 at 1 x 257 x 257: 528392 outputs > 2048 workgroups x 256 threads, so the forward's
#   grid-stride loop takes a second trip (and the column sum has 259 row groups)
DIRECT = (
    case(5, 8, 2, 7, 9, rows=0, rows_dgrad=0, fam="direct"),
    case(5, 8, 2, 7, 9, stride=2, act=ACT_LRELU, fam="direct"),
    case(5, 8, 2, 8, 10, stride=2, act=ACT_LRELU, fam="direct"),
    case(6, 4, 2, 5, 6, stride=2, tr=True, act=ACT_LRELU, fam="direct"),
    case(4, 18, 2, 5, 4, act=ACT_LRELU, ps=3, rows=0, rows_dgrad=0, fam="direct"),
    case(4, 16, 2, 6, 7, act=ACT_LRELU, ps=2, res=True, rows=0, rows_dgrad=0, fam="direct"),
    case(8, 8, 2, 9, 9, act=ACT_RELU, res=True, rows=0, rows_dgrad=0, fam="direct"),
    case(4, 3, 2, 11, 13, k=9, fam="direct"),
    case(5, 8, 1, 257, 257, act=ACT_RELU, rows=0, rows_dgrad=0, fam="direct"),
)


def check_int_direct(device):
    """A on the direct kernels (forward with every epilogue, dgrad, the atomics-based wgrad) and on conv_colsum's two
    kernels, DIRECT.  All run on the emulator."""
    return _int_cases(device, DIRECT, 7600)


def _act_grad(t, act):
    """act'(t) as the kernels take it from a saved OUTPUT: 1 where t > 0, else the slope (0 stays on the slope side)."""
    slope = torch.tensor(0.0 if act == ACT_RELU else 0.2, dtype=torch.float32)
    return torch.where(t.to(torch.float32) > 0, torch.ones((), dtype=torch.float32), slope)


# (case, r): dasr_conv2d_dgrad_act of the layer, storing through the inverse PixelShuffle(r) map.
#   3x3: 8-row NT = 2 and NT = 1 with r = 1, 2, 3 (H, W multiples of r; ragged tiles), then the 16-row forms: 32 -> 16 at
#   16 x 64 x 128 (NT = 1 dgrad) with r = 1 and r = 2, and 64 -> 16 (NT = 2 dgrad), MI355X only
#   9x9: 32 -> 3 and 64 -> 1 at the forward's and the gradients' ragged sizes, r = 1 and r = 2
DGRAD_ACT = (
    (case(32, 64, 2, 8, 34, act=ACT_RELU, rows_dgrad=8), 1),
    (case(32, 32, 2, 16, 36, act=ACT_LRELU, rows_dgrad=8), 2),
    (case(64, 32, 2, 6, 33, act=ACT_LRELU, rows_dgrad=8), 3),
    (case(32, 16, 16, 64, 128, act=ACT_LRELU, rows_dgrad=16), 2),
    (case(32, 16, 16, 64, 128, act=ACT_RELU, rows_dgrad=16, emu=False), 1),
    (case(64, 16, 16, 64, 128, act=ACT_LRELU, rows_dgrad=16, emu=False), 2),
    (case(32, 3, 2, 9, 57, k=9, act=ACT_RELU), 1),
    (case(32, 3, 2, 10, 66, k=9, act=ACT_LRELU), 2),
    (case(64, 1, 1, 10, 66, k=9, act=ACT_LRELU), 1),
    (case(64, 1, 2, 12, 30, k=9, act=ACT_RELU), 2),
)


def check_int_dgrad_act(device):
    """A for dasr_conv2d_dgrad_act, DGRAD_ACT: float64 dgrad (integers) times act'(x_act) - for LeakyReLU ONE fp32 multiply
    by fp32(0.2) - taken through F.pixel_unshuffle.  x_act holds integers in [-2, 2]: a fifth of it is exactly zero and
    must take the slope side (asserted as a condition on the inputs, and that the dgrad is non-zero there).  Emulator: all
    but two of the three 16-row cases."""
    n = zeros_hit = 0
    for i, (c, r) in enumerate([(c, r) for c, r in DGRAD_ACT if c.emu or device != "cpu"]):
        assert_form(c)
        gen = torch.Generator().manual_seed(7700 + i)
        w, dy = _ints(gen, -2, 2, *_wshape(c)), _ints(gen, -2, 2, c.B, c.cout, c.H, c.W)
        x_act = _ints(gen, -2, 2, c.B, c.cin, c.H, c.W)
        wp, dyd, xa = _packed(w, c, device), _d(dy, device), _d(x_act, device)
        assert ops.conv2d_dgrad_act_supported(xa.shape, wp, dyd.shape, 1, c.pad, False, r)
        gx = F.conv_transpose2d(dy, w, None, stride=1, padding=c.pad)
        want = (gx.to(torch.float32) * _act_grad(x_act, c.act)).to(F64)
        zeros_hit += int(((x_act == 0) & (gx != 0)).sum())
        if r > 1:
            want = F.pixel_unshuffle(want, r)
        got = nchw(_take(ops.conv2d_dgrad_act(dyd, wp, xa, c.act, r, 1, c.pad, False)))
        assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
        bad = _nbad(got, want)
        assert bad == 0, ("dgrad_act mismatching elements", c, r, bad)
        n += 1
    assert zeros_hit > 0, "input condition: no exact zero of x_act meets a non-zero gradient"
    return {"cases": n, "zeros of x_act under a non-zero gradient": zeros_hit}


# dasr_conv2d_wgrad_act on the shapes without a fused kernel: epilogue backward into the scratch, then each family's wgrad
WGRAD_ACT = (
    case(64, 64, 2, 9, 33, act=ACT_RELU, fam="mfma"),
    case(32, 128, 1, 10, 35, act=ACT_LRELU, fam="mfma"),
    case(32, 64, 2, 9, 11, stride=2, act=ACT_LRELU, fam="gather"),
    case(128, 64, 1, 5, 6, stride=2, tr=True, act=ACT_RELU, fam="gather"),
    case(32, 3, 2, 9, 57, k=9, act=ACT_LRELU, fam="conv9"),
    case(5, 8, 2, 7, 9, act=ACT_LRELU, fam="direct"),
)


def check_int_wgrad_act(device):
    """A for dasr_conv2d_wgrad_act, WGRAD_ACT: dw and db of dconv = dy * act'(y) in float64, y holding integers in [-2, 2]
    (its zeros take the slope side).  ReLU: dy in [-2, 2].  LeakyReLU: dy * fp32(0.2) is no integer, and sums of such
    values are not exact in fp32 - except that fp32(5 t) * fp32(0.2) rounds to exactly t (5 * 0.2f = 1 + 2^-26; asserted):
    on the slope side dy is 5 t with t in [-2, 2], so dconv is integer everywhere while the kernel still has to apply the
    one multiply by fp32(0.2)."""
    five = torch.tensor([5.0, 10.0, -5.0, -10.0], dtype=torch.float32)
    assert torch.equal(five * SLOPE32, torch.tensor([1.0, 2.0, -1.0, -2.0]))
    lib = _lib.get()
    n = 0
    for i, c in enumerate(_on(device, WGRAD_ACT)):
        assert lib.dasr_conv2d_wgrad_act_fused(*_geom(c)) == 0, c
        wgrad_slabs(c)
        gen = torch.Generator().manual_seed(7800 + i)
        Ho, Wo = _out_hw(c)
        x, dy = _ints(gen, -2, 2, c.B, c.cin, c.H, c.W), _ints(gen, -2, 2, c.B, c.cout, Ho, Wo)
        y = _ints(gen, -2, 2, c.B, c.cout, Ho, Wo)
        if c.act == ACT_LRELU:
            dy = torch.where(y > 0, dy, 5.0 * dy)
        dconv = (dy.to(torch.float32) * _act_grad(y, c.act)).to(F64)
        assert torch.equal(dconv, dconv.round()) and float(dconv.abs().max()) <= 2 and int(((y == 0) & (dy != 0)).sum()) > 0
        _, gw, gb = _ref_g(x, torch.zeros(_wshape(c), dtype=F64), dconv, c)
        dw, db = ops.conv2d_wgrad_act(_d(x, device), _d(dy, device), _d(y, device), (c.k, c.k, c.cin, c.cout), c.act,
                                      c.stride, c.pad, c.tr)
        bad = {"dw": _nbad(_dw_torch(_take(dw), c), gw), "db": _nbad(_take(db), gb)}
        assert not any(bad.values()), ("wgrad_act mismatching elements", c, bad)
        n += 1
    return {"cases": n}


# (B, H, W, Cin, Cout, tile rows): the fused statistics epilogue (W % 32 == 0) and the th-dependent partial records
#   (2, 16, 32, 64, 64)     two tile rows of 8, NT = 2
#   (1, 21, 64, 64, 64)     a ragged third tile row (5 of 8 rows): unequal counts in the Chan merges
#   (2, 40, 32, 32, 32)     NT = 1, five tile rows
#   (16, 64, 128, 16, 32)   16-row tiles, NT = 1 (as CONV3_16ROW)
#   (4, 64, 128, 16, 256)   16-row tiles, NT = 2; MI355X only
#   (2, 9, 20, 64, 64), (1, 16, 32, 8, 32)   the fallback: W % 32 != 0; not an MFMA shape (rows = 0)
FWD_STATS = ((2, 16, 32, 64, 64, 8, True), (1, 21, 64, 64, 64, 8, True), (2, 40, 32, 32, 32, 8, True),
             (16, 64, 128, 16, 32, 16, True), (4, 64, 128, 16, 256, 16, False), (2, 9, 20, 64, 64, 8, True),
             (1, 16, 32, 8, 32, 0, True))
GUARD_FLOATS, GUARD_VALUE = 64, 12345.0


def check_int_fwd_stats(device):
    """A for dasr_conv2d_fwd_stats, FWD_STATS: y (integer operands, bias) equals float64 in every element; mean and var
    against float64 statistics of that exact y under the gates of check_conv_fwd_stats (|mean err| / (|mean| + std) <=
    2e-6, |var err| / var <= 2e-5).  The workspace is exactly dasr_conv2d_fwd_stats_workspace() bytes, followed by guard
    floats that must come back untouched (the 16-row forms write fewer, larger tile records than the 8-row ones: a size
    computed for the other tile height would not fit), and four bytes less is refused."""
    lib = _lib.get()
    n, worst_m, worst_v = 0, 0.0, 0.0
    for i, (B, H, W, cin, cout, rows, on_emu) in enumerate(FWD_STATS):
        if device == "cpu" and not on_emu:
            continue
        c = case(cin, cout, B, H, W, parts="y", rows=rows)
        assert_form(c)
        x, w, _, bias, _, _ = _int_operands(c, 7900 + i)
        xd, wp, bd = _d(x, device), _packed(w, c, device), bias.to(torch.float32).to(device)
        nbytes = int(lib.dasr_conv2d_fwd_stats_workspace(B, H, W, cin, cout))
        assert nbytes > 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + GUARD_FLOATS,), GUARD_VALUE).to(device)
        y, mean, var = ops.empty((B, H, W, cout), xd), ops.empty((B, cout), xd), ops.empty((B, cout), xd)
        for t in (y, mean, var):
            _poison(t)
        args = (ops._p(xd), ops._p(wp), ops._p(bd), ops._p(y), ops._p(mean), ops._p(var), ops._p(ws))
        try:
            ops._call("dasr_conv2d_fwd_stats", *args, nbytes - 4, B, H, W, cin, cout)
            raise AssertionError("a workspace four bytes short was accepted")
        except RuntimeError as e:
            assert "workspace too small" in str(e), str(e)
        ops._call("dasr_conv2d_fwd_stats", *args, nbytes, B, H, W, cin, cout)
        assert torch.equal(ws[nbytes // 4:].cpu(), torch.full((GUARD_FLOATS,), GUARD_VALUE)), ("write past the workspace", c)
        y_ref = _ref_y(x, w, bias, None, c)
        bad = _nbad(nchw(_take(y)), y_ref)
        assert bad == 0, ("fwd_stats y mismatching elements", c, bad)
        yt = y_ref.reshape(B, cout, H * W)
        mt, vt = yt.mean(2), yt.var(2, unbiased=False)
        em = ((_take(mean).to(F64) - mt).abs() / (mt.abs() + vt.sqrt())).max().item()
        ev = ((_take(var).to(F64) - vt).abs() / vt).max().item()
        print("fwd_stats %-22s rows %2d  mean err %.2e  var err %.2e" % ((B, H, W, cin, cout), rows, em, ev))
        assert em <= 2e-6 and ev <= 2e-5, (c, em, ev)
        worst_m, worst_v, n = max(worst_m, em), max(worst_v, ev), n + 1
    return {"cases": n, "worst mean err": worst_m, "worst var err": worst_v}


# =====================================================================================================================
# B. full-mantissa pass-through
# =====================================================================================================================
def _round_once(a, b, what):
    """fp32(a + b) of two float64 tensors holding fp32 values, rounded ONCE.  s = a + b in float64 is exact or itself a
    rounding; rounding s again to float32 equals rounding the exact sum unless s is inexact AND sits exactly on a float32
    tie (an exact s on a tie is rounded to even here as in the kernel).  That case is asserted not to occur: the
    inexactness is the error term of Knuth's TwoSum."""
    s = a + b
    bb = s - a
    inexact = ((a - (s - bb)) + (b - bb)) != 0
    r = s.to(torch.float32)
    d = (s - r.to(F64)).abs()
    for toward in (float("inf"), -float("inf")):
        half = (torch.nextafter(r, torch.full_like(r, toward)).to(F64) - r.to(F64)).abs() / 2
        assert not bool(((d == half) & inexact).any()), ("inexact float64 sum on a float32 tie", what)
    return r.to(F64)


def _mantissa(gen, C, *shape):
    """fp32 values with full 24-bit mantissas, none zero, whose magnitudes spread over 2^-30 .. 2^30 with the channel
    (dimension 1), as float64."""
    v = torch.randn(*shape, generator=gen)
    v[v == 0] = 1.0
    e = ((torch.arange(C) * 7) % 61 - 30).to(torch.float32)
    v = v * (2.0 ** e).view(1, C, *([1] * (len(shape) - 2)))
    assert bool(torch.isfinite(v).all()) and bool((v.abs() >= 2.0 ** -100).all())
    return v.to(F64)


def _one_hot_kernel(c, produced):
    """A kernel with exactly ONE non-zero, +-2^e (e in -4 .. 4), per PRODUCED channel (``produced`` = "cout": the forward;
    "cin": the dgrad), at a tap and a reduction channel that cycle with that channel.  torch's layout."""
    w = torch.zeros(_wshape(c), dtype=F64)
    kk = c.k * c.k
    n_p, n_r = (c.cout, c.cin) if produced == "cout" else (c.cin, c.cout)
    for p in range(n_p):
        tap, red = (p * 4 + p // kk) % kk, (5 * p + 1) % n_r
        val = (-1.0 if p % 2 else 1.0) * 2.0 ** (p % 9 - 4)
        co, ci = (p, red) if produced == "cout" else (red, p)
        if c.tr:
            w[ci, co, tap // c.k, tap % c.k] = val
        else:
            w[co, ci, tap // c.k, tap % c.k] = val
    return w


def _mantissa_cases(device, cases, seed0):
    n = 0
    for i, c in enumerate(_on(device, cases)):
        assert_form(c)
        gen = torch.Generator().manual_seed(seed0 + i)
        Ho, Wo = _out_hw(c)
        x, dy = _mantissa(gen, c.cin, c.B, c.cin, c.H, c.W), _mantissa(gen, c.cout, c.B, c.cout, Ho, Wo)
        bias, base = torch.randn(c.cout, generator=gen).to(F64), torch.randn(c.B, c.cin, c.H, c.W, generator=gen).to(F64)
        bad = {}
        if "y" in c.parts:
            w = _one_hot_kernel(c, "cout")
            y = run_ops(device, c._replace(parts="y"), x, w, bias, None, dy, base)[0]
            pure = _conv64(x, w, None, c)
            assert torch.equal(pure.to(torch.float32).to(F64), pure)            # one term: 2^e x, a float32
            bad["y"] = _nbad(y, _round_once(pure, bias.view(1, -1, 1, 1).expand_as(pure), ("y", c)))
        if "x" in c.parts:
            w = _one_hot_kernel(c, "cin")
            _, dx, acc, _, _ = run_ops(device, c._replace(parts="x"), x, w, None, None, dy, base)
            gx = _ref_g(x, w, dy, c, "x" if c.stride == 1 and not c.tr else "xw")[0]
            assert torch.equal(gx.to(torch.float32).to(F64), gx) and int((gx != 0).sum()) > gx.numel() // 8
            bad["dx"], bad["dx_acc"] = _nbad(dx, gx), _nbad(acc, _round_once(gx, base, ("dx_acc", c)))
        assert not any(bad.values()), ("full-mantissa mismatching elements", c, bad)
        n += 1
    return {"cases": n}


# one shape per kernel form (the table of A, its smallest members); bias on, no activation
MANTISSA_FWD_DGRAD = (
    case(64, 64, 2, 17, 33, parts="yx", rows=8, rows_dgrad=8),
    case(16, 32, 2, 8, 34, parts="yx", rows=8, rows_dgrad=0),
    case(32, 32, 1, 8, 34, parts="yx", rows=8, rows_dgrad=8),
    case(16, 32, 16, 64, 128, parts="y", rows=16),
    case(32, 16, 16, 64, 128, parts="x", rows_dgrad=16),
    case(16, 256, 4, 64, 128, parts="y", rows=16, emu=False),
    case(256, 16, 4, 64, 128, parts="x", rows_dgrad=16, emu=False),
    case(32, 64, 2, 9, 11, stride=2, parts="yx"),
    case(128, 64, 1, 5, 6, stride=2, tr=True, parts="yx"),
    case(24, 32, 1, 7, 9, parts="yx", rows=0),
    case(32, 24, 1, 7, 9, parts="yx", rows=0, rows_dgrad=0),
    case(32, 3, 2, 9, 57, k=9, parts="yx"),
    case(64, 1, 1, 10, 66, k=9, parts="yx"),
    case(5, 8, 2, 7, 9, parts="yx", rows=0, rows_dgrad=0),
    case(6, 4, 2, 5, 6, stride=2, tr=True, parts="yx"),
)


def check_mantissa_fwd_dgrad(device):
    """B for the forward and the dgrad, MANTISSA_FWD_DGRAD.  x (dy for the dgrad) is arbitrary fp32 without zeros, its
    magnitude spread over 2^-30 .. 2^30 with the channel; the kernel has one non-zero +-2^e per produced channel
    (_one_hot_kernel).  Then y[co] = fp32(+-2^e x[ci, shifted] + bias[co]): ONE rounding, whatever the summation order
    (every other term is x * 0 = 0), and dx[ci] = +-2^e dy[co, shifted] with none (accumulating: fp32(dx + base)).
    Numeric equality on every element (+0 and -0 alike).  Emulator: every form but the NT = 2 16-row ones."""
    return _mantissa_cases(device, MANTISSA_FWD_DGRAD, 8100)


def _impulse_pixels(Ho, Wo):
    """Corners, both sides of the seams of 2-, 4-, 8-row x 32- and 64-column tiles, and the middle."""
    pix = [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (1, 31), (2, 32), (3, 31), (4, 32), (7, 31), (8, 32),
           (7, 63), (8, 64), (Ho // 2, Wo // 2)]
    return [(min(py, Ho - 1), min(px, Wo - 1)) for py, px in pix]


MANTISSA_WGRAD = (
    case(64, 64, 2, 17, 33, parts="w", fam="mfma"),
    case(32, 128, 2, 10, 35, parts="w", fam="mfma"),
    case(32, 32, 1, 8, 34, parts="w", fam="mfma"),
    case(64, 32, 1, 9, 33, parts="w", fam="mfma"),
    case(32, 64, 1, 9, 33, parts="w", fam="mfma"),
    case(32, 64, 1, 34, 34, stride=2, parts="w", fam="gather", P=2),
    case(128, 64, 1, 5, 6, stride=2, tr=True, parts="w", fam="gather"),
    case(32, 3, 2, 40, 65, k=9, parts="w", fam="conv9", P=20),
    case(64, 1, 1, 10, 66, k=9, parts="w", fam="conv9"),
    case(5, 8, 2, 7, 9, parts="w", fam="direct"),
    case(6, 4, 2, 5, 6, stride=2, tr=True, parts="w", fam="direct"),
)


def check_mantissa_wgrad(device):
    """B for the weight gradient, MANTISSA_WGRAD: x as in the forward check; dy is ONE impulse +-2^e per output channel,
    in a sample and at a pixel that cycle with the channel over _impulse_pixels (corners and tile seams).  Then
    dw[co, ci, tap] = +-2^e x[ci, p + tap] exactly (0 outside the image) through every slab, reduction and atomic, and
    db[co] = +-2^e.  Numeric equality on every element.  All run on the emulator."""
    n = 0
    for i, c in enumerate(_on(device, MANTISSA_WGRAD)):
        assert_form(c)
        gen = torch.Generator().manual_seed(8200 + i)
        Ho, Wo = _out_hw(c)
        x = _mantissa(gen, c.cin, c.B, c.cin, c.H, c.W)
        pix = _impulse_pixels(Ho, Wo)
        w0 = torch.zeros(_wshape(c), dtype=F64)
        # the 9x9 layers have three and one output channel: three runs, so that the first and the last corner (the last
        # sample's: the last strip's last slab) and a seam are met
        for shift in ((0,) if c.cout >= len(pix) else (0, 3, 8)):
            dy = torch.zeros(c.B, c.cout, Ho, Wo, dtype=F64)
            for co in range(c.cout):
                py, px = pix[(co + co // len(pix) + shift) % len(pix)]
                dy[(co + shift) % c.B, co, py, px] = (-1.0 if co % 2 else 1.0) * 2.0 ** (co % 9 - 4)
            _, gw, gb = _ref_g(x, w0, dy, c)
            assert torch.equal(gw.to(torch.float32).to(F64), gw) and int((gw != 0).sum()) > gw.numel() // 16
            _, _, _, dw, db = run_ops(device, c, x, w0, None, None, dy, torch.zeros_like(x))
            bad = {"dw": _nbad(dw, gw), "db": _nbad(db, gb)}
            assert not any(bad.values()), ("full-mantissa wgrad mismatching elements", c, shift, bad)
            n += 1
    return {"runs": n}


# =====================================================================================================================
# C. the derived per-element bound
# =====================================================================================================================
U = 2.0 ** -24
BOUND_SETS = ("plain", "in-ladder", "col-ladder", "out-ladder", "rand")


def gamma(n):
    return n * U / (1.0 - n * U)


def _bound_operands(c, kind, seed):
    """x, w (OIHW), bias, dy, residual, base as float64 holding fp32 values: the sets of make_operands, or 'rand'
    (all-positive: nothing cancels, so one lost term out of n shows as 1 / n of the magnitude)."""
    Ho, Wo = _out_hw(c)
    if kind == "rand":
        gen = torch.Generator().manual_seed(seed)
        rd = lambda *s: torch.rand(*s, generator=gen)
        x, dy = rd(c.B, c.cin, c.H, c.W), rd(c.B, c.cout, Ho, Wo)
        w, bias = rd(*_wshape(c)) / math.sqrt(c.k * c.k * c.cin), rd(c.cout) * 0.3
    else:
        op = make_operands(kind, c.cin, c.cout, c.k, c.B, c.H, c.W, seed)
        x, w, bias = op["x"], op["w"], op["bias"]
        dy = op["dy"][:, :, :Ho, :Wo].contiguous()          # (a strided layer's dy is the top-left part of the set's)
    gen = torch.Generator().manual_seed(seed + 1)
    draw = (lambda *s: torch.rand(*s, generator=gen)) if kind == "rand" else (lambda *s: torch.randn(*s, generator=gen))
    res = draw(c.B, c.cout, Ho, Wo) if c.res else None
    base = draw(c.B, c.cin, c.H, c.W)
    assert all(t is None or t.dtype == torch.float32 for t in (x, w, bias, dy, res, base))
    return [None if t is None else t.to(F64) for t in (x, w, bias, dy, res, base)]


# one shape per kernel form, the smallest of A's table; no activation, bias, a residual where the family has one
BOUND = (
    case(32, 32, 1, 8, 34, res=True, rows=8, rows_dgrad=8, fam="mfma"),
    case(64, 64, 2, 17, 33, rows=8, rows_dgrad=8, fam="mfma"),
    case(32, 64, 2, 9, 11, stride=2, fam="gather"),
    case(32, 64, 1, 34, 34, stride=2, parts="w", fam="gather", P=2),
    case(24, 32, 1, 7, 9, rows=0, fam="direct"),
    case(32, 3, 2, 9, 57, k=9, fam="conv9"),
    case(32, 3, 2, 40, 65, k=9, parts="w", fam="conv9", P=20),
    case(5, 8, 2, 7, 9, res=True, rows=0, fam="direct"),
)
# the 16-row forms of k_conv3x3_mfma (CONV3_16ROW has the arithmetic of the shapes), NT = 1 and NT = 2; the emulator runs
# them on fewer operand sets (12 s and 24 s a run there)
BOUND_16ROW_NT1 = (
    case(16, 32, 16, 64, 128, res=True, parts="y", rows=16),
    case(32, 16, 16, 64, 128, parts="x", rows_dgrad=16),
)
BOUND_16ROW_NT2 = (
    case(16, 256, 4, 64, 128, parts="y", rows=16),
    case(256, 16, 4, 64, 128, parts="x", rows_dgrad=16, emu=False),
)


def _form_name(c):
    tag = "%dx%d %d->%d" % (c.k, c.k, c.cin, c.cout) + (" s%d" % c.stride if c.stride > 1 else "")
    rows = c.rows or c.rows_dgrad
    return tag + (" %d-row" % rows if rows else "") + " %dx%dx%d" % (c.B, c.H, c.W)


def _bound_cases(device, cases, seed0, emu_sets=BOUND_SETS):
    """C: |kernel - float64| <= gamma_n * mag in every element, gamma_n = n 2^-24 / (1 - n 2^-24), on ``cases`` x BOUND_SETS (on the
    emulator: x ``emu_sets``).
      mag   the float64 convolution of the absolute operands, plus |bias| and |residual| (forward), |base| (the
            accumulating dgrad)
      n     terms + 3:  K K Cin (forward),  ceil(K / stride)^2 Cout (dgrad),  B Ho Wo (wgrad, db)
    This is the any-order bound of fp32 summation (each of n terms passes through at most n - 1 additions and one
    multiplication, each within 2^-24 relative; + 3 covers bias, residual / base and slack for the product): derived, not
    measured, and with no margin on top.  An element is judged against ITS OWN magnitude, so a wrong value in a plane
    2^-20 below the tensor's maximum (the ladder sets) cannot hide.  float64's own error, about n 2^-53 mag, is 2^-29 of
    the bound.  Returns and prints the worst error / bound per form.
    (The figures measured on the emulator and on the MI355X: DESIGN.md 2, "exact-fp32 op tests".)"""
    worst = {}
    for i, c in enumerate(_on(device, cases)):
        assert_form(c)
        Ho, Wo = _out_hw(c)
        n_y, n_x, n_w = c.k * c.k * c.cin + 3, math.ceil(c.k / c.stride) ** 2 * c.cout + 3, c.B * Ho * Wo + 3
        for si, kind in enumerate(BOUND_SETS):
            if device == "cpu" and kind not in emu_sets:
                continue
            x, w, bias, dy, res, base = _bound_operands(c, kind, seed0 + 10 * i + si)
            y, dx, acc, dw, db = run_ops(device, c, x, w, bias, res, dy, base)
            items = {}
            if "y" in c.parts:
                mag = _conv64(x.abs(), w.abs(), bias.abs(), c) + (res.abs() if res is not None else 0.0)
                items["y"] = (y, _ref_y(x, w, bias, res, c, exact_lrelu=False), gamma(n_y) * mag)
            if "x" in c.parts or "w" in c.parts:
                gx, gw, gb = _ref_g(x, w, dy, c, c.parts)
                mx, mw, mb = _ref_g(x.abs(), w.abs(), dy.abs(), c, c.parts)
                if "x" in c.parts:
                    items["dx"] = (dx, gx, gamma(n_x) * mx)
                    items["dx_acc"] = (acc, gx + base, gamma(n_x) * (mx + base.abs()))
                if "w" in c.parts:
                    items["dw"], items["db"] = (dw, gw, gamma(n_w) * mw), (db, gb, gamma(n_w) * mb)
            for nm, (got, ref, bound) in items.items():
                err = (got.to(F64) - ref).abs()
                ok = err <= bound
                ratio = float((err / bound.clamp_min(1e-300)).max())
                key = "%s %s" % (_form_name(c), nm)
                worst[key] = max(worst.get(key, 0.0), ratio)
                assert bool(ok.all()), ("per-element bound", c, kind, nm, "elements over", int((~ok).sum()),
                                        "worst error / bound", ratio)
    for k in sorted(worst):
        print("fp32 bound  %-40s worst error / bound = %.4f" % (k, worst[k]))
    return {k: round(v, 4) for k, v in worst.items()}


def check_bound(device):
    """C (_bound_cases has the bound and its derivation) on BOUND x BOUND_SETS: one shape per kernel form but the 16-row
    ones.  All run on the emulator."""
    return _bound_cases(device, BOUND, 8300)


def check_bound_16row_nt1(device):
    """C on the 16-row NT = 1 forward and dgrad, BOUND_16ROW_NT1.  Emulator: the out-ladder and the all-positive set;
    MI355X: all five."""
    return _bound_cases(device, BOUND_16ROW_NT1, 8600, emu_sets=("out-ladder", "rand"))


def check_bound_16row_nt2(device):
    """C on the 16-row NT = 2 forward and dgrad, BOUND_16ROW_NT2.  Emulator: the forward on the all-positive set;
    MI355X: both, all five sets."""
    return _bound_cases(device, BOUND_16ROW_NT2, 8700, emu_sets=("rand",))
