"""Range and per-plane checks of the fp16 x 2 split convolutions (csrc/conv_split_bf16.hip NP = 2, csrc/conv9_split.hip).
check_split_conv / check_conv9_split draw well-scaled randn operands and measure max|err| / max|ref| over the whole tensor;
the scheme scales every TENSOR by one power of two, so its weak spot is the quiet part of a tensor (channels, frames, the
surroundings of an outlier far below the maximum), and every 64 -> 64 convolution of a DGB feeds an InstanceNorm that turns
the absolute error of a quiet plane into a relative one.  Here:
  * a float64 MODEL of the scheme written from the kernels' header comment (split2_model) - kernels are compared with IT,
    per output plane, so that a lost piece or a wrong exponent shows as an error of 2^-11 .. 2^-1, not inside fp32 noise;
  * adversarial operand sets (make_operands): channel ladders down to 2^-20, a dark frame, an outlier on a tile seam, zeros,
    maxima at a power of two;
  * the model itself against float64 and the bound its arithmetic implies (no kernel involved);
  * exactness properties (zeros, power-of-two equivariance).
Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_split_range.py runs them.  Every
form runs with set_conv_bf16_impl(0) only (the alternative forms stay with check_split_conv)."""
import math

import torch
import torch.nn.functional as F

from dasr_amd import graph, ops, synth
from oracle import depthnet_oracle as O
from tests.parity_checks import ZERO_GRAD_KEYS, _compare_with_oracle, _oracle_sd, build_net, nchw, nhwc, rel_max

F64 = torch.float64
INF = float("inf")
# Bands of plane level log2(max|ref_plane| / max|ref|): [0,-6), [-6,-14), [-14,-18), below -18.  x1 stays a normal fp16
# number down to 2^-18 of the tensor's maximum (kernel header), so the last band is where the scheme gives up precision.
BAND_EDGES = (-6.0, -14.0, -18.0)
BAND_NAMES = ("0..-6", "-6..-14", "-14..-18", "<-18")
MIN_POOL = 8          # planes a band needs to be compared on its own: the count the issue asks of the ladder cases

# (a) / (c): worst band ratio  max_planes E(split kernel vs model) / max_planes E(exact-fp32 kernel vs float64), per
# device, over every form and operand set of this file; the gate is 2x the measured worst (maxima over ~100 planes are
# extreme-value statistics that move with the seed).  DESIGN.md 4.11 holds the per-form, per-band figures.
#   emulator : measured worst 2.57 (9x9 dgrad, output-channel ladder, band -14..-18) -> gate 5.14
#   MI355X   : measured worst 1.92 (3x3 64 -> 64 forward, maximum exactly 2^3; every other case <= 1.32) -> gate 3.84
RATIO_GATE = {"cpu": 2 * 2.57, "cuda": 2 * 1.92}
# the same for (c), the error against float64 over the plane's own standard deviation (what the InstanceNorm sees), in the
# bands down to -14 (below: the floor of (b) plus the fp32 kernel's error times this gate)
#   emulator : measured worst 2.31 (9x9 dgrad, maximum at 2^3) -> gate 4.62
#   MI355X   : measured worst 1.06 (9x9 accumulating dgrad) -> gate 2.12
NORM_GATE = {"cpu": 2 * 2.31, "cuda": 2 * 1.06}


# =====================================================================================================================
# The float64 model
# =====================================================================================================================
def scale_exp(t):
    """k of the scale 2^k of a tensor: 14 - floor(log2 max|t|), clamped to [-60, 60]; an all-zero tensor gets 60."""
    m = float(t.abs().max())
    if m == 0.0:
        return 60
    k = 14 - (math.frexp(m)[1] - 1)             # m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    return max(-60, min(60, k))


def pieces(t):
    """(t0, t1, s): t0 = fp16(t s), t1 = fp16(t s - t0) as float64, round-to-nearest float16.  t s and t s - t0 are exact in
    fp32 (s is a power of two, t0 holds the leading bits of t s), so each piece is ONE rounding."""
    s = 2.0 ** scale_exp(t)
    ts = t.to(F64) * s
    t0 = ts.float().half().to(F64)
    t1 = (ts - t0).float().half().to(F64)
    return t0, t1, s


def bilinear(kind, a, b, pad):
    """The three bilinear forms of a stride-1 convolution, NCHW float64: 'fwd' (x, w) -> y; 'dgrad' (dy, w) -> dx;
    'wgrad' (x, dy) -> dw [Cout, Cin, k, k]."""
    if kind == "fwd":
        return F.conv2d(a, b, padding=pad)
    if kind == "dgrad":
        return F.conv_transpose2d(a, b, padding=pad)
    assert kind == "wgrad"
    return F.conv2d(a.transpose(0, 1), b.transpose(0, 1), padding=pad).transpose(0, 1)


def split2_model(kind, a, b, pad, drop_a1b0=False, scale_mul=1.0):
    """a0 (*) b0 + a0 (*) b1 + a1 (*) b0 in float64, divided by s(a) s(b).  The two keyword arguments exist for the mutation
    check only (a lost piece, a wrong exponent): tests never pass them."""
    a0, a1, sa = pieces(a)
    b0, b1, sb = pieces(b)
    acc = bilinear(kind, a0, b0, pad) + bilinear(kind, a0, b1, pad)
    if not drop_a1b0:
        acc = acc + bilinear(kind, a1, b0, pad)
    return acc / (sa * sb * scale_mul)


def operand_delta(t):
    """Per element, what two fp16 pieces can miss of t: max(2^-22 |t|, 2^-25 / s(t)) - the second rounding is to 11 bits of
    a remainder <= 2^-11 |t s|, or to the fp16 subnormal spacing 2^-24 in scaled units."""
    s = 2.0 ** scale_exp(t)
    return torch.maximum(t.to(F64).abs() * 2.0 ** -22, torch.full_like(t, 2.0 ** -25 / s, dtype=F64))


def scheme_floor(kind, a, b, pad):
    """Bound on |model - float64| per element: conv(da, |b|) + conv(|a|, db) + 2^-22 conv(|a|, |b|) (the dropped a1 b1).
    Times 1 + 2^-9 for what the first-order form leaves out: da db, and |a1| <= 2^-11 |a s| + 2^-24 where a0 is subnormal."""
    a, b = a.to(F64), b.to(F64)
    fl = (bilinear(kind, operand_delta(a), b.abs(), pad) + bilinear(kind, a.abs(), operand_delta(b), pad)
          + 2.0 ** -22 * bilinear(kind, a.abs(), b.abs(), pad))
    return fl * (1.0 + 2.0 ** -9)


# =====================================================================================================================
# Operand sets
# =====================================================================================================================
def ladder(C):
    return 2.0 ** (-20.0 * torch.arange(C, dtype=F64) / (C - 1)).float()


def make_operands(kind, cin, cout, k, B, H, W, seed, seam=None, p=None):
    """dict(x, w, bias, dy) as NCHW / OIHW fp32 CPU tensors.  Ladders: 'in' on the layer's INPUT channels - x for the
    forward and the wgrad, the kernel's input columns ('col-ladder') for the dgrad, whose operands are dy and the kernel and
    whose output planes are those channels; 'out' on its OUTPUT channels (the kernel's rows and the bias, and dy)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, dy = rn(B, cin, H, W), rn(B, cout, H, W)
    w = rn(cout, cin, k, k) / math.sqrt(k * k * cin)
    bias = rn(cout) * 0.3
    if kind == "in-ladder":
        x = x * ladder(cin).view(1, cin, 1, 1)
    elif kind == "col-ladder":
        w = w * ladder(cin).view(1, cin, 1, 1)
    elif kind == "out-ladder":
        w = w * ladder(cout).view(cout, 1, 1, 1)
        bias = bias * ladder(cout)
        dy = dy * ladder(cout).view(1, cout, 1, 1)
    elif kind == "frame":
        assert B >= 2
        x[1] *= 2.0 ** p
        dy[1] *= 2.0 ** p
    elif kind == "outlier":
        (ya, xa), (yb, xb) = seam
        x[0, 1, ya, xa] = 2.0 ** p
        dy[0, 2, yb, xb] = -2.0 ** p
    elif kind == "boundary":         # maximum exactly 2^3 (p = 0) or the float below it (p = 1)
        top = 8.0 if p == 0 else float(torch.nextafter(torch.tensor(8.0), torch.tensor(0.0)))
        for t in (x, dy, w):
            t.clamp_(-7.0, 7.0)
            t.view(-1)[t.numel() // 3] = -top
        assert float(x.abs().max()) == top and float(w.abs().max()) == top
    else:
        assert kind == "plain"
    return dict(x=x, w=w, bias=bias, dy=dy)


# =====================================================================================================================
# Kernel forms: each returns (split result, exact-fp32 kernel's result) as NCHW (wgrad: OIHW) float64 CPU tensors
# =====================================================================================================================
def _cpu64(t, layout):
    t = t.detach().cpu().to(F64)
    return nchw(t) if layout == "nhwc" else t.permute(3, 2, 0, 1).contiguous()


class Kernels:
    """The operands of one case on the device, and the kernel calls on them (3x3 or 9x9 by the kernel's size)."""

    def __init__(self, device, op, act=0, ps=1):
        self.k = op["w"].shape[2]
        self.pad = self.k // 2
        self.cout = op["w"].shape[0]
        self.act, self.ps = act, ps
        self.x, self.dy = nhwc(op["x"]).to(device), nhwc(op["dy"]).to(device)
        self.wp = ops.pack_hwio(op["w"].permute(2, 3, 1, 0).contiguous().to(device))
        self.bias = op["bias"].to(device) if op["bias"] is not None else None
        self.xm, self.dm = ops.absmax(self.x), ops.absmax(self.dy)
        if self.k == 3:
            self.ws = ops.conv3x3_split2_weights(self.wp)
        else:
            self.wm = ops.absmax(self.wp[0])

    def fwd(self, amax=None):
        if self.k == 3:
            return ops.conv3x3_fwd_split2(self.x, self.xm, self.ws, self.bias, self.cout, None, self.act, self.ps, amax=amax)
        return ops.conv9_fwd_split2(self.x, self.xm, self.wp, self.wm, self.bias)

    def fwd32(self):
        return ops.conv2d_fwd(self.x, self.wp, self.bias, None, 1, self.pad, False, self.act, self.ps)

    def dgrad(self, out=None):
        if self.k == 3:
            return ops.conv3x3_dgrad_split2(self.dy, self.dm, self.ws, self.x.shape, out=out)
        return ops.conv9_dgrad_split2(self.dy, self.dm, self.wp, self.wm, self.x.shape, out=out)

    def dgrad32(self, out=None):
        return ops.conv2d_dgrad(self.dy, self.wp, self.x.shape, pad=self.pad, out=out)

    def wgrad(self):
        if self.k == 3:
            return ops.conv3x3_wgrad_split2(self.x, self.xm, self.dy, self.dm)
        return ops.conv9_wgrad_split2(self.x, self.xm, self.dy, self.dm)

    def wgrad32(self):
        return ops.conv2d_wgrad(self.x, self.dy, (self.k, self.k, self.x.shape[3], self.cout), pad=self.pad)


def _epilogue(t, act, ps, magnitude=False):
    """PixelShuffle(ps) and LeakyReLU(0.2) of the fused forward epilogue on a float64 NCHW tensor (a magnitude is only
    shuffled: the activation never enlarges an error)."""
    if ps > 1:
        t = F.pixel_shuffle(t, ps)
    if act == 2 and not magnitude:
        t = F.leaky_relu(t, 0.2)
    return t


def run_form(form, kn, op, base=None):
    """One kernel form on one operand set: dict(y_sp, y_32, ref, model, mag, floor), all float64 CPU, planes in the first
    two dimensions.  ref = plain float64, model = split2_model, mag = conv(|a|, |b|) (+ |bias|, + |base|), floor = (b)."""
    x, w, dy = op["x"].to(F64), op["w"].to(F64), op["dy"].to(F64)
    pad = kn.pad
    if form == "fwd":
        a, b, kind, add = x, w, "fwd", (op["bias"].to(F64).view(1, -1, 1, 1) if op["bias"] is not None else None)
        y_sp, y_32 = _cpu64(kn.fwd(), "nhwc"), _cpu64(kn.fwd32(), "nhwc")
    elif form in ("dgrad", "dgrad_acc"):
        a, b, kind, add = dy, w, "dgrad", None
        if form == "dgrad":
            y_sp, y_32 = _cpu64(kn.dgrad(), "nhwc"), _cpu64(kn.dgrad32(), "nhwc")
        else:
            add = base.to(F64)
            o_sp, o_32 = nhwc(base).to(kn.x.device), nhwc(base).to(kn.x.device)
            kn.dgrad(out=o_sp)
            kn.dgrad32(out=o_32)
            y_sp, y_32 = _cpu64(o_sp, "nhwc"), _cpu64(o_32, "nhwc")
    else:
        assert form == "wgrad"
        a, b, kind, add = x, dy, "wgrad", None
        (dw_sp, db_sp), (dw_32, db_32) = kn.wgrad(), kn.wgrad32()
        y_sp, y_32 = _cpu64(dw_sp, "hwio"), _cpu64(dw_32, "hwio")
        gb = dy.sum((0, 2, 3))
        # the bias gradient is a plain fp32 sum in both kernels (no pieces): the bound check_split_conv holds it to
        assert rel_max(db_sp, gb) <= 2 * rel_max(db_32, gb) + 1e-6, ("dbias", rel_max(db_sp, gb), rel_max(db_32, gb))
    ref, model = bilinear(kind, a, b, pad), split2_model(kind, a, b, pad)
    mag, floor = bilinear(kind, a.abs(), b.abs(), pad), scheme_floor(kind, a, b, pad)
    if add is not None:
        ref, model, mag = ref + add, model + add, mag + add.abs()
    if form == "fwd":
        ref, model = _epilogue(ref, kn.act, kn.ps), _epilogue(model, kn.act, kn.ps)
        mag, floor = _epilogue(mag, kn.act, kn.ps, True), _epilogue(floor, kn.act, kn.ps, True)
    assert y_sp.shape == ref.shape == y_32.shape, (y_sp.shape, y_32.shape, ref.shape)
    assert bool(torch.isfinite(y_sp).all())
    return dict(y_sp=y_sp, y_32=y_32, ref=ref, model=model, mag=mag, floor=floor)


# =====================================================================================================================
# Per-plane, band-wise analysis
# =====================================================================================================================
def _pmax(t):
    return t.abs().flatten(2).amax(2)


def plane_bands(ref):
    """Band index (0..3) of every plane of a float64 reference, from log2(max|plane| / max|tensor|)."""
    lvl = torch.log2(_pmax(ref) / ref.abs().max())
    band = torch.zeros_like(lvl, dtype=torch.long)
    for e in BAND_EDGES:
        band += (lvl < e).long()
    return band


def analyse(r, with_norm):
    """Band-wise maxima over planes.  (a): E = max|y - model| / max mag for the split kernel, max|y - ref| / max mag for the
    exact-fp32 kernel.  (c): max|y - ref| / std(ref plane) for both, and the floor of (b) in the same units."""
    band = plane_bands(r["ref"])
    live = _pmax(r["mag"]) > 0
    den = _pmax(r["mag"]).clamp_min(1e-300)
    e_sp, e_32 = _pmax(r["y_sp"] - r["model"]) / den, _pmax(r["y_32"] - r["ref"]) / den
    m_err, m_floor = _pmax(r["model"] - r["ref"]) / den, _pmax(r["floor"]) / den
    # (b) holds per ELEMENT, not only per plane
    assert bool(((r["model"] - r["ref"]).abs() <= r["floor"]).all()), "model error above the scheme's floor"
    out = {}
    if with_norm:
        std = r["ref"].flatten(2).std(2).clamp_min(1e-300)
        n_sp, n_32, n_fl = _pmax(r["y_sp"] - r["ref"]) / std, _pmax(r["y_32"] - r["ref"]) / std, _pmax(r["floor"]) / std
    # A band is compared as a maximum over its planes because a single plane's fp32 error can be small by luck, so a band
    # that holds fewer than MIN_POOL planes is no band: its planes are pooled with the next lower band's (the last one with
    # the band above it), and the pool goes by the name of its highest band.
    pools, cur = [], None
    for bi in range(len(BAND_NAMES)):
        sel = (band == bi) & live
        if int(sel.sum()) == 0:
            continue
        cur = (cur[0], cur[1] | sel) if cur else (bi, sel)
        if int(cur[1].sum()) >= MIN_POOL:
            pools.append(cur)
            cur = None
    if cur:
        pools = pools[:-1] + [(pools[-1][0], pools[-1][1] | cur[1])] if pools else [cur]
    for bi, sel in pools:
        o = dict(planes=int(sel.sum()), e_sp=float(e_sp[sel].max()), e_32=float(e_32[sel].max()), model=float(m_err[sel].max()),
                 floor=float(m_floor[sel].max()))
        if with_norm:
            low = sel & (band >= 2)                 # the planes below -14: only they are allowed the floor of (b)
            o.update(n_sp=float(n_sp[sel].max()), n_32=float(n_32[sel].max()), low=bool(low.any()),
                     n_floor=float(n_fl[low].max()) if bool(low.any()) else 0.0)
        out[BAND_NAMES[bi]] = o
    return out


def _ratio(num, den):
    return 0.0 if num == 0.0 else (INF if den == 0.0 else num / den)


def judge(tag, bands, device, gate, report):
    """Assert (a) and (c) of one analysed case; collect the figures in ``report`` (worst ratios, per band)."""
    rg = RATIO_GATE[device] if gate is None else gate
    ng = NORM_GATE[device] if gate is None else gate
    for name, o in bands.items():
        ra = _ratio(o["e_sp"], o["e_32"])
        line = "%-44s band %-8s planes %4d  E_split/model %.2e  E_fp32/f64 %.2e  ratio %5.2f  model/f64 %.2e floor %.2e" % (
            tag, name, o["planes"], o["e_sp"], o["e_32"], ra, o["model"], o["floor"])
        key = (tag.split(" ")[0], name)
        w = report.setdefault(key, dict(ratio=0.0, norm=0.0, model=0.0, floor=0.0))
        w["ratio"], w["model"], w["floor"] = max(w["ratio"], ra), max(w["model"], o["model"]), max(w["floor"], o["floor"])
        if "n_sp" in o:
            rn_ = _ratio(o["n_sp"], o["n_32"])
            if not o["low"]:
                w["norm"] = max(w["norm"], rn_)
            line += "  N_split %.2e N_fp32 %.2e ratio %5.2f N_floor %.2e" % (o["n_sp"], o["n_32"], rn_, o["n_floor"])
        print(line)
        assert ra <= rg, ("(a) kernel vs model", tag, name, o, rg)
        if "n_sp" in o:
            # down to -14: the fp32 kernel's error times the gate (n_floor is 0); planes below -14 add the scheme's own floor
            assert o["n_sp"] <= o["n_floor"] + ng * o["n_32"], ("(c) error / plane std", tag, name, o, ng)


def _need_planes(ref, tag, least=8):
    """The ladder cases must put >= 8 planes into each band - asserted on the float64 reference alone."""
    cnt = torch.bincount(plane_bands(ref).flatten(), minlength=4).tolist()
    assert min(cnt) >= least, (tag, cnt)
    return cnt


def report_lines(report):
    return ["%-10s %-8s worst ratio (a) %5.2f  (c) %5.2f  model %.2e floor %.2e" % (k[0], k[1], v["ratio"], v["norm"],
                                                                                 v["model"], v["floor"])
            for k, v in sorted(report.items())]


def _worst(report):
    """Worst band ratio of (a), and of (c) over the bands it is gated in (down to -14)."""
    return dict(a=max(v["ratio"] for v in report.values()), c=max(v["norm"] for v in report.values()))


# =====================================================================================================================
# The checks
# =====================================================================================================================
SEAM3 = ((15, 31), (16, 32))          # 17 x 33 frame, 16 x 32 tiles: the halo of three neighbouring tiles
SEAM9 = ((7, 55), (8, 32))            # 9 x 57 frame: forward tiles 8 x 56 (x), dgrad / wgrad tiles 8 x 32 (dy)
# the spreading ladder of each form: the one whose channel index is the form's plane index
SPREAD = {"fwd": ("out-ladder",), "dgrad": ("col-ladder",), "dgrad_acc": ("col-ladder",), "wgrad": ("in-ladder", "out-ladder")}
NOT_DGRAD, DGRAD = ("fwd", "wgrad"), ("dgrad", "dgrad_acc")
NOT_WGRAD = ("fwd",) + DGRAD           # a scaled FRAME: the weight gradient sums over the frames, it has no plane of frame 1


def _sets(full):
    """(name, kind, batch, p, forms it applies to | None): every adversarial set on the GPU; on the emulator (a launch of the
    64 -> 64 shape takes 2.4 s per sample there) plain, the ladders, the 2^-10 frame and the 2^12 seam outlier, one sample
    where the set allows (a ladder needs two to put 8 planes below -18) and the output ladder without the dgrad, whose
    planes it does not spread."""
    if full:
        return [("plain", "plain", 2, None), ("in-ladder", "in-ladder", 2, None, NOT_DGRAD), ("col-ladder", "col-ladder", 2, None, DGRAD),
                ("out-ladder", "out-ladder", 2, None), ("frame-10", "frame", 2, -10, NOT_WGRAD), ("frame-20", "frame", 2, -20, NOT_WGRAD), ("outlier+12", "outlier", 2, 12),
                ("outlier+20", "outlier", 2, 20), ("boundary", "boundary", 2, 0), ("boundary-", "boundary", 2, 1)]
    return [("plain", "plain", 1, None), ("in-ladder", "in-ladder", 1, None, NOT_DGRAD), ("col-ladder", "col-ladder", 2, None, DGRAD),
            ("out-ladder", "out-ladder", 2, None, NOT_DGRAD), ("frame-10", "frame", 2, -10, NOT_WGRAD),
            ("outlier+12", "outlier", 1, 12)]


def _run_sets(device, cin, cout, k, H, W, forms, seam, seed, gate, full, act=0, ps=1, least=8):
    report = {}
    ops.set_conv_bf16_impl(0)
    for si, (name, kind, B, p, *only) in enumerate(_sets(full)):
        op = make_operands(kind, cin, cout, k, B, H, W, seed + si, seam, p)
        kn = Kernels(device, op, act, ps)
        base = None
        if "dgrad_acc" in forms:
            base = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(seed + 100 + si))
            if kind == "col-ladder":
                base = base * ladder(cin).view(1, cin, 1, 1)
        for form in forms:
            if only and form not in only[0]:
                continue
            r = run_form(form, kn, op, base)
            tag = "%s %d->%d k%d %s" % (form, cin, cout, k, name)
            if name in SPREAD[form] and least:
                print(tag, "planes per band", _need_planes(r["ref"], tag, least))
            judge(tag, analyse(r, with_norm=form != "wgrad"), device, gate, report)
    for ln in report_lines(report):
        print(ln)
    return report


def check_conv3_range(device, gate=None):
    """(a), (b), (c) for the 64 -> 64 trunk convolution (forward, dgrad, wgrad), 17 x 33: two 16 x 32 tiles each way, both
    ragged.  The emulator runs the reduced list of _sets."""
    full = device != "cpu"
    return _worst(_run_sets(device, 64, 64, 3, 17, 33, ("fwd", "dgrad", "wgrad"), SEAM3, 11, gate, full))


def check_conv3_other_forms(device, gate=None):
    """GPU only (the emulator's minute is spent on the 64 -> 64 shape): the other forward form at 128 produced channels, the
    32-channel tile (64 -> 32, 9 x 40), the PixelShuffle(2) + LeakyReLU epilogue (32 -> 128, 10 x 33) and the accumulating
    dgrad.  One sample each (the sets' own batch of two where a frame is scaled)."""
    rep = {}
    for (cin, cout, H, W, act, ps, forms, least) in ((128, 128, 17, 33, 0, 1, ("fwd", "dgrad", "dgrad_acc", "wgrad"), 8),
                                                     (64, 32, 9, 40, 0, 1, ("fwd", "dgrad", "wgrad"), 0),
                                                     (32, 128, 10, 33, 2, 2, ("fwd", "dgrad", "wgrad"), 0)):
        seam = ((H - 2, 31), (H - 1, 32))
        r = _run_sets(device, cin, cout, 3, H, W, forms, seam, 23 + cin, gate, True, act, ps, least)
        for (form, band), v in r.items():
            rep[("%s_%d_%d" % (form, cin, cout), band)] = v
    return _worst(rep)


def check_conv9_range(device, gate=None):
    """The 9 x 9 output layer, 32 -> 3 at B = 2, 9 x 57 (forward tiles 8 x 56, dgrad / wgrad tiles 8 x 32): forward, dgrad,
    accumulating dgrad, wgrad.  Three output channels cannot fill four bands: the >= 8 planes condition is asserted for the
    dgrad (64 planes) only, with >= 4 (32 channels over 20 octaves: 3 .. 4 per two octaves and sample)."""
    full = device != "cpu"
    rep = {}
    ops.set_conv_bf16_impl(0)
    sets = _sets(True) if full else [("plain", "plain", 2, None), ("in-ladder", "in-ladder", 2, None, NOT_DGRAD),
                                                    ("col-ladder", "col-ladder", 2, None, DGRAD), ("outlier+12", "outlier", 2, 12)]
    for si, (name, kind, B, p, *only) in enumerate(sets):
        op = make_operands(kind, 32, 3, 9, 2, 9, 57, 41 + si, SEAM9, p)
        kn = Kernels(device, op)
        base = torch.randn(2, 32, 9, 57, generator=torch.Generator().manual_seed(141 + si))
        if kind == "col-ladder":
            base = base * ladder(32).view(1, 32, 1, 1)
        for form in ("fwd", "dgrad", "dgrad_acc", "wgrad"):
            if only and form not in only[0]:
                continue
            r = run_form(form, kn, op, base)
            tag = "%s9 32->3 k9 %s" % (form, name)
            if form == "dgrad" and name == "col-ladder":
                print(tag, "planes per band", _need_planes(r["ref"], tag, 4))
            judge(tag, analyse(r, with_norm=form != "wgrad"), device, gate, rep)
    for ln in report_lines(rep):
        print(ln)
    return _worst(rep)


def check_model_vs_float64():
    """(b): the scheme's own error, no kernel involved - the model against float64 under the bound its arithmetic implies
    (scheme_floor, per element), for every operand set and bilinear form at the shapes of the kernel checks; and the ladder
    sets fill the four bands.  Returns the observed model error and the floor per form and band (normalised by the
    plane's conv(|a|, |b|)) - the figures of DESIGN.md 4.11."""
    out = {}
    for (cin, cout, k, H, W, seam, seed) in ((64, 64, 3, 17, 33, SEAM3, 11), (32, 3, 9, 9, 57, SEAM9, 41)):
        for si, (name, kind, B, p, *only) in enumerate(_sets(True)):
            op = make_operands(kind, cin, cout, k, B, H, W, seed + si, seam, p)
            x, w, dy = op["x"].to(F64), op["w"].to(F64), op["dy"].to(F64)
            for form, a, b in (("fwd", x, w), ("dgrad", dy, w), ("wgrad", x, dy)):
                if only and form not in only[0]:
                    continue
                ref, model = bilinear(form, a, b, k // 2), split2_model(form, a, b, k // 2)
                floor, mag = scheme_floor(form, a, b, k // 2), bilinear(form, a.abs(), b.abs(), k // 2)
                assert bool(((model - ref).abs() <= floor).all()), (form, k, name)
                if k == 3 and name in SPREAD[form]:
                    _need_planes(ref, (form, name), 8)
                band, den = plane_bands(ref), _pmax(mag).clamp_min(1e-300)
                for bi, bn in enumerate(BAND_NAMES):
                    sel = band == bi
                    if int(sel.sum()):
                        o = out.setdefault("%s k%d %s" % (form, k, bn), [0.0, 0.0])
                        o[0] = max(o[0], float((_pmax(model - ref) / den)[sel].max()))
                        o[1] = max(o[1], float((_pmax(floor) / den)[sel].max()))
    for kk, v in sorted(out.items()):
        print("model vs float64 %-22s observed %.2e  floor %.2e" % (kk, v[0], v[1]))
    return out


def _same(a, b, device, tag, atomics=False):
    """Bitwise; results summed with float atomics (wgrad, dbias) on the GPU: the 1e-5 summation-order bound of
    check_soft_dispatch."""
    if atomics and device != "cpu":
        assert rel_max(a, b) <= 1e-5, (tag, rel_max(a, b))
    else:
        assert torch.equal(a, b), (tag, rel_max(a, b))


def check_exactness(device, gate=None):
    """(d): zeros give the bias exactly; a zero input channel and a zero kernel row contribute exactly nothing; scaling an
    operand by 2^+-40 scales the result bitwise (forward, dgrad, the maximum the forward leaves behind; wgrad / dbias
    bitwise on the emulator, to summation order on the GPU) - the scales are exact powers of two, 2^+-40 stays inside the
    kernels' [-60, 60] clamp and the two exponents sum to < 126; a tensor maximum of exactly 2^3, and of the float below
    it, gives finite results that pass (a).  3 x 3 at 64 -> 64, 1 x 17 x 33, and the 9 x 9 layer at 1 x 9 x 57; on the
    emulator, which needs 0.6 s per tile and launch, one ragged tile each (1 x 5 x 12, 1 x 5 x 33): the seams are
    check_conv3_range's and check_conv9_range's there."""
    ops.set_conv_bf16_impl(0)
    emu = device == "cpu"
    report = {}
    for (cin, cout, k, H, W) in ((64, 64, 3, 5 if emu else 17, 12 if emu else 33), (32, 3, 9, 5 if emu else 9, 33 if emu else 57)):
        op = make_operands("plain", cin, cout, k, 1, H, W, 71 + k)
        # a channel / a kernel row that does not hold the kernel's or x's maximum (zeroing it must leave the scales alone)
        wtop = int(op["w"].abs().flatten().argmax())
        wcol, wrow, xch = wtop // (k * k) % cin, wtop // (k * k * cin), int(op["x"].abs().amax((0, 2, 3)).argmax())
        c0 = [c for c in range(cin) if c not in (wcol, xch)][3]
        r0 = (wrow + 1) % cout
        zero = lambda t: torch.zeros_like(t)
        bias_plane = nhwc(op["bias"].view(1, cout, 1, 1).expand(1, cout, H, W)).to(device)
        # all-zero x, all-zero kernel: the bias; all-zero dy: zero, and the accumulating form leaves its target alone
        for which in ("x", "w"):
            kn = Kernels(device, dict(op, **{which: zero(op[which])}))
            assert torch.equal(kn.fwd(), bias_plane), ("zero " + which, k)
        kn = Kernels(device, dict(op, dy=zero(op["dy"])))
        assert not bool(kn.dgrad().any()), ("zero dy", k)
        base = torch.randn(1, H, W, cin, generator=torch.Generator().manual_seed(5)).to(device)
        acc = base.clone()
        kn.dgrad(out=acc)
        assert torch.equal(acc, base), ("zero dy, accumulate", k)
        dw, db = kn.wgrad()
        assert not bool(dw.any()) and not bool(db.any()), ("zero dy, wgrad", k)
        # one zero input channel == the same call with that channel's kernel column zeroed too; one zero kernel row: that
        # plane is the bias (both in one pair of launches; the maxima, hence the scales, are those of the plain operands)
        x0, w1 = op["x"].clone(), op["w"].clone()
        x0[:, c0] = 0
        w1[r0] = 0
        w0 = w1.clone()
        w0[:, c0] = 0
        assert float(w0.abs().max()) == float(op["w"].abs().max()) and float(x0.abs().max()) == float(op["x"].abs().max())
        y = Kernels(device, dict(op, x=x0, w=w1)).fwd()
        assert torch.equal(y, Kernels(device, dict(op, x=x0, w=w0)).fwd()), ("zero channel", k)
        assert torch.equal(y[..., r0], bias_plane[..., r0]), ("zero kernel row", k)
        assert bool((y[..., (r0 + 1) % cout] != bias_plane[..., (r0 + 1) % cout]).any())
        # power-of-two equivariance, no bias.  x and dy are scaled in one set of launches, by 2^e and 2^-e (the forward sees
        # x, the dgrad dy, the wgrad both: dw must not move), the kernel in another
        nb = dict(op, bias=None)
        k0 = Kernels(device, nb)
        a0 = ops.amax_buffer(k0.x) if k == 3 else None
        y0, dx0, (dw0, db0) = k0.fwd(amax=a0) if k == 3 else k0.fwd(), k0.dgrad(), k0.wgrad()
        assert float(y0.abs().max()) > 0 and float(dx0.abs().max()) > 0 and float(dw0.abs().max()) > 0

        def fwd_scaled(kq, f, tag):
            aq = ops.amax_buffer(kq.x) if k == 3 else None
            yq = kq.fwd(amax=aq) if k == 3 else kq.fwd()
            assert torch.equal(yq, y0 * f), ("fwd equivariance", tag, k, rel_max(yq, y0 * f))
            if k == 3:
                assert ops.amax_value(aq) == ops.amax_value(a0) * f == float(yq.abs().max()), ("ymax", tag)

        for e in (40, -40):
            f = 2.0 ** e
            kq = Kernels(device, dict(nb, x=op["x"] * f, dy=op["dy"] / f))
            fwd_scaled(kq, f, ("x", e))
            _same(kq.dgrad(), dx0 / f, device, ("dgrad equivariance", "dy", -e, k))
            dwq, dbq = kq.wgrad()
            _same(dwq, dw0, device, ("wgrad equivariance", e, k), atomics=True)
            _same(dbq, db0 / f, device, ("dbias equivariance", -e, k), atomics=True)
            kq = Kernels(device, dict(nb, w=op["w"] * f))
            fwd_scaled(kq, f, ("w", e))
            _same(kq.dgrad(), dx0 * f, device, ("dgrad equivariance", "w", e, k))
        # the two boundary maxima
        for p in (0, 1):
            opb = make_operands("boundary", cin, cout, k, 1, H, W, 81 + k, p=p)
            kn = Kernels(device, opb)
            for form in ("fwd", "dgrad", "wgrad"):
                judge("%s%d boundary%s" % (form, k, "-" * p), analyse(run_form(form, kn, opb), form != "wgrad"), device, gate, report)
    return _worst(report)


DARK_SEED = 2
DARK_CASE = dict(scale=8, which=[0, 1], L=16, nb=4, B=2, H=8, W=12)


def _dark_batch(seed):
    lq, _, dm, mk = synth.closed_form_batch(seed, 2, 8, 12, 8)
    lq = lq.clone()
    lq[1] *= 2.0 ** -10
    return lq, dm, mk


def oracle_gradient_jump(net, cfg, lq, dm, mk, draws=4):
    """How far the ORACLE's own gradient (of _compare_with_oracle's functional, same rel-L2) moves when lq, the depth map
    and every parameter are perturbed by one fp32 ulp (random signs): ~1.2e-6 where the functional is smooth, 2e-4 .. 1.5e-3
    where a ReLU input sits at rounding distance from zero.  No kernel involved."""
    def grads(lq_, dm_, sd):
        ref = O.depthnet_forward(sd, cfg, lq_, dm_, mk)
        wgt = torch.cos(torch.arange(ref.numel(), dtype=torch.float32) * 0.013).reshape(ref.shape)
        (ref * wgt).sum().backward()
        return {k: v.grad.double() for k, v in sd.items() if v.grad is not None and not any(z in k for z in ZERO_GRAD_KEYS)}

    def ulp(t, gen):
        return t * (1 + ((torch.rand(t.shape, generator=gen) < 0.5).to(t.dtype) * 2 - 1) * 2.0 ** -23)

    g0 = grads(lq, dm, _oracle_sd(net))
    worst = 0.0
    for d in range(draws):
        gen = torch.Generator().manual_seed(2000 + d)
        sd = {k: ulp(v.detach(), gen).requires_grad_(True) if v.is_floating_point() else v for k, v in _oracle_sd(net).items()}
        g1 = grads(ulp(lq, gen), ulp(dm, gen), sd)
        num = sum((g1[k] - g0[k]).pow(2).sum().item() for k in g0)
        worst = max(worst, math.sqrt(num / sum(g0[k].pow(2).sum().item() for k in g0)))
    return worst


def check_whole_net_dark_frame(device):
    """One whole-net case with the split convolutions FORCED on (graph.SPLIT_MIN_PIXELS = 0, fp16 x 2): the shape of
    check_batch_independence_and_determinism (x8, two DGBs of four blocks, L = 16, 8 x 12) at B = 2 with frame 1 of lq
    multiplied by 2^-10 - a dark frame next to a bright one, whose activations in front of the first InstanceNorm get their
    scale from frame 0.  _compare_with_oracle's default gates, unchanged (forward 2e-4, gradient rel-L2 2e-5); each frame
    run alone agrees with its in-batch output to the existing 2e-5.
    Seed: this net has ReLU knife-edges (tests/test_gpu_parity.py, _SPLIT_CASES), so the frames (closed_form_batch index
    DARK_SEED) were chosen WITHOUT consulting the split run, as the lowest index that meets two conditions on the reference
    side: (1) the EXACT-fp32 run (graph.SPLIT_BF16 = False) passes both gates with >= 4x headroom - MI355X: forward
    6.4e-6, gradient 1.66e-6, emulator: 6.7e-6, 1.74e-6 (the exact-fp32 run itself fails the gradient gate at index 1 on the
    emulator, 1.1e-3, and at indices 0 and 5 on the MI355X, 5.8e-4 and 1.3e-3); (2) the ORACLE's own gradient is smooth there - it moves by
    <= 5e-6 (the same 4x headroom) under one-ulp perturbations of inputs and parameters (oracle_gradient_jump; asserted
    below, no kernel involved).  (1) alone does not find the knife-edges: at indices 0, 1, 3, 4, 6, 7 the oracle's gradient
    jumps by 2e-4 .. 1.5e-3 under such a perturbation (indices 2 and 5: 1.2e-6 .. 1.3e-6), whatever the frames' brightness."""
    net, cfg = build_net(DARK_CASE, device)
    lq, dm, mk = _dark_batch(DARK_SEED)
    jump = oracle_gradient_jump(build_net(DARK_CASE, "cpu")[0], cfg, lq, dm, mk)
    assert jump <= 2e-5 / 4, ("the reference itself is not smooth at this seed", jump)
    old = graph.SPLIT_BF16, graph.SPLIT_MIN_PIXELS, graph.SPLIT_PIECES
    graph.SPLIT_BF16, graph.SPLIT_MIN_PIXELS, graph.SPLIT_PIECES = True, 0, 2
    try:
        err, rel = _compare_with_oracle(net, cfg, lq, dm, mk, device)
        with torch.no_grad():
            full = net(lq.to(device), dm.to(device), mk.to(device))
            worst = 0.0
            for b in range(2):
                solo = net(lq[b:b + 1].contiguous().to(device), dm[b:b + 1].contiguous().to(device),
                           mk[b:b + 1].contiguous().to(device))
                d = (full[b:b + 1] - solo).abs().max().item()
                print("dark frame: frame %d alone vs in its batch: max |diff| %.3g" % (b, d))
                worst = max(worst, d)
            assert worst <= 2e-5, worst
    finally:
        graph.SPLIT_BF16, graph.SPLIT_MIN_PIXELS, graph.SPLIT_PIECES = old
    print("dark frame whole net: forward err %.3g, gradient rel-L2 %.3g, batch dependence %.3g, oracle jump %.3g" % (err, rel, worst, jump))
    return dict(fwd=err, grad=rel, batch=worst, oracle_jump=jump)


def whole_net_fp32_headroom(device, seed):
    """The exact-fp32 run of check_whole_net_dark_frame's case (condition (1) of its seed), and condition (2)."""
    net, cfg = build_net(DARK_CASE, device)
    lq, dm, mk = _dark_batch(seed)
    jump = oracle_gradient_jump(build_net(DARK_CASE, "cpu")[0], cfg, lq, dm, mk)
    old = graph.SPLIT_BF16
    graph.SPLIT_BF16 = False
    try:
        return _compare_with_oracle(net, cfg, lq, dm, mk, device, fwd_tol=2e-4 / 4, grad_tol=2e-5 / 4) + (jump,)
    finally:
        graph.SPLIT_BF16 = old
