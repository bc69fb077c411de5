"""Tensor-level wrappers of the C ABI (include/dasr.h).

PyTorch is used here for device memory (``torch.empty``) and the current stream only; every
computation is a call into libdasr_hip.so.  Activations are NHWC ``[B,H,W,C]``, kernels are HWIO
``[KH,KW,Cin,Cout]``.  fp32 is the default; a bf16 activation tensor selects the ``*_bf16`` entry
points (mixed-precision path: bf16 activations and trunk kernels, fp32 parameters / statistics /
accumulators) - the dtype of the tensors passed in decides, nothing is converted silently.
"""
import ctypes

import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
IN_EPS = 1e-5  # nn.InstanceNorm2d default eps (sftmd_arch.py:813, normalization.py:17)


BF16 = torch.bfloat16


def _p(t, allow_none=False):
    return _lib.ptr(t, allow_none)


def _pa(t, allow_none=False):
    """Pointer of an activation tensor: float32 or bfloat16."""
    if t is None:
        return _lib.ptr(t, allow_none)
    return _lib.ptr(t, allow_none, dtype=t.dtype if t.dtype in (torch.float32, BF16) else torch.float32)


def _is_bf(*ts):
    """True when the tensors that are given are bfloat16 (mixing is a caller bug)."""
    kinds = {t.dtype for t in ts if t is not None}
    if len(kinds) > 1:
        raise TypeError("dasr_amd: mixed activation dtypes %s" % sorted(str(k) for k in kinds))
    return kinds == {BF16}


def _call(name, *args):
    fn = getattr(_lib.get(), name)
    _lib.check(fn(*args, _lib.stream()), name)


def empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


# ---- edge ----------------------------------------------------------------------------------
def nchw_to_nhwc(x):
    B, C, H, W = x.shape
    out = empty((B, H, W, C), x)
    _call("dasr_nchw_to_nhwc", _p(x), _p(out), B, C, H, W)
    return out


def nhwc_to_nchw(x):
    B, H, W, C = x.shape
    out = empty((B, C, H, W), x)
    _call("dasr_nhwc_to_nchw", _p(x), _p(out), B, C, H, W)
    return out


def clamp_to_nchw(y, lo, hi):
    B, H, W, C = y.shape
    out = empty((B, C, H, W), y)
    _call("dasr_clamp_to_nchw", _p(y), _p(out), B, C, H, W, float(lo), float(hi))
    return out


def clamp_to_nchw_bwd(dout, y, lo, hi):
    B, H, W, C = y.shape
    dy = empty(y.shape, y)
    _call("dasr_clamp_to_nchw_bwd", _p(dout), _p(y), _p(dy), B, C, H, W, float(lo), float(hi))
    return dy


def resize_nearest_nchw(x, H, W):
    B, C, h, w = x.shape
    if (h, w) == (H, W):
        return x
    out = empty((B, C, H, W), x)
    _call("dasr_resize_nearest_nchw", _p(x), _p(out), B * C, h, w, H, W)
    return out


def resize_nearest_u8(region, H, W):
    B, h, w = region.shape
    if (h, w) == (H, W):
        return region
    out = torch.empty((B, H, W), dtype=torch.uint8, device=region.device)
    _call("dasr_resize_nearest_u8", _lib.ptr(region, dtype=torch.uint8), _lib.ptr(out, dtype=torch.uint8), B, h, w, H, W)
    return out


# ---- max |.| of a tensor, carried on the tensor (fp16 x 2 split convolutions) ---------------------------------------
# A producer kernel that is handed an amax buffer (dasr.h: DASR_AMAX_FLOATS floats - a count and one partial maximum per
# workgroup) fills it while it stores its output; the buffer then travels with the tensor as an attribute.  Every op that
# writes into an existing tensor drops it.
AMAX_FLOATS = 4097


def amax_buffer(like):
    """An (uninitialised) amax buffer on ``like``'s device: nothing to clear, the producer writes every word it declares."""
    return torch.empty((AMAX_FLOATS,), dtype=torch.float32, device=like.device)


def amax_value(buf):
    """Host-side read of an amax buffer (tests and tools only: the kernels never need it on the host)."""
    h = buf.detach().cpu()
    n = int(h[:1].view(torch.int32).item())
    assert 1 <= n < AMAX_FLOATS, n
    return float(h[1:1 + n].max().item())


def set_amax(t, amax):
    if amax is not None:
        t._dasr_amax = amax
    return t


def get_amax(t):
    return getattr(t, "_dasr_amax", None)


def drop_amax(t):
    if t is not None and getattr(t, "_dasr_amax", None) is not None:
        t._dasr_amax = None


def add(a, b):
    out = torch.empty_like(a)
    if _is_bf(a, b):
        _call("dasr_add_bf16", _pa(a), _pa(b), _pa(out), a.numel())
    else:
        _call("dasr_add", _p(a), _p(b), _p(out), a.numel())
    return out


def accumulate_(dst, src):
    assert dst.shape == src.shape
    drop_amax(dst)
    if dst.dtype == torch.float32 and src.dtype == BF16:       # bf16 gradient arriving at an fp32 tensor
        _call("dasr_cast_bf16_to_f32", _pa(src), _p(dst), 1, dst.numel())
    elif _is_bf(dst, src):
        _call("dasr_accumulate_bf16", _pa(dst), _pa(src), dst.numel())
    else:
        _call("dasr_accumulate", _p(dst), _p(src), dst.numel())
    return dst


def copy_(dst, src):
    assert dst.numel() == src.numel() and dst.dtype == src.dtype
    drop_amax(dst)
    if dst.dtype == BF16:
        assert dst.numel() % 2 == 0
        _call("dasr_copy", _pa(dst), _pa(src), dst.numel() // 2)      # a byte copy: two bf16 per float
    else:
        _call("dasr_copy", _p(dst), _p(src), dst.numel())
    return dst


def cast_to_bf16(x):
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    _call("dasr_cast_f32_to_bf16", _p(x), _pa(out), x.numel())
    return out


def cast_to_f32(x):
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _call("dasr_cast_bf16_to_f32", _pa(x), _p(out), 0, x.numel())
    return out


# ---- the encoder's stride-2 layers in stride-1 form (csrc/s2d.hip; bf16 path only) ----------------------------------
def set_conv_bf16_impl(impl):
    """0 (default): the persistent LDS-DMA kernel runs the bf16 trunk forward / dgrad where it applies; 1: the first
    (register-staged) kernel everywhere - for A/B measurements and tests."""
    _call("dasr_set_conv_bf16_impl", int(impl))


def conv_bf16_v2_launches():
    return int(_lib.get().dasr_conv_bf16_v2_launches())


def tensor_version(t):
    """torch's in-place edit counter of ``t``; tensors created under ``torch.inference_mode()`` do not track one
    (reading it raises) and are reported as version -1: they are treated as immutable."""
    try:
        return t._version
    except RuntimeError:
        return -1


def space_to_depth2(x, valid_hw=None):
    """[B,H,W,C] fp32 or bf16 -> bf16 [B,ceil(H/2),ceil(W/2),4C], channel (2py+px)C + c = x[2i+py][2j+px][c].
    ``valid_hw`` = (Hv, Wv): rows / columns of x at or beyond them are read as zeros (the PixelShuffle image of the
    encoder's transposed layer carries one row and one column the reference's layer does not have)."""
    B, H, W, C = x.shape
    Hv, Wv = valid_hw if valid_hw is not None else (H, W)
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2, 4 * C), dtype=BF16, device=x.device)
    _call("dasr_space_to_depth2_bf16", _pa(x), 1 if x.dtype == BF16 else 0, _pa(out), B, H, W, C, Hv, Wv)
    return out


def depth_to_space2_bwd(dy, x_shape, dtype, out=None, valid_hw=None):
    """Adjoint of space_to_depth2: bf16 gradient [B,Hs,Ws,4C] -> gradient of x (``dtype``), zero beyond ``valid_hw``;
    ``out``: accumulate into it."""
    B, H, W, C = x_shape
    Hv, Wv = valid_hw if valid_hw is not None else (H, W)
    acc = out is not None
    if out is None:
        out = torch.empty(tuple(x_shape), dtype=dtype, device=dy.device)
    drop_amax(out)
    _call("dasr_depth_to_space2_bwd_bf16", _pa(dy), _pa(out), 1 if out.dtype == BF16 else 0, 1 if acc else 0, B, H, W, C,
          Hv, Wv)
    return out


def weight_expand_s2(w_packed):
    """fp32 packed kernel (2,3,3,Cin,Cout) of a stride-2 conv -> bf16 packed kernel (2,3,3,4Cin,Cout) of its stride-1 form."""
    _, KH, KW, Cin, Cout = w_packed.shape
    assert (KH, KW) == (3, 3)
    out = torch.empty((2, 3, 3, 4 * Cin, Cout), dtype=BF16, device=w_packed.device)
    _call("dasr_weight_expand_s2_bf16", _p(w_packed), _pa(out), Cin, Cout)
    return out


def weight_collapse_s2(dw_expanded, Cin, Cout):
    out = torch.empty((3, 3, Cin, Cout), dtype=torch.float32, device=dw_expanded.device)
    _call("dasr_weight_collapse_s2", _p(dw_expanded), _p(out), Cin, Cout)
    return out


def weight_expand_t2(w_packed, bias):
    """fp32 packed kernel (2,3,3,Cin,Cout) of a stride-2 ConvTranspose2d (+ bias) -> bf16 packed kernel (2,3,3,Cin,4Cout) and
    bias [4Cout] of the stride-1 convolution whose PixelShuffle(2) is the transposed convolution."""
    _, KH, KW, Cin, Cout = w_packed.shape
    assert (KH, KW) == (3, 3)
    out = torch.empty((2, 3, 3, Cin, 4 * Cout), dtype=BF16, device=w_packed.device)
    b4 = torch.empty((4 * Cout,), dtype=torch.float32, device=w_packed.device) if bias is not None else None
    _call("dasr_weight_expand_t2_bf16", _p(w_packed), _p(bias, True), _pa(out), _p(b4, True), Cin, Cout)
    return out, b4


def weight_collapse_t2(dw_expanded, db_expanded, Cin, Cout):
    dw = torch.empty((3, 3, Cin, Cout), dtype=torch.float32, device=dw_expanded.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=dw_expanded.device) if db_expanded is not None else None
    _call("dasr_weight_collapse_t2", _p(dw_expanded), _p(db_expanded, True), _p(dw), _p(db, True), Cin, Cout)
    return dw, db


def zeros(shape, like):
    return torch.zeros(shape, dtype=torch.float32, device=like.device)


# ---- weights ------------------------------------------------------------------------------
def weight_pack(v, g, transposed=False, out=None, o_off=0, dtype=torch.float32):
    """Pack a PyTorch-layout fp32 kernel (optionally weight-normed) into HWIO, fp32 or bf16.  Returns (w, inv_norm)."""
    if transposed:
        I, O, KH, KW = v.shape
    else:
        O, I, KH, KW = v.shape
    if out is None:
        out = empty((2, KH, KW, I, O), v, dtype)   # [0]: HWIO, [1]: memory holds the per-tap transpose [KH,KW,O,I]
    ldo = out.shape[4]
    inv = empty((I if transposed else O,), v) if g is not None else None
    if out.dtype == BF16:
        _call("dasr_weight_pack_fwd_bf16", _p(v), _p(g, True), _pa(out), _p(inv, True), O, I, KH, KW, int(transposed), ldo,
              int(o_off))
    else:
        _call("dasr_weight_pack_fwd", _p(v), _p(g, True), _p(out), _p(inv, True), O, I, KH, KW, int(transposed), ldo,
              int(o_off))
    return out, inv


class PackJob(ctypes.Structure):
    """include/dasr.h: dasr_pack_job."""
    _fields_ = [("v", ctypes.c_void_p), ("g", ctypes.c_void_p), ("w", ctypes.c_void_p), ("inv_norm", ctypes.c_void_p),
                ("amax", ctypes.c_void_p)] + [(n, ctypes.c_int) for n in
                                              ("O", "I", "KK", "transposed", "ldo", "o_off", "bf16", "plain", "wg_begin", "reserved")]


class SplitJob(ctypes.Structure):
    """include/dasr.h: dasr_split_job."""
    _fields_ = [("w_packed", ctypes.c_void_p), ("wmax", ctypes.c_void_p), ("w_split", ctypes.c_void_p)] + \
               [(n, ctypes.c_int) for n in ("Cin", "Cout", "wg_begin", "reserved")]


class JobTable:
    """A job table of one multi-tensor launch: the ctypes array (host copy) and its image in device memory, kept together
    with the tensors the jobs point at."""

    def __init__(self, jobs, device, keep):
        self.n = len(jobs)
        self.host = (type(jobs[0]) * self.n)(*jobs)
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)
        self.keep = keep


def pack_job(v, g, w, inv, amax, transposed, o_off, plain, wg_begin):
    """One dasr_weight_pack_fwd call as a table entry (``w``: the packed buffer (2, KH, KW, I, ldo), or a flat buffer of
    ldo floats when ``plain``: a bias vector placed at o_off)."""
    if plain:
        O, I, KK, ldo = v.numel(), 1, 1, w.numel()
    else:
        if transposed:
            I, O, KH, KW = v.shape
        else:
            O, I, KH, KW = v.shape
        KK, ldo = KH * KW, w.shape[4]
    bf = w.dtype == BF16
    return PackJob(_p(v), _p(g, True), _lib.ptr(w, False, w.dtype), _p(inv, True), _p(amax, True), O, I, KK, int(transposed), ldo,
                   int(o_off), int(bf), int(plain), int(wg_begin), 0), (I if transposed else O)


def weight_pack_multi(table):
    _call("dasr_weight_pack_multi", ctypes.addressof(table.host), table.dev.data_ptr(), table.n)


def split_job(w, wmax, ws, wg_begin):
    KH, KW, Cin, Cout = _wdims(w)
    assert (KH, KW) == (3, 3) and w.dtype == torch.float32
    return (SplitJob(_p(w), _p(wmax), _lib.ptr(ws, False, torch.float16), Cin, Cout, int(wg_begin), 0),
            int(_lib.get().dasr_conv3x3_split2_weights_slabs(Cin, Cout)))


def conv3x3_split2_weights_multi(table):
    _call("dasr_conv3x3_split2_weights_multi", ctypes.addressof(table.host), table.dev.data_ptr(), table.n)


def weight_pack_bwd(dw, v, g, inv, transposed=False, o_off=0):
    if transposed:
        I, O, KH, KW = v.shape
    else:
        O, I, KH, KW = v.shape
    dv = torch.empty_like(v)
    dg = torch.empty_like(g) if g is not None else None
    assert dw.dim() == 4, "weight gradients are plain HWIO"
    _call("dasr_weight_pack_bwd", _p(dw), _p(v), _p(g, True), _p(inv, True), _p(dv), _p(dg, True), O, I, KH, KW,
          int(transposed), dw.shape[3], int(o_off))
    return dv, dg


# ---- convolution ----------------------------------------------------------------------------
def conv_out_hw(H, W, KH, KW, stride, pad, transposed):
    if transposed:
        return (H - 1) * stride - 2 * pad + KH, (W - 1) * stride - 2 * pad + KW
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def pack_hwio(w4):
    """Packed kernel (HWIO + per-tap transpose) from a plain HWIO tensor - for tests and micro-benchmarks; the
    product path gets packed kernels from weight_pack (dasr_weight_pack_fwd)."""
    KH, KW, I, O = w4.shape
    out = torch.empty((2, KH, KW, I, O), dtype=w4.dtype, device=w4.device)      # bf16 in, bf16 packed
    out[0].copy_(w4)
    out[1].view(KH, KW, O, I).copy_(w4.permute(0, 1, 3, 2))
    return out


def _wdims(w):
    if w.dim() != 5 or w.shape[0] != 2:
        raise ValueError("dasr_amd: convolution kernels must be packed (ops.weight_pack / ops.pack_hwio)")
    return tuple(w.shape[1:])


def conv2d_fwd(x, w, bias=None, residual=None, stride=1, pad=1, transposed=False, act=ACT_NONE, ps_r=1, out_dtype=None,
               amax=None):
    """``out_dtype=torch.bfloat16`` with an fp32 ``x`` is the mask layer of the bf16 path (fp32 depth map in, bf16
    activation out); a bf16 ``x`` selects the bf16 path by itself (the 9x9 output conv then returns fp32).
    ``amax`` (fp32 path): a zeroed device float that receives max |y| and is attached to y (set_amax)."""
    B, H, W, Cin = x.shape
    KH, KW, wi, Cout = _wdims(w)
    assert wi == Cin, (w.shape, x.shape)
    Ho, Wo = conv_out_hw(H, W, KH, KW, stride, pad, transposed)
    bf = x.dtype == BF16 or out_dtype == BF16
    ydt = torch.float32
    if bf and not (KH == 9 and Cout <= 3):
        ydt = BF16
    if ps_r > 1:
        y = empty((B, Ho * ps_r, Wo * ps_r, Cout // (ps_r * ps_r)), x, ydt)
    else:
        y = empty((B, Ho, Wo, Cout), x, ydt)
    if bf:
        _call("dasr_conv2d_fwd_bf16", _pa(x), _pa(w), _p(bias, True), _pa(residual, True), _pa(y), B, H, W, Cin, Ho, Wo,
              Cout, KH, KW, stride, pad, int(transposed), act, ps_r)
    else:
        _call("dasr_conv2d_fwd", _p(x), _p(w), _p(bias, True), _p(residual, True), _p(y), _p(amax, True), B, H, W, Cin, Ho, Wo,
              Cout, KH, KW, stride, pad, int(transposed), act, ps_r)
        set_amax(y, amax)
    return y


def conv2d_fwd_tile_rows(B, H, W, Cin, Cout):
    """Tile rows (8 or 16) of the fp32 MFMA kernel that carries this 3x3 / stride 1 / pad 1 geometry, 0: another family."""
    return int(_lib.get().dasr_conv2d_fwd_tile_rows(B, H, W, Cin, Cout))


def conv2d_epilogue_bwd(dy, y, Ho, Wo, Cout, act, ps_r, amax=None):
    B = y.shape[0]
    dconv = empty((B, Ho, Wo, Cout), y, y.dtype)
    if _is_bf(dy, y):
        _call("dasr_conv2d_epilogue_bwd_bf16", _pa(dy), _pa(y), _pa(dconv), B, Ho, Wo, Cout, act, ps_r)
    else:
        _call("dasr_conv2d_epilogue_bwd", _p(dy), _p(y), _p(dconv), _p(amax, True), B, Ho, Wo, Cout, act, ps_r)
        set_amax(dconv, amax)
    return dconv


def conv2d_dgrad(dconv, w, x_shape, stride=1, pad=1, transposed=False, out=None, out_dtype=torch.float32):
    """``out_dtype`` = dtype of the conv's input (bf16 input -> bf16 gradient; the 9x9 output conv takes an fp32 dconv)."""
    B, H, W, Cin = x_shape
    KH, KW, _, Cout = _wdims(w)
    _, Ho, Wo, _ = dconv.shape
    acc = out is not None
    if out is None:
        out = torch.empty(x_shape, dtype=out_dtype, device=dconv.device)
    drop_amax(out)
    if out.dtype == BF16:
        _call("dasr_conv2d_dgrad_bf16", _pa(dconv), _pa(w), _pa(out), int(acc), B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride,
              pad, int(transposed))
    else:
        _call("dasr_conv2d_dgrad", _p(dconv), _p(w), _p(out), int(acc), B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad,
              int(transposed))
    return out


def conv2d_dgrad_act_supported(x_shape, w, dconv_shape, stride, pad, transposed, ps_r):
    B, H, W, Cin = x_shape
    KH, KW, _, Cout = _wdims(w)
    _, Ho, Wo, _ = dconv_shape
    return bool(_lib.get().dasr_conv2d_dgrad_act_supported(B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad,
                                                          int(transposed), ps_r))


def conv2d_dgrad_act(dconv, w, x_act, act, ps_r, stride=1, pad=1, transposed=False):
    """Gradient w.r.t. the PRODUCER conv's raw output: dgrad * act'(x_act), stored un-shuffled."""
    B, H, W, Cin = x_act.shape
    KH, KW, _, Cout = _wdims(w)
    _, Ho, Wo, _ = dconv.shape
    out = torch.empty((B, H // ps_r, W // ps_r, Cin * ps_r * ps_r), dtype=torch.float32, device=dconv.device)
    _call("dasr_conv2d_dgrad_act", _p(dconv), _p(w), _p(x_act), _p(out), B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad,
          int(transposed), act, ps_r)
    return out


def conv2d_wgrad(x, dconv, w_shape, stride=1, pad=1, transposed=False, want_bias=True):
    B, H, W, Cin = x.shape
    KH, KW, _, Cout = w_shape
    _, Ho, Wo, _ = dconv.shape
    lib = _lib.get()
    bf = x.dtype == BF16
    wsfn = lib.dasr_conv2d_wgrad_workspace_bf16 if bf else lib.dasr_conv2d_wgrad_workspace
    nbytes = wsfn(B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, int(transposed))
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
    dw = empty(w_shape, x)
    db = empty((Cout,), x) if want_bias else None
    if bf:
        _call("dasr_conv2d_wgrad_bf16", _pa(x), _pa(dconv), _p(dw), _p(db, True), _p(ws), nbytes, B, H, W, Cin, Ho, Wo,
              Cout, KH, KW, stride, pad, int(transposed))
    else:
        _call("dasr_conv2d_wgrad", _p(x), _p(dconv), _p(dw), _p(db, True), _p(ws), nbytes, B, H, W, Cin, Ho, Wo, Cout, KH,
              KW, stride, pad, int(transposed))
    return dw, db


def conv2d_wgrad_act(x, dy, y, w_shape, act, stride=1, pad=1, transposed=False, want_bias=True):
    """Weight/bias gradient of a conv whose input needs no gradient, activation backward fused."""
    B, H, W, Cin = x.shape
    KH, KW, _, Cout = w_shape
    _, Ho, Wo, _ = y.shape
    lib = _lib.get()
    if _is_bf(dy, y):                      # the mask layer of the bf16 path: fused kernel only
        dw = empty(w_shape, x)
        db = empty((Cout,), x) if want_bias else None
        _call("dasr_conv2d_wgrad_act_bf16", _p(x), _pa(dy), _pa(y), _p(dw), _p(db, True), B, H, W, Cin, Ho, Wo, Cout, KH, KW,
              stride, pad, int(transposed), act)
        return dw, db
    nbytes = lib.dasr_conv2d_wgrad_workspace(B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, int(transposed))
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
    fused = bool(lib.dasr_conv2d_wgrad_act_fused(B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, int(transposed)))
    scratch = None if fused else torch.empty_like(y)
    dw = empty(w_shape, x)
    db = empty((Cout,), x) if want_bias else None
    _call("dasr_conv2d_wgrad_act", _p(x), _p(dy), _p(y), _p(dw), _p(db, True), _p(scratch, True), _p(ws), nbytes, B, H,
          W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, int(transposed), act)
    return dw, db


# ---- fp32 convolutions on the bf16 matrix cores (split bf16 x 3: three pieces per operand, six products) -------
def conv3x3_split_supported(H, W, Cin, Cout):
    return bool(_lib.get().dasr_conv3x3_split_supported(H, W, Cin, Cout))


def conv3x3_split_weights(w):
    """fp32 packed kernel (2,3,3,Cin,Cout) -> the bf16 three-piece image both split kernels read."""
    KH, KW, Cin, Cout = _wdims(w)
    assert (KH, KW) == (3, 3) and w.dtype == torch.float32
    n = int(_lib.get().dasr_conv3x3_split_weights_bytes(Cin, Cout)) // 2
    ws = torch.empty((n,), dtype=BF16, device=w.device)
    _call("dasr_conv3x3_split_weights", _p(w), _pa(ws), Cin, Cout)
    return ws


def conv3x3_fwd_split(x, ws, bias, Cout, residual=None, act=ACT_NONE, ps_r=1):
    B, H, W, Cin = x.shape
    if ps_r > 1:
        y = empty((B, H * ps_r, W * ps_r, Cout // (ps_r * ps_r)), x)
    else:
        y = empty((B, H, W, Cout), x)
    _call("dasr_conv3x3_fwd_split", _p(x), _pa(ws), _p(bias, True), _p(residual, True), _p(y), B, H, W, Cin, Cout, act, ps_r)
    return y


def conv3x3_wgrad_split(x, dconv, want_bias=True):
    """(dw [3,3,Cin,Cout], dbias | None) of a plain 3x3 convolution, fp32, on the split-bf16 kernel."""
    B, H, W, Cin = x.shape
    Cout = dconv.shape[3]
    nbytes = int(_lib.get().dasr_conv3x3_wgrad_split_workspace(B, H, W, Cin, Cout))
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
    dw = empty((3, 3, Cin, Cout), x)
    db = empty((Cout,), x) if want_bias else None
    _call("dasr_conv3x3_wgrad_split", _p(x), _p(dconv), _p(dw), _p(db, True), _p(ws), nbytes, B, H, W, Cin, Cout)
    return dw, db


def conv3x3_dgrad_split(dconv, ws, x_shape, out=None):
    B, H, W, Cin = x_shape
    Cout = dconv.shape[3]
    acc = out is not None
    if out is None:
        out = empty(tuple(x_shape), dconv)
    drop_amax(out)
    _call("dasr_conv3x3_dgrad_split", _p(dconv), _pa(ws), _p(out), 1 if acc else 0, B, H, W, Cin, Cout)
    return out


# ---- the same with two fp16 pieces / three products; every tensor operand comes with its max |.| in device memory ----
def absmax(x):
    """max |x| as an amax buffer on the device (the fp16 scheme's kernels derive their power-of-two scale from it)."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = amax_buffer(x)
    _call("dasr_absmax", _p(x), x.numel(), _p(out))
    return out


def conv3x3_split2_weights(w):
    """fp32 packed kernel (2,3,3,Cin,Cout) -> (fp16 two-piece image, max |w| device scalar)."""
    KH, KW, Cin, Cout = _wdims(w)
    assert (KH, KW) == (3, 3) and w.dtype == torch.float32
    wmax = absmax(w[0])
    n = int(_lib.get().dasr_conv3x3_split2_weights_bytes(Cin, Cout)) // 2
    ws = torch.empty((n,), dtype=torch.float16, device=w.device)
    _call("dasr_conv3x3_split2_weights", _p(w), _p(wmax), _lib.ptr(ws, False, torch.float16), Cin, Cout)
    return ws, wmax


def conv3x3_fwd_split2(x, xmax, ws, bias, Cout, residual=None, act=ACT_NONE, ps_r=1, amax=None):
    B, H, W, Cin = x.shape
    if ps_r > 1:
        y = empty((B, H * ps_r, W * ps_r, Cout // (ps_r * ps_r)), x)
    else:
        y = empty((B, H, W, Cout), x)
    _call("dasr_conv3x3_fwd_split2", _p(x), _p(xmax), _lib.ptr(ws[0], False, torch.float16), _p(ws[1]), _p(bias, True),
          _p(residual, True), _p(y), _p(amax, True), B, H, W, Cin, Cout, act, ps_r)
    return set_amax(y, amax)


def conv3x3_wgrad_split2(x, xmax, dconv, dmax, want_bias=True):
    B, H, W, Cin = x.shape
    Cout = dconv.shape[3]
    nbytes = int(_lib.get().dasr_conv3x3_wgrad_split_workspace(B, H, W, Cin, Cout))
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
    dw = empty((3, 3, Cin, Cout), x)
    db = empty((Cout,), x) if want_bias else None
    _call("dasr_conv3x3_wgrad_split2", _p(x), _p(xmax), _p(dconv), _p(dmax), _p(dw), _p(db, True), _p(ws), nbytes, B, H, W, Cin,
          Cout)
    return dw, db


def conv3x3_dgrad_split2(dconv, dmax, ws, x_shape, out=None):
    B, H, W, Cin = x_shape
    Cout = dconv.shape[3]
    acc = out is not None
    if out is None:
        out = empty(tuple(x_shape), dconv)
    drop_amax(out)
    _call("dasr_conv3x3_dgrad_split2", _p(dconv), _p(dmax), _lib.ptr(ws[0], False, torch.float16), _p(ws[1]), _p(out), 1 if acc else 0, B, H, W, Cin, Cout)
    return out


def conv3x3_dgrad_act_supported(x_shape, Cout, act, ps_r, accumulate=False):
    B, H, W, Cin = x_shape
    return bool(_lib.get().dasr_conv3x3_dgrad_act_supported(H, W, Cin, Cout, act, ps_r, 1 if accumulate else 0))


def conv3x3_dgrad_act_split2(dconv, dmax, ws, x_act, act, ps_r, out=None, amax=None):
    """conv3x3_dgrad_split2 with the producer's activation / PixelShuffle(2) backward in its epilogue (32 produced channels):
    x_act [B,H,W,Cin] is the convolution's saved input.  ps_r = 1: returns dprev [B,H,W,Cin], into ``out`` =
    (dgrad + out) * act'(x_act) when given; ps_r = 2: dprev [B,H/2,W/2,4 Cin].  max |dprev| is left in ``amax`` when given."""
    B, H, W, Cin = x_act.shape
    Cout = dconv.shape[3]
    acc = out is not None
    if out is None:
        out = empty((B, H // 2, W // 2, 4 * Cin) if ps_r == 2 else (B, H, W, Cin), dconv)
    drop_amax(out)
    _call("dasr_conv3x3_dgrad_act_split2", _p(dconv), _p(dmax), _lib.ptr(ws[0], False, torch.float16), _p(ws[1]), _p(x_act),
          _p(out), _p(amax, True), 1 if acc else 0, B, H, W, Cin, Cout, act, ps_r)
    return set_amax(out, amax)


# ---- the 9x9 output convolution in the same scheme (csrc/conv9_split.hip); w = the packed kernel (2,9,9,Cin,Cout) ------
def conv9_split_supported(H, W, Cin, Cout):
    return bool(_lib.get().dasr_conv9_split_supported(H, W, Cin, Cout))


def conv9_fwd_split2(x, xmax, w, wmax, bias):
    B, H, W, Cin = x.shape
    Cout = w.shape[4]
    y = empty((B, H, W, Cout), x)
    _call("dasr_conv9_fwd_split2", _p(x), _p(xmax), _p(w), _p(wmax), _p(bias, True), _p(y), B, H, W, Cin, Cout)
    return y


def conv9_dgrad_split2(dconv, dmax, w, wmax, x_shape, out=None):
    B, H, W, Cin = x_shape
    Cout = dconv.shape[3]
    acc = out is not None
    if out is None:
        out = empty(tuple(x_shape), dconv)
    drop_amax(out)
    _call("dasr_conv9_dgrad_split2", _p(dconv), _p(dmax), _p(w), _p(wmax), _p(out), 1 if acc else 0, B, H, W, Cin, Cout)
    return out


def conv9_dgrad_act_supported(x_shape, Cout, act, ps_r):
    B, H, W, Cin = x_shape
    return (ps_r == 2 and H % 2 == 0 and W % 2 == 0 and act in (ACT_NONE, ACT_RELU, ACT_LRELU)
            and conv9_split_supported(H, W, Cin, Cout))


def conv9_dgrad_act_split2(dconv, dmax, w, wmax, x_act, act, ps_r, amax=None):
    """The 9x9 split dgrad with the producer's activation / PixelShuffle(2) backward in its epilogue: x_act [B,H,W,Cin] is the
    convolution's saved input; returns dprev [B, H/2, W/2, 4 Cin] (max |dprev| left in ``amax`` when given)."""
    B, H, W, Cin = x_act.shape
    Cout = dconv.shape[3]
    dprev = empty((B, H // 2, W // 2, 4 * Cin), dconv)
    _call("dasr_conv9_dgrad_act_split2", _p(dconv), _p(dmax), _p(w), _p(wmax), _p(x_act), _p(dprev), _p(amax, True),
          B, H, W, Cin, Cout, act, ps_r)
    return set_amax(dprev, amax)


def conv9_wgrad_split2(x, xmax, dconv, dmax, want_bias=True):
    B, H, W, Cin = x.shape
    Cout = dconv.shape[3]
    nbytes = int(_lib.get().dasr_conv9_wgrad_split2_workspace(B, H, W, Cin, Cout))
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
    dw = empty((9, 9, Cin, Cout), x)
    db = empty((Cout,), x) if want_bias else None
    _call("dasr_conv9_wgrad_split2", _p(x), _p(xmax), _p(dconv), _p(dmax), _p(dw), _p(db, True), _p(ws), nbytes, B, H, W, Cin, Cout)
    return dw, db


def conv2d_fwd_stats(x, w, bias):
    """3x3 / stride 1 / pad 1 conv (+bias) and the InstanceNorm statistics of its output: (y, mean[B,C], var[B,C])."""
    B, H, W, Cin = x.shape
    KH, KW, Cin2, Cout = w.shape[1:]
    assert (KH, KW) == (3, 3) and Cin2 == Cin
    y = empty((B, H, W, Cout), x)
    mean = empty((B, Cout), x)
    var = empty((B, Cout), x)
    nbytes = int(_lib.get().dasr_conv2d_fwd_stats_workspace(B, H, W, Cin, Cout))
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
    _call("dasr_conv2d_fwd_stats", _p(x), _p(w), _p(bias, True), _p(y), _p(mean), _p(var), _p(ws), nbytes, B, H, W, Cin,
          Cout)
    return y, mean, var


# ---- instance norm / SEAN -------------------------------------------------------------------
def instnorm_stats(x):
    B, H, W, C = x.shape
    mean = empty((B, C), x)
    var = empty((B, C), x)
    nbytes = _lib.get().dasr_instnorm_stats_workspace(B, H * W, C)
    ws = torch.empty((max(1, nbytes // 4),), dtype=torch.float32, device=x.device)
    if x.dtype == BF16:
        _call("dasr_instnorm_stats_bf16", _pa(x), _p(mean), _p(var), _p(ws), nbytes, B, H * W, C)
    else:
        _call("dasr_instnorm_stats", _p(x), _p(mean), _p(var), _p(ws), nbytes, B, H * W, C)
    return mean, var


def dynk_fwd(st, A_w, A_b, Wg, Wb):
    B, K, L = st.shape
    C = Wg.shape[0]
    stp = torch.empty_like(st)
    D = empty((B, 2, 9, K, C), st)
    _call("dasr_dynk_fwd", _p(st), _p(A_w), _p(A_b), _p(Wg), _p(Wb), _p(stp), _p(D), B, K, L, C)
    return stp, D


def dynk_bwd(dD, st, stp, A_w, Wg, Wb, dst_accum):
    """Returns (dWg, dWb, dA_w, dA_b); adds the depth-matrix gradient into ``dst_accum`` in place."""
    B, K, L = st.shape
    C = Wg.shape[0]
    dWg, dWb = torch.empty_like(Wg), torch.empty_like(Wb)
    dA_w = torch.empty_like(A_w)
    dA_b = empty((K,), st)
    scratch = torch.empty_like(st)
    _call("dasr_dynk_bwd", _p(dD), _p(st), _p(stp), _p(A_w), _p(Wg), _p(Wb), _p(dWg), _p(dWb), _p(dA_w), _p(dA_b),
          _p(dst_accum), _p(scratch), B, K, L, C)
    return dWg, dWb, dA_w, dA_b


def soft_mask_max_regions():
    return int(_lib.get().dasr_sean_soft_mask_max_regions())


def mask_compress(mask):
    """Region index per pixel (uint8 [B,H,W]) + device flag (int32 [1], non-zero = masks are not one-hot)."""
    B, K, H, W = mask.shape
    region = torch.empty((B, H, W), dtype=torch.uint8, device=mask.device)
    flag = torch.empty((1,), dtype=torch.int32, device=mask.device)
    _call("dasr_mask_compress", _p(mask), _lib.ptr(region, dtype=torch.uint8), _lib.ptr(flag, dtype=torch.int32), B, K,
          H, W)
    return region, flag


def depth_to_masks(depth, num_masks=10, fixed_edges=None, want_planes=True, out=None):
    """Device getDepthMask (dasr_depth_to_masks): depth [B,1,h,w] or [B,h,w] -> (planes [B,K,h,w] float or None,
    region bytes [B,h,w]).  fixed_edges: None (per-sample min/max range) or K+1 float32 device values.  ``out``:
    ``(planes, region)`` buffers of those shapes to write into instead of new ones."""
    h, w = depth.shape[-2:]
    B = depth.numel() // (h * w)
    d = depth.contiguous()
    if out is not None:
        planes, region = out
        assert tuple(region.shape) == (B, h, w) and (planes is None or tuple(planes.shape) == (B, num_masks, h, w))
    else:
        planes = torch.empty((B, num_masks, h, w), dtype=torch.float32, device=d.device) if want_planes else None
        region = torch.empty((B, h, w), dtype=torch.uint8, device=d.device)
    nbytes = int(_lib.get().dasr_depth_to_masks_workspace(B, h * w))
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=d.device)
    _call("dasr_depth_to_masks", _p(d), _p(fixed_edges, True) if fixed_edges is not None else None,
          _p(planes) if planes is not None else None, _lib.ptr(region, dtype=torch.uint8), _p(ws), nbytes, B, h * w,
          num_masks)
    return planes, region


def depth_to_masks_soft(depth, num_masks=10, width=1.0, fixed_range=False, out=None, pair=False):
    """Soft (hat-function) membership planes (dasr_depth_to_masks_soft): depth [B,1,h,w] or [B,h,w] float32 -> planes
    [B,K,h,w] float32, at most two non-zero per pixel, summing to 1.  ``width`` in (0, 1]: the share of a bin over which
    two neighbours blend (1: linear interpolation between bin centres).  ``fixed_range``: bins over [0,1] instead of the
    sample's own [min, max].  ``out``: a ``[B,K,h,w]`` buffer to write into instead of a new one.
    ``pair=True`` (dasr_depth_to_masks_soft_pair, the same launch): returns ``(planes, pair_k, pair_s)`` - the planes, bit
    for bit those of ``pair=False``, and their pair encoding (include/dasr.h), uint8 and float32 ``[B,h,w]``."""
    if depth.dtype != torch.float32:
        raise TypeError("depth_to_masks_soft: depth must be float32, got %s" % depth.dtype)
    if not 0.0 < float(width) <= 1.0:                    # False for NaN too
        raise ValueError("depth_to_masks_soft: width must be in (0, 1], got %r" % (width,))
    if not 1 <= int(num_masks) <= 16:
        raise ValueError("depth_to_masks_soft: num_masks must be in 1..16, got %r" % (num_masks,))
    h, w = depth.shape[-2:]
    B = depth.numel() // (h * w)
    d = depth.contiguous()
    if out is not None:
        planes = out
        if tuple(planes.shape) != (B, num_masks, h, w):
            raise ValueError("depth_to_masks_soft: out must be [%d,%d,%d,%d], got %s" % (B, num_masks, h, w, tuple(planes.shape)))
    else:
        planes = torch.empty((B, num_masks, h, w), dtype=torch.float32, device=d.device)
    nbytes = int(_lib.get().dasr_depth_to_masks_soft_workspace(B, h * w))
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=d.device)
    if pair:
        pair_k = torch.empty((B, h, w), dtype=torch.uint8, device=d.device)
        pair_s = torch.empty((B, h, w), dtype=torch.float32, device=d.device)
        _call("dasr_depth_to_masks_soft_pair", _p(d), _p(planes), _lib.ptr(pair_k, dtype=torch.uint8), _p(pair_s), _p(ws),
              nbytes, B, h * w, int(num_masks), float(width), int(bool(fixed_range)))
        return planes, pair_k, pair_s
    _call("dasr_depth_to_masks_soft", _p(d), _p(planes), _p(ws), nbytes, B, h * w, int(num_masks), float(width),
          int(bool(fixed_range)))
    return planes


def _rf(region, flag):
    if region is None:
        return None, None
    return _lib.ptr(region, dtype=torch.uint8), (_lib.ptr(flag, dtype=torch.int32) if flag is not None else None)


def sean_fwd(t, mean, var, gb2, mask, region, flag, D, bias_g, bias_b, alpha_g, alpha_b, residual, relu, amax=None):
    B, H, W, C = t.shape
    K = mask.shape[1]
    assert mask.shape == (B, K, H, W) and gb2.shape == (B, H, W, 2 * C) and D.shape == (B, 2, 9, K, C)
    out = torch.empty_like(t)
    rp, fp = _rf(region, flag)
    if _is_bf(t, gb2, residual):
        _call("dasr_sean_fwd_bf16", _pa(t), _p(mean), _p(var), _pa(gb2), _p(mask), rp, fp, _p(D), _p(bias_g), _p(bias_b),
              _p(alpha_g), _p(alpha_b), _pa(residual, True), _pa(out), int(relu), B, H, W, C, K, IN_EPS)
    else:
        _call("dasr_sean_fwd", _p(t), _p(mean), _p(var), _p(gb2), _p(mask), rp, fp, _p(D), _p(bias_g), _p(bias_b),
              _p(alpha_g), _p(alpha_b), _p(residual, True), _p(out), _p(amax, True), int(relu), B, H, W, C, K, IN_EPS)
        set_amax(out, amax)
    return out


def sean_fwd_pair(t, mean, var, gb2, pair_k, pair_s, D, bias_g, bias_b, alpha_g, alpha_b, residual, relu, amax=None):
    """``sean_fwd`` for a soft mask in the pair encoding (dasr_sean_fwd_pair[_bf16]): ``pair_k`` uint8 and ``pair_s``
    float32 ``[B,H,W]`` instead of the planes.  Forward only - the backward is ``sean_bwd`` on the planes."""
    B, H, W, C = t.shape
    K = D.shape[3]
    assert pair_k.shape == (B, H, W) and pair_s.shape == (B, H, W) and gb2.shape == (B, H, W, 2 * C)
    assert D.shape == (B, 2, 9, K, C)
    out = torch.empty_like(t)
    kp = _lib.ptr(pair_k, dtype=torch.uint8)
    if _is_bf(t, gb2, residual):
        _call("dasr_sean_fwd_pair_bf16", _pa(t), _p(mean), _p(var), _pa(gb2), kp, _p(pair_s), _p(D), _p(bias_g), _p(bias_b),
              _p(alpha_g), _p(alpha_b), _pa(residual, True), _pa(out), int(relu), B, H, W, C, K, IN_EPS)
    else:
        _call("dasr_sean_fwd_pair", _p(t), _p(mean), _p(var), _p(gb2), kp, _p(pair_s), _p(D), _p(bias_g), _p(bias_b),
              _p(alpha_g), _p(alpha_b), _p(residual, True), _p(out), _p(amax, True), int(relu), B, H, W, C, K, IN_EPS)
        set_amax(out, amax)
    return out


def sean_bwd(dout, out, t, mean, var, gb2, mask, region, flag, D, bias_g, bias_b, alpha_g, alpha_b, relu, want_dres,
             dt_amax=None, dgb2_amax=None):
    B, H, W, C = t.shape
    K = mask.shape[1]
    lib = _lib.get()
    nbytes = lib.dasr_sean_bwd_workspace(B, H, W, C, K)
    ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=t.device)
    dt = torch.empty_like(t)
    dgb2 = torch.empty_like(gb2)
    dD = torch.empty_like(D)
    dbg, dbb = empty((C,), t), empty((C,), t)        # fp32 whatever the activation dtype
    dag, dab = empty((1,), t), empty((1,), t)
    dres = torch.empty_like(t) if want_dres else None
    rp, fp = _rf(region, flag)
    if _is_bf(dout, out, t, gb2):
        _call("dasr_sean_bwd_bf16", _pa(dout), _pa(out), _pa(t), _p(mean), _p(var), _pa(gb2), _p(mask), rp, fp, _p(D), _p(bias_g),
              _p(bias_b), _p(alpha_g), _p(alpha_b), _pa(dt), _pa(dgb2), _p(dD), _p(dbg), _p(dbb), _p(dag), _p(dab),
              _pa(dres, True), _p(ws), nbytes, int(relu), B, H, W, C, K, IN_EPS)
    else:
        _call("dasr_sean_bwd", _p(dout), _p(out), _p(t), _p(mean), _p(var), _p(gb2), _p(mask), rp, fp, _p(D), _p(bias_g),
              _p(bias_b), _p(alpha_g), _p(alpha_b), _p(dt), _p(dgb2), _p(dD), _p(dbg), _p(dbb), _p(dag), _p(dab),
              _p(dres, True), _p(dt_amax, True), _p(dgb2_amax, True), _p(ws), nbytes, int(relu), B, H, W, C, K, IN_EPS)
        set_amax(dt, dt_amax)
        set_amax(dgb2, dgb2_amax)
    return dt, dgb2, dD, dbg, dbb, dag, dab, dres


# ---- region pooling -------------------------------------------------------------------------
def region_pool_fwd(feat, mask):
    B, h, w, L = feat.shape
    _, K, H, W = mask.shape
    maskr = empty((B, K, h, w), feat)
    area = empty((B, K), feat)
    out = empty((B, K, L), feat)
    _call("dasr_region_pool_fwd", _p(feat), _p(mask), _p(maskr), _p(area), _p(out), B, K, L, h, w, H, W)
    return out, maskr, area


def region_pool_bwd(dout, maskr, area, feat_shape):
    B, h, w, L = feat_shape
    K = maskr.shape[1]
    dfeat = torch.empty(feat_shape, dtype=torch.float32, device=dout.device)
    _call("dasr_region_pool_bwd", _p(dout), _p(maskr), _p(area), _p(dfeat), B, K, L, h, w)
    return dfeat


# ---- harness losses: csrc/loss.hip, one kernel family with two criterion policies ------------------------------------
LOSS_MAX_REGIONS = 16
CRIT_CODES = {"l1": 0, "l2": 1, "cb": 2, "smoothl1": 3}       # DASR_CRIT_*; None -> DASR_CRIT_NONE


def _loss_dims(sr, hr, aux, K):
    """``aux``: region bytes [B,h,w] (uint8, dasr_mask_compress) or float masks [B,K,h,w]; -> (soft, aux pointer, B, C, h,
    w, scale) of an integer HR / LR scale."""
    B, C, H, W = sr.shape
    soft = aux.dtype != torch.uint8
    h, w = aux.shape[-2:]
    scale = H // h
    assert hr.shape == sr.shape and aux.shape[:-2] == ((B, K) if soft else (B,)) and H == h * scale and W == w * scale
    return soft, _p(aux) if soft else _lib.ptr(aux, dtype=torch.uint8), B, C, h, w, scale


def _loss_call(name, sr, hr, aux, dsums, K, crits=None):
    """One of the eight entry points dasr_loss_{sums,bwd}[_soft][_crit]: ``dsums`` None - the sums; otherwise dsr.
    ``crits`` None: the fixed policy (pixel l1, region smooth-L1); (pixel, A, B or None): the criteria as arguments."""
    soft, aux_p, B, C, h, w, scale = _loss_dims(sr, hr, aux, K)
    nsums = (2 if crits is None or crits[2] is None else 3) * K + 1
    codes = () if crits is None else tuple(-1 if c is None else CRIT_CODES[c] for c in crits)
    if dsums is None:
        out, mid = empty((nsums,), sr), ()
    else:
        assert dsums.numel() == nsums
        out, mid = torch.empty_like(sr), (_p(dsums),)
    _call("dasr_loss_" + name + ("_soft" if soft else "") + ("" if crits is None else "_crit"), _p(sr), _p(hr), aux_p, *mid,
          _p(out), B, C, h, w, scale, K, *codes)
    return out


def loss_sums(sr, hr, region, K):
    """K smooth-L1 numerators | K areas | sum|sr-hr| for region bytes [B,h,w] (dasr_loss_sums)."""
    return _loss_call("sums", sr, hr, region, None, K)


def loss_bwd(sr, hr, region, dsums, K):
    return _loss_call("bwd", sr, hr, region, dsums, K)


def loss_sums_soft(sr, hr, mask, K):
    """K numerators sum smooth_l1(M_k (sr-hr)) | K areas | sum|sr-hr| for float masks [B,K,h,w] (dasr_loss_sums_soft)."""
    return _loss_call("sums", sr, hr, mask, None, K)


def loss_bwd_soft(sr, hr, mask, dsums, K):
    return _loss_call("bwd", sr, hr, mask, dsums, K)


def loss_sums_crit(sr, hr, aux, K, pixel, crit_a, crit_b=None):
    """K numerators of criterion A | K areas | the pixel criterion's sum | with ``crit_b``: K numerators of criterion B
    (dasr_loss_sums_crit / dasr_loss_sums_soft_crit).  ``pixel``: 'l1' | 'l2' | 'cb'; ``crit_a`` / ``crit_b``:
    'l1' | 'l2' | 'smoothl1'."""
    return _loss_call("sums", sr, hr, aux, None, K, (pixel, crit_a, crit_b))


def loss_bwd_crit(sr, hr, aux, dsums, K, pixel, crit_a, crit_b=None):
    """dsr from the device vector ``dsums`` (the layout of loss_sums_crit's result; the areas' entries are not read)."""
    return _loss_call("bwd", sr, hr, aux, dsums, K, (pixel, crit_a, crit_b))


# ---- SSIM: validation metric and training criterion (csrc/ssim.hip, csrc/ssim_bwd.hip) ----------
_ssim_window = None


def _ssim_window11():
    """The reference's eleven 1-D window weights as a host array (the entry points take them by value)."""
    global _ssim_window
    if _ssim_window is None:
        from .validate import _window_1d
        _ssim_window = (ctypes.c_float * 11)(*[float(v) for v in _window_1d()])
    return ctypes.cast(_ssim_window, ctypes.c_void_p)


def ssim(img1, img2):
    """Per-sample mean of the SSIM map of two [B,C,H,W] images (dasr_ssim): float32 [B]."""
    a, b = img1.contiguous().float(), img2.contiguous().float()
    B, C, H, W = a.shape
    out = torch.empty((B,), dtype=torch.float32, device=a.device)
    nbytes = int(_lib.get().dasr_ssim_workspace(B, C, H, W))
    ws = torch.empty((max(1, nbytes // 4),), dtype=torch.float32, device=a.device)
    _call("dasr_ssim", _p(a), _p(b), _ssim_window11(), _p(out), _p(ws), nbytes, B, C, H, W)
    return out


def ssim_bwd(img1, img2, dscale, out=None, accumulate=False):
    """dscale * dS/dimg1 for S = the mean of the SSIM map over all of [B,C,H,W] (dasr_ssim_bwd, one launch).  ``dscale``:
    a float32 tensor of one element on the images' device (never read by the host).  ``out``: the buffer to write, or with
    ``accumulate`` to add into; a new one by default."""
    B, C, H, W = img1.shape
    assert img2.shape == img1.shape and dscale.numel() == 1
    if out is None:
        assert not accumulate, "ssim_bwd: accumulate needs the buffer to add into"
        out = torch.empty_like(img1)
    assert out.shape == img1.shape
    _call("dasr_ssim_bwd", _p(img1), _p(img2), _ssim_window11(), _p(dscale), _p(out), int(bool(accumulate)), B, C, H, W)
    return out


# ---- video frames: the uint8 edge of inference (csrc/frame.hip) --------------------------------
def _pu8(t):
    return _lib.ptr(t, dtype=torch.uint8)


def frame_ingest_u8(frames, swap_rb=True, out=None):
    """uint8 [B,H,W,C] (HWC, BGR when C == 3 and swap_rb) -> float32 NHWC RGB [B,H,W,C] = frames / 255 (dasr_frame_ingest_u8)."""
    B, H, W, C = frames.shape
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=frames.device)
    assert tuple(out.shape) == (B, H, W, C)
    drop_amax(out)
    _call("dasr_frame_ingest_u8", _pu8(frames), _p(out), B, H, W, C, int(bool(swap_rb)))
    return out


def frame_emit_u8(y, net_lo, net_hi, min_max=(0, 1), swap_rb=True, out=None):
    """float32 NHWC [B,H,W,C] before the output clamp -> uint8 [B,H,W,C] (BGR when C == 3 and swap_rb): clamp to the net's
    range, then tensor2img's clamp / rescale / round(x * 255) (dasr_frame_emit_u8)."""
    B, H, W, C = y.shape
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.uint8, device=y.device)
    assert tuple(out.shape) == (B, H, W, C)
    _call("dasr_frame_emit_u8", _p(y), _pu8(out), B, H, W, C, float(net_lo), float(net_hi), float(min_max[0]),
          float(min_max[1]), int(bool(swap_rb)))
    return out


def frame_ssd_u8(a, b, crop=0, out=None):
    """Exact sum of squared differences per frame of two uint8 [B,H,W,C] batches inside a ``crop``-pixel border, as int64
    [B] on the device (dasr_frame_ssd_u8 writes unsigned 64-bit sums; they stay below 2^63 for any image that fits memory)."""
    assert a.shape == b.shape
    B, H, W, C = a.shape
    if out is None:
        out = torch.empty((B,), dtype=torch.int64, device=a.device)
    assert out.numel() == B
    nbytes = int(_lib.get().dasr_frame_ssd_u8_workspace(B, H, W, C, int(crop)))
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device=a.device)
    _call("dasr_frame_ssd_u8", _pu8(a), _pu8(b), _lib.ptr(out, dtype=torch.int64), _lib.ptr(ws, dtype=torch.int64), nbytes,
          B, H, W, C, int(crop))
    return out


# ---- the test script's metrics of uint8 images (csrc/metrics.hip) ------------------------------
def image_metrics_u8(a, b, crop=0, out=None):
    """The sums behind PSNR, SSIM, PSNR_Y and SSIM_Y of the reference's test script for two uint8 [B,H,W,C] batches (C = 3:
    BGR; C = 1) inside a ``crop``-pixel border: ``(ssd int64 [B], sums float64 [B,3])`` on the device - the exact sum of
    squared differences, the sum of squared luma differences, the sum of the float64 valid-window SSIM map over positions
    and channels, and that of the luma image (dasr_image_metrics_u8; ``validate.image_metrics`` turns them into the four
    figures).  ``out``: ``(ssd, sums)`` tensors to write into, e.g. slices of a caller's result buffers.  Refused with
    ValueError: C other than 1 or 3, fewer than 11 rows or columns left inside the border."""
    for t, nm in ((a, "a"), (b, "b")):
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4:
            raise TypeError("dasr_amd: image_metrics_u8: %s must be a uint8 [B,H,W,C] tensor" % nm)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("dasr_amd: image_metrics_u8: a %s on %s and b %s on %s do not belong together"
                         % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    B, H, W, C = a.shape
    crop = int(crop)
    if C not in (1, 3):
        raise ValueError("dasr_amd: image_metrics_u8: C must be 1 or 3, got %d" % C)
    if B < 1 or crop < 0 or H - 2 * crop < 11 or W - 2 * crop < 11:
        raise ValueError("dasr_amd: image_metrics_u8: %dx%d frames with a border of %d leave less than the 11x11 window"
                         % (H, W, crop))
    if out is None:
        ssd = torch.empty((B,), dtype=torch.int64, device=a.device)
        sums = torch.empty((B, 3), dtype=torch.float64, device=a.device)
    else:
        ssd, sums = out
        if ssd.dtype != torch.int64 or ssd.numel() != B or sums.dtype != torch.float64 or sums.numel() != 3 * B \
                or ssd.device != a.device or sums.device != a.device:
            raise ValueError("dasr_amd: image_metrics_u8: out must be (int64 [%d], float64 [%d,3]) on %s" % (B, B, a.device))
    nbytes = int(_lib.get().dasr_image_metrics_u8_workspace(B, H, W, C, crop))
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device=a.device)
    _call("dasr_image_metrics_u8", _pu8(a), _pu8(b), _lib.ptr(ssd, dtype=torch.int64), _lib.ptr(sums, dtype=torch.float64),
          _lib.ptr(ws, dtype=torch.int64), nbytes, B, H, W, C, crop)
    return ssd, sums


# ---- training batches from uint8 HR frames (csrc/batch.hip) --------------------------------------------------------
def _pi32(t, allow_none=False):
    return _lib.ptr(t, allow_none, dtype=torch.int32)


def _batch_tables(B, origins, flags, device):
    """Pointers of the per-sample device tables (None: no crop offset / no augmentation) after a shape and dtype check."""
    if origins is not None and (origins.dtype != torch.int32 or tuple(origins.shape) != (B, 2)):
        raise TypeError("dasr_amd: origins must be int32 [B,2], got %s %s" % (origins.dtype, tuple(origins.shape)))
    if flags is not None and (flags.dtype != torch.uint8 or tuple(flags.shape) != (B,)):
        raise TypeError("dasr_amd: flags must be uint8 [B], got %s %s" % (flags.dtype, tuple(flags.shape)))
    return _pi32(origins, True), (_pu8(flags) if flags is not None else None)


def _batch_out(out, shape, dtype, like):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if tuple(out.shape) != tuple(shape):
        raise ValueError("dasr_amd: out has shape %s, expected %s" % (tuple(out.shape), tuple(shape)))
    drop_amax(out)
    return out


def _batch_check(name, rc):
    """Shape refusals of the batch entry points are the caller's error: ValueError, like the Python-side checks."""
    if rc in (-2, -3):
        msg = _lib.get().dasr_error_string(rc)
        raise ValueError("dasr_amd: %s refused: %s (code %d)" % (name, msg.decode() if msg else "?", rc))
    _lib.check(rc, name)


def batch_lr_u8(frames, scale, tables, window=None, origins=None, flags=None, allow_transpose=False, out=None):
    """uint8 [B,H,W,3] HWC BGR -> float32 [B,3,ch,cw] NCHW RGB: the reference's LR image ``imresize_np(frames / 255,
    1 / scale, True)``, its window ``(ch, cw)`` at the per-sample ``origins``, augmented by the per-sample ``flags``
    (dasr_batch_lr_u8).  ``tables`` = (wh, ih, ww, iw) device tensors from ``data.resize_tables``; ``window`` None: the
    whole LR image; ``origins`` int32 [B,2] / ``flags`` uint8 [B] on the device, or None."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise TypeError("dasr_amd: frames must be uint8 [B,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
    B, H, W, _ = frames.shape
    s = int(scale)
    if s <= 0 or H % s or W % s:
        raise ValueError("dasr_amd: frame size %dx%d is not a multiple of the scale %d" % (H, W, s))
    wh, ih, ww, iw = tables
    if tuple(wh.shape) != (H // s, 4 * s) or tuple(ww.shape) != (W // s, 4 * s) or ih.numel() != H // s or iw.numel() != W // s:
        raise ValueError("dasr_amd: resize tables do not belong to %dx%d frames at scale %d" % (H, W, s))
    ch, cw = (H // s, W // s) if window is None else (int(window[0]), int(window[1]))
    po, pf = _batch_tables(B, origins, flags, frames.device)
    out = _batch_out(out, (B, 3, ch, cw), torch.float32, frames)
    rc = _lib.get().dasr_batch_lr_u8(_pu8(frames), _p(out), _p(wh), _pi32(ih), _p(ww), _pi32(iw), po, pf, B, H, W, s, ch, cw,
                                     int(bool(allow_transpose)), _lib.stream())
    _batch_check("dasr_batch_lr_u8", rc)
    return out


def batch_gt_u8(frames, scale, window=None, origins=None, flags=None, allow_transpose=False, out=None):
    """uint8 [B,H,W,3] HWC BGR -> float32 [B,3,s*ch,s*cw] NCHW RGB GT: ``frames / 255`` (the values of
    ``frame_ingest_u8``) of the HR window that belongs to the LR ``window`` at ``origins``, augmented (dasr_batch_gt_u8)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise TypeError("dasr_amd: frames must be uint8 [B,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
    B, H, W, _ = frames.shape
    s = int(scale)
    if s <= 0 or H % s or W % s:
        raise ValueError("dasr_amd: frame size %dx%d is not a multiple of the scale %d" % (H, W, s))
    ch, cw = (H // s, W // s) if window is None else (int(window[0]), int(window[1]))
    po, pf = _batch_tables(B, origins, flags, frames.device)
    out = _batch_out(out, (B, 3, s * ch, s * cw), torch.float32, frames)
    rc = _lib.get().dasr_batch_gt_u8(_pu8(frames), _p(out), po, pf, B, H, W, s, ch, cw, int(bool(allow_transpose)),
                                     _lib.stream())
    _batch_check("dasr_batch_gt_u8", rc)
    return out


def batch_plane(x, window=None, origins=None, flags=None, allow_transpose=False, out=None):
    """float32 or uint8 [B,C,h,w] -> [B,C,ch,cw]: the window of every plane, augmented (dasr_batch_plane_f32 / _u8): the
    depth map, the mask planes, the region bytes ([B,h,w] uint8 is taken as C = 1 and returned as [B,ch,cw])."""
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("dasr_amd: batch_plane takes float32 or uint8, got %s" % x.dtype)
    if x.dim() not in (3, 4):
        raise TypeError("dasr_amd: batch_plane takes [B,C,h,w] or [B,h,w], got %s" % (tuple(x.shape),))
    B, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    C = x.shape[1] if x.dim() == 4 else 1
    ch, cw = (h, w) if window is None else (int(window[0]), int(window[1]))
    po, pf = _batch_tables(B, origins, flags, x.device)
    out = _batch_out(out, (B, C, ch, cw) if x.dim() == 4 else (B, ch, cw), x.dtype, x)
    if x.dtype == torch.float32:
        rc = _lib.get().dasr_batch_plane_f32(_p(x), _p(out), po, pf, B, C, h, w, ch, cw, int(bool(allow_transpose)),
                                             _lib.stream())
    else:
        rc = _lib.get().dasr_batch_plane_u8(_pu8(x), _pu8(out), po, pf, B, C, h, w, ch, cw, int(bool(allow_transpose)),
                                            _lib.stream())
    _batch_check("dasr_batch_plane", rc)
    return out


# ---- geometric self-ensemble inference (csrc/ensemble.hip) ---------------------------------------------------------------
def _ensemble_outs(name, out, N, H, W, C, dtype, like):
    """The two group buffers ``([4N,H,W,C], [4N,W,H,C])`` of an expand: the caller's, shape-checked, or new ones."""
    shapes = ((4 * N, H, W, C), (4 * N, W, H, C))
    if out is None:
        return tuple(torch.empty(s, dtype=dtype, device=like.device) for s in shapes)
    a, t = out
    if tuple(a.shape) != shapes[0] or tuple(t.shape) != shapes[1]:
        raise ValueError("dasr_amd: %s out has shapes %s / %s, expected %s / %s"
                         % (name, tuple(a.shape), tuple(t.shape), shapes[0], shapes[1]))
    drop_amax(a)
    drop_amax(t)
    return a, t


def ensemble_expand(x, out=None):
    """float32 or uint8 ``[N,H,W,C]`` (C in 1, 3) -> ``(a [4N,H,W,C], t [4N,W,H,C])``: the eight flip / transpose members
    of the reference's test_x8 (dasr_ensemble_expand_f32 / _u8; member numbering and layout in include/dasr.h), a
    bit-exact move.  ``out``: ``(a, t)`` buffers of those shapes to write into instead of new ones."""
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("dasr_amd: ensemble_expand takes float32 or uint8, got %s" % x.dtype)
    if x.dim() != 4:
        raise TypeError("dasr_amd: ensemble_expand takes [N,H,W,C], got %s" % (tuple(x.shape),))
    N, H, W, C = x.shape
    a, t = _ensemble_outs("ensemble_expand", out, N, H, W, C, x.dtype, x)
    if x.dtype == torch.float32:
        rc = _lib.get().dasr_ensemble_expand_f32(_p(x), _p(a), _p(t), N, H, W, C, _lib.stream())
    else:
        rc = _lib.get().dasr_ensemble_expand_u8(_pu8(x), _pu8(a), _pu8(t), N, H, W, C, _lib.stream())
    _batch_check("dasr_ensemble_expand", rc)
    return a, t


def ensemble_ingest_u8(frames, swap_rb=True, out=None):
    """uint8 ``[N,H,W,C]`` camera frames -> the eight float32 members ``(a, t)``: ``ensemble_expand(frame_ingest_u8(frames,
    swap_rb))`` bit for bit, in one pass (dasr_ensemble_ingest_u8)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise TypeError("dasr_amd: frames must be uint8 [N,H,W,C], got %s %s" % (frames.dtype, tuple(frames.shape)))
    N, H, W, C = frames.shape
    a, t = _ensemble_outs("ensemble_ingest_u8", out, N, H, W, C, torch.float32, frames)
    rc = _lib.get().dasr_ensemble_ingest_u8(_pu8(frames), _p(a), _p(t), N, H, W, C, int(bool(swap_rb)), _lib.stream())
    _batch_check("dasr_ensemble_ingest_u8", rc)
    return a, t


def ensemble_merge(y_a, y_t, lo, hi, out=None):
    """``y_a [4N,H,W,C]``, ``y_t [4N,W,H,C]`` float32 (the members' results before the output clamp) -> ``[N,H,W,C]``:
    every member mapped back and clamped to ``[lo, hi]`` (NaN kept), summed in member order, times 0.125
    (dasr_ensemble_merge)."""
    if y_a.dim() != 4 or y_t.dim() != 4 or y_a.shape[0] % 4 or \
            tuple(y_t.shape) != (y_a.shape[0], y_a.shape[2], y_a.shape[1], y_a.shape[3]):
        raise ValueError("dasr_amd: ensemble_merge takes [4N,H,W,C] and [4N,W,H,C], got %s and %s"
                         % (tuple(y_a.shape), tuple(y_t.shape)))
    N, H, W, C = y_a.shape[0] // 4, y_a.shape[1], y_a.shape[2], y_a.shape[3]
    out = _batch_out(out, (N, H, W, C), torch.float32, y_a)
    rc = _lib.get().dasr_ensemble_merge(_p(y_a), _p(y_t), _p(out), N, H, W, C, float(lo), float(hi), _lib.stream())
    _batch_check("dasr_ensemble_merge", rc)
    return out
