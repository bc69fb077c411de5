"""Soft (non one-hot) depth masks on the fp32-MFMA dynamic-convolution kernels (csrc/sean.hip, k_sean_fwd_soft /
k_sean_bwd_a_soft), up to 16 regions.  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X);
tests/test_soft_masks.py runs every one of them on both."""
import itertools

import torch
import torch.nn.functional as F

from dasr_amd import graph, ops, synth
from dasr_amd.depthnet import DepthNet
from oracle import depthnet_oracle as O
from tests.parity_checks import _compare_with_oracle, build_net, nchw, nhwc, rel_max  # noqa: F401

BF16 = torch.bfloat16
GRAD_NAMES = ("dt", "dgb2", "dD", "dbg", "dbb", "dag", "dab", "dres")
# B = 2, H = 9, W = 33: one column past a 32-wide tile, one row past an 8-row tile (two tile rows, two tile columns)
B_, H_, W_ = 2, 9, 33
CK_CASES = ((64, 10), (64, 16), (32, 16), (64, 7), (64, 1))


def _bf(x):
    return x.to(BF16).float()


def _onehot(B, K, H, W):
    return synth.closed_form_batch(1, B, H, W, 1, K)[3].float()


def make_mask(kind, B, K, H, W, gen):
    """(a) 0.7*onehot + 0.3*rand; (b) exact zeros, negative values and values > 1; (c) sample 0 one-hot, sample 1 soft."""
    mk = _onehot(B, K, H, W)
    rnd = torch.rand(mk.shape, generator=gen)
    if kind == "a":
        return 0.7 * mk + 0.3 * rnd
    if kind == "b":
        m = 3.0 * rnd - 1.0                                   # in [-1, 2): negative values and values above 1
        m[torch.rand(mk.shape, generator=gen) < 0.3] = 0.0    # exact zeros
        assert (m == 0).any() and (m < 0).any() and (m > 1).any()
        return m
    assert kind == "c" and B >= 2
    m = mk.clone()
    m[1] = 0.7 * mk[1] + 0.3 * rnd[1]
    return m


def make_inputs(C, K, gen, B=B_, H=H_, W=W_, bf_valued=False):
    rn = lambda *s: torch.randn(*s, generator=gen)
    q = _bf if bf_valued else (lambda x: x)
    return dict(t=q(rn(B, H, W, C)), gb2=q(rn(B, H, W, 2 * C)), res=q(rn(B, H, W, C)), D=rn(B, 2, 9, K, C) * 0.1,
                bg=rn(C) * 0.1, bb=rn(C) * 0.1, ag=torch.full((1,), 0.7), ab=torch.full((1,), 0.74),
                dout=q(rn(B, H, W, C)))


def reference_f64(inp, mask, relu, use_res):
    """float64 restatement: IN(IN(t)), the dynamic convolution as F.conv2d of the mask with D[b] as [2C, K, 3, 3],
    the DFN modulation, residual, ReLU; gradients by autograd.  Returns (out NHWC, the eight gradients)."""
    d = {k: v.double().clone().requires_grad_(True) for k, v in inp.items() if k != "dout"}
    B, H, W, C = inp["t"].shape
    K = mask.shape[1]
    xh = F.instance_norm(F.instance_norm(nchw(d["t"]), eps=ops.IN_EPS), eps=ops.IN_EPS)
    gb1 = []
    for b in range(B):
        # D[b][s][tap][k][c] -> weight [(s, c), k, dy, dx]
        w = d["D"][b].reshape(2, 3, 3, K, C).permute(0, 4, 3, 1, 2).reshape(2 * C, K, 3, 3)
        gb1.append(F.conv2d(mask[b:b + 1].double(), w, padding=1))
    gb1 = torch.cat(gb1, 0)
    g1 = gb1[:, :C] + d["bg"].reshape(1, C, 1, 1)
    b1 = gb1[:, C:] + d["bb"].reshape(1, C, 1, 1)
    gb2 = nchw(d["gb2"])
    g2, b2 = gb2[:, :C], gb2[:, C:]
    ag, ab = d["ag"], d["ab"]
    pre = xh * (1 + ag * g1 + (1 - ag) * g2) + ab * b1 + (1 - ab) * b2
    # `res` always enters with unit weight so that its gradient is dout*relu' (what dres holds); its VALUE only if used
    r = nchw(d["res"])
    pre = pre + (r if use_res else r - r.detach())
    out = torch.relu(pre) if relu else pre
    out.backward(nchw(inp["dout"].double()))
    grads = (d["t"].grad, d["gb2"].grad, d["D"].grad, d["bg"].grad, d["bb"].grad, d["ag"].grad, d["ab"].grad,
             d["res"].grad)
    return nhwc(out.detach()), grads


def run_kernels(inp, mask, device, relu, use_res, region_flag="compress", dtype=torch.float32):
    dev = lambda x: x.to(device)
    act = lambda x: dev(x).to(dtype)
    m = dev(mask).contiguous()
    if region_flag == "compress":
        region, flag = ops.mask_compress(m)
    elif region_flag == "region_only":
        region, flag = ops.mask_compress(m)[0], None
    else:
        region, flag = None, None
    mean, var = ops.instnorm_stats(act(inp["t"]))
    common = (m, region, flag, dev(inp["D"]), dev(inp["bg"]), dev(inp["bb"]), dev(inp["ag"]), dev(inp["ab"]))
    y = ops.sean_fwd(act(inp["t"]), mean, var, act(inp["gb2"]), *common, act(inp["res"]) if use_res else None, relu)
    g = ops.sean_bwd(act(inp["dout"]), y, act(inp["t"]), mean, var, act(inp["gb2"]), *common, relu, True)
    return y, g


def check_soft_op_vs_float64(device):
    """Output and all eight gradients of the soft-mask SEAN kernels against float64, gated at the project's op-level
    bound rel_max <= 2e-4 (check_sean_golden).  Shapes B = 2, H = 9, W = 33 for (C, K) in CK_CASES, relu x residual in
    all four combinations, masks (a), (b), (c) of make_mask: 60 small launches.  Measured with the scalar general kernels
    this replaces (K <= 14, same inputs, MI355X): see DESIGN.md 4.1."""
    worst = {}
    combos = list(itertools.product((False, True), (False, True)))
    for ci, (C, K) in enumerate(CK_CASES):
        gen = torch.Generator().manual_seed(100 + ci)
        inp = make_inputs(C, K, gen)
        for mi, kind in enumerate(("a", "b", "c")):
            mask = make_mask(kind, B_, K, H_, W_, gen)
            for ri, (relu, use_res) in enumerate(combos):
                y, g = run_kernels(inp, mask, device, relu, use_res)
                ref, gref = reference_f64(inp, mask, relu, use_res)
                errs = {"out": rel_max(y, ref)}
                for nm, a, r in zip(GRAD_NAMES, g, gref):
                    errs[nm] = rel_max(a, r)
                print("soft op C=%d K=%d mask=%s relu=%d res=%d: %s" %
                      (C, K, kind, relu, use_res, " ".join("%s=%.2e" % kv for kv in errs.items())))
                assert max(errs.values()) <= 2e-4, (C, K, kind, relu, use_res, errs)
                for nm, e in errs.items():
                    worst[nm] = max(worst.get(nm, 0.0), e)
    return worst


def check_soft_dispatch(device):
    """Soft masks: (region, flag) from ops.mask_compress and (None, None) give bitwise equal outputs and gradients (the
    gather kernel stood aside).  One-hot masks: (region, flag) is bitwise (region, None) (the soft kernel stood aside).
    Bitwise: out, dgb2, dD, dres everywhere, and every gradient on the emulator.  On the GPU dt (through the per-(b,c)
    sums), dbias and dalpha are accumulated over workgroups with float atomics in the one-hot AND the soft pass A, so two
    runs of the SAME kernel differ in summation order; they are held to the 1e-5 "summation-order noise" bound of
    check_bf16_ops_vs_fp32_kernels there."""
    gen = torch.Generator().manual_seed(7)
    for C, K in ((64, 16), (32, 10)):
        inp = make_inputs(C, K, gen)
        soft = make_mask("c", B_, K, H_, W_, gen)
        ya, ga = run_kernels(inp, soft, device, True, True, "compress")
        yb, gb = run_kernels(inp, soft, device, True, True, "none")
        assert torch.equal(ya, yb), ("soft fwd", C, K)
        for nm, a, b in zip(GRAD_NAMES, ga, gb):
            if nm in ("dt", "dbg", "dbb", "dag", "dab") and device != "cpu":
                # per-channel sums are accumulated over workgroups with float atomics (order not fixed on the GPU)
                assert rel_max(a, b) <= 1e-5, ("soft bwd", nm, C, K)
            else:
                assert torch.equal(a, b), ("soft bwd", nm, C, K)
        hard = _onehot(B_, K, H_, W_)
        ya, ga = run_kernels(inp, hard, device, True, True, "compress")
        yb, gb = run_kernels(inp, hard, device, True, True, "region_only")
        assert torch.equal(ya, yb), ("one-hot fwd", C, K)
        for nm, a, b in zip(GRAD_NAMES, ga, gb):
            if nm in ("dt", "dbg", "dbb", "dag", "dab") and device != "cpu":
                assert rel_max(a, b) <= 1e-5, ("one-hot bwd", nm, C, K)
            else:
                assert torch.equal(a, b), ("one-hot bwd", nm, C, K)
    return True


def check_soft_bf16_k16(device):
    """The assertions of check_bf16_ops_vs_fp32_kernels at K = 16, C = 64 on soft masks: bf16 storage is the exact
    rounding of the fp32 instantiation's result (y, dgb2, dres), fp32 outputs agree to 1e-5, dt to 2^-7."""
    gen = torch.Generator().manual_seed(1)
    C, K = 64, 16
    inp = make_inputs(C, K, gen, bf_valued=True)
    mask = make_mask("a", B_, K, H_, W_, gen)
    out = {}
    for use_res in (False, True):
        y32, _ = run_kernels(inp, mask, device, True, use_res)
        y16, _ = run_kernels(inp, mask, device, True, use_res, dtype=BF16)
        assert y16.dtype == BF16 and torch.equal(y16, y32.to(BF16)), ("sean fwd", use_res)
    # backward on the bf16-valued forward output
    dev = lambda x: x.to(device)
    h = lambda x: dev(x).to(BF16)
    m = dev(mask).contiguous()
    region, flag = ops.mask_compress(m)
    mean, var = ops.instnorm_stats(dev(inp["t"]))
    common = (m, region, flag, dev(inp["D"]), dev(inp["bg"]), dev(inp["bb"]), dev(inp["ag"]), dev(inp["ab"]))
    g32 = ops.sean_bwd(dev(inp["dout"]), y16.float(), dev(inp["t"]), mean, var, dev(inp["gb2"]), *common, True, True)
    g16 = ops.sean_bwd(h(inp["dout"]), y16, h(inp["t"]), mean, var, h(inp["gb2"]), *common, True, True)
    for nm, a, b in zip(GRAD_NAMES, g32, g16):
        if nm in ("dgb2", "dres"):
            assert b.dtype == BF16 and torch.equal(b, a.to(BF16)), ("sean bwd", nm)
        elif nm == "dt":      # pass B re-reads the (rounded) intermediate it stored: one extra rounding
            e = (b.float() - a).abs().max().item() / a.abs().max().item()
            assert b.dtype == BF16 and e <= 2.0 ** -7, ("sean bwd dt", e)
            out["dt"] = e
        else:
            assert b.dtype == torch.float32 and rel_max(b, a) <= 1e-5, ("sean bwd", nm, rel_max(b, a))
            out[nm] = rel_max(b, a)
    return out


def check_soft_dD_repeatable(device):
    """Two backward calls on the same soft inputs give bitwise equal dD (slabs summed in a fixed order, no atomics)."""
    gen = torch.Generator().manual_seed(3)
    inp = make_inputs(64, 16, gen)
    mask = make_mask("a", B_, 16, H_, W_, gen)
    _, g1 = run_kernels(inp, mask, device, True, True)
    _, g2 = run_kernels(inp, mask, device, True, True)
    assert torch.equal(g1[2], g2[2])
    assert g1[2].abs().max().item() > 0
    return True


def _soften(mk, key="soft"):
    return 0.7 * mk + 0.3 * synth.hash_uniform(mk.numel(), key).reshape(mk.shape).float()


def check_soft_whole_net_k16(device):
    """Soft masks with 16 regions carry the whole net (forward and all gradients against the oracle)."""
    K = 16
    cfg = O.make_cfg(which_ResBlk_depth=[0, 1], nb=4, scale=2, depth_latent_ch=32, depthRangeNum=K)
    net = DepthNet(which_ResBlk_depth=[0, 1], nb=4, scale=2, depth_latent_ch=32, depthRangeNum=K)
    synth.closed_form_fill_(net.state_dict().items())
    net = net.to(device)
    lq, _, dm, mk = synth.closed_form_batch(1, 2, 8, 12, 2, K)
    assert mk.shape[1] == K
    return _compare_with_oracle(net, cfg, lq, dm, _soften(mk), device)


def check_soft_whole_net_c32_resized(device):
    """A 32-channel DGB (scale 4: block 4 of 4) on soft masks delivered at half the LR resolution (nearest resize inside
    SEAN), K = 10."""
    case = dict(scale=4, which=[0, 1, 2, 3], L=16, nb=4)
    net, cfg = build_net(case, device)
    lq, _, _, _ = synth.closed_form_batch(0, 2, 12, 16, 4)
    _, _, dm, mk = synth.closed_form_batch(0, 2, 6, 8, 4)          # half-resolution depth inputs
    return _compare_with_oracle(net, cfg, lq, dm, _soften(mk), device)


def check_mask_pack_k16(device):
    assert ops.soft_mask_max_regions() == 16
    K = 16
    mk = synth.closed_form_batch(1, 2, 8, 12, 2, K)[3]
    pack = graph.MaskPack(_soften(mk).contiguous().to(device))
    assert pack.region is not None and pack.flag is not None
    assert int(pack.flag.item()) != 0                     # (the test reads the flag; the pack does not)
    small = pack.resized(4, 6)
    assert small.flag is not None and small.region is not None and tuple(small.shape) == (2, K, 4, 6)
    return True
