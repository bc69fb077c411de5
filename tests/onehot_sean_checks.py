"""The one-hot ("gather") SEAN kernels of csrc/sean.hip at op level against float64: k_sean_fwd_onehot, k_sean_fwd_onehot_w8,
k_sean_bwd_a_onehot<float | bf16_t>, k_sean_bwd_b, k_sean_bwd_b_rows (and, for C % 4 != 0, the scalar kernels with region
bytes given).  Each check takes the device ("cpu": the kernel emulator, "cuda": the MI355X); tests/test_onehot_sean.py runs
every one of them on both.

The mask planes are built from region integers (0 .. K-1, K = "no plane claims the pixel"); the float64 reference reads the
planes, the kernels read the bytes ops.mask_compress makes of them, which are checked against the integers."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from dasr_amd import ops, prep, synth
from tests.parity_checks import _compare_with_oracle, build_net, rel_max
from tests.soft_mask_checks import GRAD_NAMES, make_inputs, reference_f64, run_kernels

BF16 = torch.bfloat16
# B = 2, H = 9, W = 33: one row past an 8-row forward tile, one column past a 32-column tile
B_, H_, W_ = 2, 9, 33
MASK_KINDS = ("blob", "hashed", "hole", "allnone", "uniform")
ALL4 = tuple(itertools.product((False, True), (False, True)))       # (relu, residual)
BOTH = ((True, True), (False, False))
# (C, K, (B, H, W), mask kinds, (relu, residual) combinations): what each reaches is in check_onehot_op_vs_float64
OP_CASES = (
    (64, 10, (B_, H_, W_), MASK_KINDS, ALL4),
    (64, 16, (B_, H_, W_), ("hashed", "hole"), BOTH),
    (64, 1, (B_, H_, W_), ("hashed", "allnone"), BOTH),
    (32, 16, (B_, H_, W_), ("hashed", "hole"), BOTH),
    (96, 10, (B_, H_, W_), ("hashed", "hole"), BOTH),
    (48, 10, (B_, H_, W_), ("hashed",), ((True, True),)),
    (128, 7, (1, 5, 40), ("hashed", "hole"), BOTH),
    (6, 3, (B_, H_, W_), ("hashed", "hole"), BOTH),
    (64, 10, (3, 2, 3), ("hashed",), ((True, True),)),
    (64, 10, (1, 17, 70), ("hashed", "hole"), ((True, True),)),
)


def atomic_grads(C):
    """Gradients summed over workgroups with float atomics (dt through the per-(b, c) sums): bitwise only on the emulator.
    The MFMA kernels (C % 4 == 0) write dD as per-workgroup slabs summed in a fixed order; the scalar k_sean_bwd_a
    (C % 4 != 0) adds it up with LDS and global float atomics like the per-channel sums."""
    return ("dt", "dbg", "dbb", "dag", "dab") + (("dD",) if C % 4 else ())


def regions_of(planes):
    """[B, K, H, W] one-hot-or-zero planes -> region integers [B, H, W] (K where no plane is 1)."""
    K = planes.shape[1]
    return torch.where(planes.sum(1) > 0, planes.argmax(1), torch.full_like(planes.argmax(1), K))


def planes_of(r, K):
    return F.one_hot(r, K + 1)[..., :K].permute(0, 3, 1, 2).float().contiguous()


def make_regions(kind, B, K, H, W):
    """Region integers [B, H, W] in 0 .. K (RNG-free).
    blob: the contiguous depth regions of synth.closed_form_batch; hashed: an independent region per pixel, ~10 % unclaimed
    (nearly every 3x3 neighbourhood mixed); hole: blob with rows 2:8, columns 5:20 unclaimed in every sample; allnone: blob
    with sample 1 entirely unclaimed; uniform: region K-1 everywhere in sample 0, region 0 in sample 1."""
    if kind == "hashed":
        n = B * H * W
        r = (synth.hash_uniform(n, "onehot.region.%d" % K) * K).long().clamp_(max=K - 1)
        r[synth.hash_uniform(n, "onehot.none.%d" % K) < 0.1] = K
        return r.reshape(B, H, W)
    if kind == "uniform":
        r = torch.full((B, H, W), K - 1, dtype=torch.long)
        r[1:] = 0
        return r
    r = regions_of(synth.closed_form_batch(1, B, H, W, 1, K)[3])
    if kind == "hole":
        r[:, 2:8, 5:20] = K
    elif kind == "allnone":
        assert B >= 2
        r[1] = K
    else:
        assert kind == "blob"
    return r


def make_mask(kind, B, K, H, W, device):
    """Planes [B, K, H, W] of a mask kind; asserts that ops.mask_compress returns exactly the region integers and flag 0."""
    r = make_regions(kind, B, K, H, W)
    planes = planes_of(r, K)
    assert planes.shape == (B, K, H, W) and bool(((planes == 0) | (planes == 1)).all()) and planes.sum(1).max() <= 1
    region, flag = ops.mask_compress(planes.to(device))
    assert int(flag.item()) == 0 and torch.equal(region.cpu().long(), r), ("mask_compress", kind, K)
    return planes


def fwd_plan(B, H, W, C, has_res):
    """The tile split of sean_fwd_impl / k_sean_fwd_onehot restated: B * ceil(W/32) * ceil(H/8) tiles dealt over at most
    768 / slices workgroups (512 / slices with a residual: two resident workgroups per CU), slices = ceil(C/64); the first
    `rem` workgroups take base + 1 consecutive tiles, the others base.  Returns (tiles_per_sample, [(first, last), ...])."""
    tiles_per_sample = -(-W // 32) * -(-H // 8)
    tiles = B * tiles_per_sample
    slices = -(-C // 64)
    nwg = max(1, (512 if has_res else 768) // slices)
    nwg = min(nwg, tiles)
    base, rem = tiles // nwg, tiles % nwg
    chunks = []
    for wg in range(nwg):
        first = wg * base + min(wg, rem)
        chunks.append((first, min(first + base + (1 if wg < rem else 0), tiles)))
    assert chunks[0][0] == 0 and chunks[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    return tiles_per_sample, chunks


def crossing_workgroups(B, H, W, C, has_res):
    """Workgroups of the forward whose chunk holds tiles of two samples."""
    tps, chunks = fwd_plan(B, H, W, C, has_res)
    return [wg for wg, (first, last) in enumerate(chunks) if last > first and first // tps != (last - 1) // tps]


def check_onehot_op_vs_float64(device):
    """Output and all eight gradients of the one-hot kernels against float64 (reference_f64 of soft_mask_checks), gated at the
    project's op-level bound rel_max <= 2e-4 (check_sean_golden, check_soft_op_vs_float64).  OP_CASES:
      C = 64, K = 10  the production shape, every mask kind, relu x residual in all four combinations
      C = 64, K = 16  SEAN_MAXK: byte 16 matches no row of the 16-row one-hot matrix operand
      C = 64, K = 1   a single region
      C = 32, K = 16  half of the 64-channel slice dead
      C = 96, K = 10  second slice half dead; 256 % (C/4) != 0: k_sean_bwd_b instead of k_sean_bwd_b_rows
      C = 48, K = 10  k_sean_bwd_b with one slice
      C = 128, K = 7  two full slices, fewer rows (5) than a tile
      C = 6, K = 3    C % 4 != 0: the scalar kernels with region bytes given
      B = 3, 2 x 3    an image smaller than one tile and than its halo
      17 x 70         three tile rows and columns, ragged both ways
    Every case runs in two dispatch modes: (region, flag) - the flag is decided on the device - and (region, None), the
    gather kernel alone.  The two give bitwise equal out, dgb2, dD and dres; the gradients accumulated with float atomics
    are bitwise equal on the emulator and within 1e-5 on the GPU (the rule of check_soft_dispatch).  At C = 6 both modes run
    the scalar backward, which accumulates dD with float atomics as well (two runs of it differ on the MI355X): there dD is
    held to the same 1e-5 on the GPU and stays bitwise on the emulator.
    Unclaimed pixels inside the image (hole, allnone, ~10 % of hashed) get the bias alone as gamma1 / beta1."""
    worst = {}
    for ci, (C, K, (B, H, W), kinds, combos) in enumerate(OP_CASES):
        inp = make_inputs(C, K, torch.Generator().manual_seed(300 + ci), B, H, W)
        for kind in kinds:
            mask = make_mask(kind, B, K, H, W, device)
            for relu, use_res in combos:
                ref, gref = reference_f64(inp, mask, relu, use_res)
                runs = {}
                for mode in ("compress", "region_only"):
                    y, g = run_kernels(inp, mask, device, relu, use_res, mode)
                    runs[mode] = (y, g)
                    errs = {"out": rel_max(y, ref)}
                    for nm, a, r in zip(GRAD_NAMES, g, gref):
                        errs[nm] = rel_max(a, r)
                    print("onehot op C=%d K=%d %dx%dx%d mask=%s relu=%d res=%d %s: %s" %
                          (C, K, B, H, W, kind, relu, use_res, mode, " ".join("%s=%.2e" % kv for kv in errs.items())))
                    assert max(errs.values()) <= 2e-4, (C, K, (B, H, W), kind, relu, use_res, mode, errs)
                    for nm, e in errs.items():
                        worst[nm] = max(worst.get(nm, 0.0), e)
                (ya, ga), (yb, gb) = runs["compress"], runs["region_only"]
                assert torch.equal(ya, yb), ("dispatch fwd", C, K, kind, relu, use_res)
                for nm, a, b in zip(GRAD_NAMES, ga, gb):
                    if nm in atomic_grads(C) and device != "cpu":
                        e = rel_max(a, b)
                        assert e <= 1e-5, ("dispatch bwd", nm, C, K, kind, relu, use_res, e)
                        worst["modes:" + nm] = max(worst.get("modes:" + nm, 0.0), e)
                    else:
                        assert torch.equal(a, b), ("dispatch bwd", nm, C, K, kind, relu, use_res)
    return worst


def _fwd_bf16_both_forms(inp, mask, device, relu, use_res):
    y8 = run_kernels(inp, mask, device, relu, use_res, dtype=BF16)[0]          # eight channels per lane (C % 8 == 0)
    ops.set_conv_bf16_impl(2048)                                                # four channels per lane
    try:
        y4 = run_kernels(inp, mask, device, relu, use_res, dtype=BF16)[0]
    finally:
        ops.set_conv_bf16_impl(0)
    return y8, y4


def check_onehot_bf16(device):
    """The identities of check_bf16_ops_vs_fp32_kernels on bf16-valued inputs with unclaimed pixels and ragged channel
    slices: the bf16 forward (eight and four channels per lane) is the exact rounding of the fp32 instantiation's output;
    in the backward dgb2 and dres are exact roundings, dt and dD (G rounded to bf16 once for the matrix cores) are within
    2^-7, the other fp32 outputs within 1e-5."""
    out = {}
    cases = ((64, 10, "hashed"), (64, 10, "hole"), (64, 10, "allnone"), (32, 16, "hole"), (96, 10, "hashed"))
    dev = lambda x: x.to(device)
    h = lambda x: dev(x).to(BF16)
    for ci, (C, K, kind) in enumerate(cases):
        inp = make_inputs(C, K, torch.Generator().manual_seed(400 + ci), bf_valued=True)
        mask = make_mask(kind, B_, K, H_, W_, device)
        for use_res in (False, True):
            y32 = run_kernels(inp, mask, device, True, use_res)[0]
            y8, y4 = _fwd_bf16_both_forms(inp, mask, device, True, use_res)
            assert y8.dtype == BF16 and torch.equal(y8, y32.to(BF16)), ("sean fwd, 8 channels per lane", C, K, kind, use_res)
            assert y4.dtype == BF16 and torch.equal(y4, y32.to(BF16)), ("sean fwd, 4 channels per lane", C, K, kind, use_res)
        # backward on the bf16-valued forward output (with residual)
        m = dev(mask).contiguous()
        region, flag = ops.mask_compress(m)
        mean, var = ops.instnorm_stats(dev(inp["t"]))
        common = (m, region, flag, dev(inp["D"]), dev(inp["bg"]), dev(inp["bb"]), dev(inp["ag"]), dev(inp["ab"]))
        g32 = ops.sean_bwd(dev(inp["dout"]), y8.float(), dev(inp["t"]), mean, var, dev(inp["gb2"]), *common, True, True)
        g16 = ops.sean_bwd(h(inp["dout"]), y8, h(inp["t"]), mean, var, h(inp["gb2"]), *common, True, True)
        errs = {}
        for nm, a, b in zip(GRAD_NAMES, g32, g16):
            if nm in ("dgb2", "dres"):
                assert b.dtype == BF16 and torch.equal(b, a.to(BF16)), ("sean bwd", nm, C, K, kind)
            elif nm in ("dt", "dD"):
                e = errs[nm] = rel_max(b.float(), a)
                assert b.dtype == (BF16 if nm == "dt" else torch.float32) and e <= 2.0 ** -7, ("sean bwd", nm, C, K, kind, e)
            else:
                e = errs[nm] = rel_max(b, a)
                assert b.dtype == torch.float32 and e <= 1e-5, ("sean bwd", nm, C, K, kind, e)
        print("onehot bf16 C=%d K=%d mask=%s: %s" % (C, K, kind, " ".join("%s=%.2e" % kv for kv in errs.items())))
        out[(C, K, kind)] = errs
    return out


# 57 x 3 = 171 tiles per sample (one ragged tile row, one ragged tile column), 855 tiles: more than the 768 (512 with a
# residual) workgroups of the forward, and 171 is odd, so a workgroup that takes two consecutive tiles straddles samples.
# (tiles > 768 is needed for any workgroup to hold two tiles at C = 64; 855 is the smallest count found with B <= 5.)
CROSS_SHAPE = dict(B=5, H=449, W=65, C=64, K=4)


def check_onehot_fwd_crosses_samples(device):
    """Forward workgroups whose chunk of consecutive tiles crosses a sample boundary (D, mean and scale restaged, the next
    tile's first group prefetched from the next sample): fp32 forward with and without residual against float64 at 2e-4,
    and the bf16 forward in both forms equal to the rounding of the fp32 output."""
    B, H, W, C, K = (CROSS_SHAPE[k] for k in "BHWCK")
    crossing = {res: crossing_workgroups(B, H, W, C, res) for res in (False, True)}
    # by hand: without residual base = 1, rem = 87: workgroup 85 takes tiles 170 (sample 0) and 171 (sample 1);
    # with residual base = 1, rem = 343: workgroups 85 and 256 (tiles 512, 513 = samples 2, 3)
    assert 85 in crossing[False] and 85 in crossing[True] and 256 in crossing[True], crossing
    inp = make_inputs(C, K, torch.Generator().manual_seed(500), B, H, W, bf_valued=True)
    mask = make_mask("hashed", B, K, H, W, device)
    out = {}
    for use_res in (False, True):
        ref = reference_f64(inp, mask, True, use_res)[0]
        m = mask.to(device)
        region, _ = ops.mask_compress(m)
        t, gb2, res = (inp[k].to(device) for k in ("t", "gb2", "res"))
        mean, var = ops.instnorm_stats(t)
        common = (m, region, None) + tuple(inp[k].to(device) for k in ("D", "bg", "bb", "ag", "ab"))
        y32 = ops.sean_fwd(t, mean, var, gb2, *common, res if use_res else None, True)
        e = rel_max(y32, ref)
        print("onehot crossing %dx%dx%d C=%d K=%d res=%d: out=%.2e (%d workgroups cross)" %
              (B, H, W, C, K, use_res, e, len(crossing[use_res])))
        assert e <= 2e-4, (use_res, e)
        a16 = (t.to(BF16), mean, var, gb2.to(BF16)) + common + (res.to(BF16) if use_res else None, True)
        y8 = ops.sean_fwd(*a16)
        ops.set_conv_bf16_impl(2048)
        try:
            y4 = ops.sean_fwd(*a16)
        finally:
            ops.set_conv_bf16_impl(0)
        want = y32.to(BF16)
        assert torch.equal(y8, want), ("bf16 fwd, 8 channels per lane", use_res)
        assert torch.equal(y4, want), ("bf16 fwd, 4 channels per lane", use_res)
        out["res%d" % use_res] = e
    return out


WHOLE_NET_CASE = dict(scale=2, which=[0, 1, 2, 3], L=16, nb=4)


def check_onehot_whole_net_unclaimed(device):
    """The whole net (forward and every gradient against the oracle, default gates of _compare_with_oracle) on one-hot
    masks with unclaimed pixels inside the image: (1) the closed-form masks with a 6 x 9 patch of sample 0 and all of sample
    1 zeroed; (2) masks from prep.depth_to_masks in fixed-range mode, sample 0 a constant depth map outside every bin and
    sample 1 with depth in [-0.2, 1.2) (the real input path: region bytes attached by the preparation kernel)."""
    out = {}
    lq, _, dm, mk = synth.closed_form_batch(2, 2, 10, 14, 2)
    mk = mk.clone()
    mk[0, :, 2:8, 3:12] = 0
    mk[1] = 0
    net, cfg = build_net(WHOLE_NET_CASE, device)
    out["zeroed"] = _compare_with_oracle(net, cfg, lq, dm, mk, device)
    depth = torch.empty(2, 1, 10, 14)
    depth[0] = 3.25                                                            # constant, outside [0, 1): every bin empty
    depth[1] = (synth.hash_uniform(10 * 14, "onehot.depth") * 1.4 - 0.2).reshape(1, 10, 14).float()
    masks = prep.depth_to_masks(depth.to(device), 10, fixed_range=True)
    planes = masks.cpu()
    want = torch.stack([synth.depth_to_masks(depth[b], 10, True) for b in range(2)])
    assert torch.equal(planes, want)
    r = regions_of(planes)
    assert bool((r[0] == 10).all()) and bool((r[1] == 10).any()) and bool((r[1] < 10).any())
    assert torch.equal(masks._dasr_region.cpu().long(), r)
    net, cfg = build_net(WHOLE_NET_CASE, device)
    # _compare_with_oracle gives `mk` to the CPU oracle and `mk.to(device)` to the net: the oracle gets the planes on the
    # host, the net the prepared tensor itself (its region bytes are attached to that very tensor)
    planes.to = lambda _device: masks
    out["prepared"] = _compare_with_oracle(net, cfg, lq, depth, planes, device)
    return out


def check_scalar_region_limit(device):
    """C % 4 != 0 runs the scalar kernels, whose backward keeps two [2][9][K][64] tables in LDS: K = 14 is the largest
    region count they take (and matches float64); K = 15 is refused by forward and backward before anything is launched
    (DASR_E_UNSUPPORTED, raised by the wrapper)."""
    C, B, H, W = 6, B_, H_, W_
    inp = make_inputs(C, 14, torch.Generator().manual_seed(600), B, H, W)
    mask = make_mask("hashed", B, 14, H, W, device)
    y, g = run_kernels(inp, mask, device, True, True)
    ref, gref = reference_f64(inp, mask, True, True)
    errs = {"out": rel_max(y, ref)}
    for nm, a, r in zip(GRAD_NAMES, g, gref):
        errs[nm] = rel_max(a, r)
    print("onehot scalar C=6 K=14: %s" % " ".join("%s=%.2e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 2e-4, errs
    inp = make_inputs(C, 15, torch.Generator().manual_seed(601), B, H, W)
    mask = make_mask("hashed", B, 15, H, W, device)
    dev = lambda x: x.to(device)
    m = dev(mask)
    region, flag = ops.mask_compress(m)
    t, gb2 = dev(inp["t"]), dev(inp["gb2"])
    mean, var = ops.instnorm_stats(t)
    common = (m, region, flag, dev(inp["D"]), dev(inp["bg"]), dev(inp["bb"]), dev(inp["ag"]), dev(inp["ab"]))
    with pytest.raises(RuntimeError, match="dasr_sean_fwd failed.*code"):
        ops.sean_fwd(t, mean, var, gb2, *common, None, True)
    with pytest.raises(RuntimeError, match="dasr_sean_bwd failed.*code"):
        ops.sean_bwd(dev(inp["dout"]), t, t, mean, var, gb2, *common, True, True)      # (`out`: any tensor of t's shape)
    return errs


def check_dynk_odd_latent(device):
    """dasr_dynk_fwd / dasr_dynk_bwd with an odd latent width (L = 5, K = 3, C = 4, B = 1: the last K step of the
    32x32x2 MFMA has only its first half) against float64 einsums."""
    B, K, L, C = 1, 3, 5, 4
    gen = torch.Generator().manual_seed(700)
    rn = lambda *s: torch.randn(*s, generator=gen)
    st, A_w, A_b = rn(B, K, L), rn(K, K, 1, 1) * 0.3, rn(K) * 0.1
    Wg, Wb = rn(C, L, 3, 3), rn(C, L, 3, 3)
    dD = rn(B, 2, 9, K, C)
    d = [x.double().clone().requires_grad_(True) for x in (st, A_w, A_b, Wg, Wb)]
    stp_ref = d[2].reshape(1, K, 1) + torch.einsum("kj,bjl->bkl", d[1].reshape(K, K), d[0])
    W2 = torch.stack((d[3], d[4])).reshape(2, C, L, 9)
    D_ref = torch.einsum("sclt,bkl->bstkc", W2, stp_ref)
    D_ref.backward(dD.double())
    dev = lambda x: x.to(device)
    stp, D = ops.dynk_fwd(dev(st), dev(A_w), dev(A_b), dev(Wg), dev(Wb))
    dst = torch.zeros_like(dev(st))
    dWg, dWb, dA_w, dA_b = ops.dynk_bwd(dev(dD), dev(st), stp, dev(A_w), dev(Wg), dev(Wb), dst)
    errs = {"stp": rel_max(stp, stp_ref.detach()), "D": rel_max(D, D_ref.detach()), "dst": rel_max(dst, d[0].grad),
            "dA_w": rel_max(dA_w, d[1].grad), "dA_b": rel_max(dA_b, d[2].grad), "dWg": rel_max(dWg, d[3].grad),
            "dWb": rel_max(dWb, d[4].grad)}
    print("dynk L=5: %s" % " ".join("%s=%.2e" % kv for kv in errs.items()))
    # fp32 sums of at most 18 * C = 72 terms against float64: a few ulp
    assert max(errs.values()) <= 1e-5, errs
    return errs
