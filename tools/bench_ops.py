#!/usr/bin/env python3
"""Per-op timing on the GPU (HIP events on the launch stream): SEAN fwd/bwd and the hot conv shapes.
Usage: python tools/bench_ops.py [--batch 16] [--iters 10] [--soft] [--only loss]
--only loss: the harness-loss kernels at the c2 size (3 x 1024 x 1280 HR, K = 10, scale 8): the one-hot pair, the soft pair on the
same one-hot-valued masks and on truly soft ones, and the PyTorch formulation on the soft masks; five rounds each.
--soft: SEAN only; adds forward and backward through the general (soft-mask) path, on the one-hot-valued masks and on a truly
soft mask (0.7*mk + 0.3*rand: all 9*K terms of the dynamic convolution live)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dasr_amd  # noqa
from dasr_amd import ops, synth


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def bench_loss(a, dev, rounds=5):
    """One-hot and soft loss kernels and the PyTorch formulation, forward and backward, median (min .. max) of ``rounds``
    windows of ``--iters`` calls.  GB/s = the bytes the algorithm needs (forward: sr + hr and the LR planes / region bytes;
    backward: + dsr) over the time."""
    from dasr_amd import harness
    B, K, s, h, w = a.batch, 10, 8, 128, 160
    H, W = h * s, w * s
    mk = synth.seeded_batch(0, B, h, w, 1, K)[3].to(dev).contiguous()
    soft = (0.7 * mk + 0.3 * torch.rand(mk.shape, device=dev)).contiguous()
    hr = torch.rand(B, 3, H, W, device=dev)
    sr = (hr + 0.6 * torch.randn(B, 3, H, W, device=dev)).clamp(-1, 2)
    region, flag = ops.mask_compress(mk)
    assert int(flag.item()) == 0
    dsums = torch.rand(2 * K + 1, device=dev) + 0.5
    img = B * 3 * H * W * 4

    def row(name, fn, nbytes=None):
        ts = sorted(timeit(fn, a.iters) for _ in range(rounds))
        med = ts[len(ts) // 2]
        bw = "  %7.1f GB/s" % (nbytes / med / 1e3) if nbytes else ""
        print("%-44s %9.1f us (%.1f .. %.1f)%s" % (name, med, ts[0], ts[-1], bw), flush=True)
        return med

    row("loss_sums      one-hot (region bytes)", lambda: ops.loss_sums(sr, hr, region, K), 2 * img + B * h * w)
    row("loss_bwd       one-hot (region bytes)", lambda: ops.loss_bwd(sr, hr, region, dsums, K), 3 * img + B * h * w)
    for name, m in (("one-hot-valued", mk), ("truly soft", soft)):
        row("loss_sums_soft %s" % name, lambda: ops.loss_sums_soft(sr, hr, m, K), 2 * img + m.numel() * 4)
        row("loss_bwd_soft  %s" % name, lambda: ops.loss_bwd_soft(sr, hr, m, dsums, K), 3 * img + m.numel() * 4)
    loss = harness.DynamicMaskLoss(K).to(dev)
    srg = sr.clone().requires_grad_(True)

    def torch_fwd():
        return torch.nn.functional.l1_loss(srg, hr) + loss(srg, hr, soft)[2]

    def torch_fwd_bwd():
        srg.grad = None
        torch_fwd().backward()

    f = row("PyTorch formulation, soft masks: forward", torch_fwd)
    fb = row("PyTorch formulation, soft masks: fwd + bwd", torch_fwd_bwd)
    print("%-44s %9.1f us" % ("PyTorch formulation, soft masks: backward", fb - f))


def bench_pair(a, dev, t, gb2, D, bg, bb, ag, ab, resid, mk, region, rounds=3):
    """The pair-gather forward (dasr_sean_fwd_pair) against the general forward on the same producer-made soft masks (random
    depth maps, width 1.0: nearly every pixel has two planes) and against the gather forward on the one-hot masks, in one
    process: ``rounds`` alternating rounds of ``--iters`` calls each, fp32 and bf16, with and without the residual.  Prints
    min / median / max per arm and one JSON line."""
    import json
    B, H, W, C = t.shape
    K = D.shape[3]
    depth = torch.rand(B, 1, H, W, device=dev)
    planes, pk, ps = ops.depth_to_masks_soft(depth, K, 1.0, False, pair=True)
    two = float((ps != 0).float().mean())
    result = {"shape": [B, H, W, C, K], "width": 1.0, "pixels_with_two_planes": round(two, 4), "iters": a.iters, "arms": {}}
    for dname, cast in (("fp32", lambda x: x), ("bf16", ops.cast_to_bf16)):
        tt, gg, rr = cast(t), cast(gb2), cast(resid)
        mean, var = ops.instnorm_stats(tt)
        for rname, r in (("", None), ("+res", rr)):
            arms = (("pair", lambda: ops.sean_fwd_pair(tt, mean, var, gg, pk, ps, D, bg, bb, ag, ab, r, True)),
                    ("general", lambda: ops.sean_fwd(tt, mean, var, gg, planes, None, None, D, bg, bb, ag, ab, r, True)),
                    ("gather (one-hot masks)", lambda: ops.sean_fwd(tt, mean, var, gg, mk, region, None, D, bg, bb, ag, ab, r, True)))
            ts = {nm: [] for nm, _ in arms}
            for _ in range(rounds):                       # alternating: every round times every arm once
                for nm, fn in arms:
                    ts[nm].append(timeit(fn, a.iters))
            for nm, _ in arms:
                v = sorted(ts[nm])
                result["arms"]["%s%s %s" % (dname, rname, nm)] = {"min": round(v[0], 1), "median": round(v[len(v) // 2], 1),
                                                                  "max": round(v[-1], 1)}
                print("sean_fwd%-4s %-4s %-24s %8.1f us (%.1f .. %.1f)" % (rname, dname, nm, v[len(v) // 2], v[0], v[-1]), flush=True)
    print(json.dumps({"soft_pair_ops": result}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--amax", action="store_true", help="SEAN forward: the instantiation that also leaves max |out| behind")
    ap.add_argument("--soft", action="store_true", help="SEAN only: the general (soft-mask) path, forward and backward, "
                    "on one-hot-valued and on truly soft masks")
    a = ap.parse_args()
    if a.soft:
        a.only = "sean"
    dev = torch.device("cuda")
    B, H, W, C, K = a.batch, 128, 160, 64, 10
    torch.manual_seed(0)
    res = {}
    if not a.only or "sean" in a.only:
        t = torch.randn(B, H, W, C, device=dev)
        gb2 = torch.randn(B, H, W, 2 * C, device=dev)
        _, _, _, mk = synth.seeded_batch(0, B, H, W, 1, K)
        mk = mk.to(dev)
        region, flag = ops.mask_compress(mk)
        flag = None if int(flag.item()) == 0 else flag   # what graph.MaskPack does
        D = torch.randn(B, 2, 9, K, C, device=dev) * 0.1
        bg, bb = torch.randn(C, device=dev), torch.randn(C, device=dev)
        ag, ab = torch.full((1,), 0.7, device=dev), torch.full((1,), 0.74, device=dev)
        resid = torch.randn(B, H, W, C, device=dev)
        mean, var = ops.instnorm_stats(t)
        px = B * H * W
        us = timeit(lambda: ops.instnorm_stats(t), a.iters)
        print("instnorm_stats            %8.1f us  %7.1f GB/s" % (us, px * C * 4 / us / 1e3))
        for name, r in (("sean_fwd", None), ("sean_fwd+res", resid)):
            am = ops.amax_buffer(t) if a.amax else None      # (--amax: the instantiation that also keeps max |out|)
            us = timeit(lambda: ops.sean_fwd(t, mean, var, gb2, mk, region, flag, D, bg, bb, ag, ab, r, True, amax=am), a.iters)
            nbytes = px * (4 * (4 * C + (C if r is not None else 0)) + 4 * K)
            print("%-25s %8.1f us  %7.1f GB/s algorithmic (%.1f%% of 8 TB/s)" % (name, us, nbytes / us / 1e3,
                                                                                 nbytes / us / 1e3 / 80))
        us = timeit(lambda: ops.sean_fwd(t, mean, var, gb2, mk, None, None, D, bg, bb, ag, ab, None, True), a.iters)
        print("sean_fwd general path     %8.1f us" % us)
        out = ops.sean_fwd(t, mean, var, gb2, mk, region, flag, D, bg, bb, ag, ab, resid, True)
        dout = torch.randn_like(out)
        us = timeit(lambda: ops.sean_bwd(dout, out, t, mean, var, gb2, mk, region, flag, D, bg, bb, ag, ab, True, True),
                    a.iters)
        print("sean_bwd (fast)           %8.1f us  %7.1f GB/s (12C floats/px)" % (us, px * 12 * C * 4 / us / 1e3))
        if a.soft:
            soft = (0.7 * mk + 0.3 * torch.rand(mk.shape, device=dev)).contiguous()
            for name, m in (("one-hot-valued", mk), ("truly soft", soft)):
                for rname, r in (("", None), ("+res", resid)):
                    us = timeit(lambda: ops.sean_fwd(t, mean, var, gb2, m, None, None, D, bg, bb, ag, ab, r, True), a.iters)
                    print("sean_fwd%-4s general path, %-14s %8.1f us" % (rname, name, us))
                o = ops.sean_fwd(t, mean, var, gb2, m, None, None, D, bg, bb, ag, ab, resid, True)
                us = timeit(lambda: ops.sean_bwd(dout, o, t, mean, var, gb2, m, None, None, D, bg, bb, ag, ab, True, True),
                            a.iters)
                print("sean_bwd     general path, %-14s %8.1f us" % (name, us))
            bench_pair(a, dev, t, gb2, D, bg, bb, ag, ab, resid, mk, region)
    if not a.only or "loss" in a.only:
        bench_loss(a, dev)
    if not a.only or "dynk" in a.only:
        L = 256
        st = torch.randn(B, K, L, device=dev)
        A_w, A_b = torch.randn(K, K, 1, 1, device=dev) * 0.3, torch.randn(K, device=dev) * 0.1
        Wg, Wb = torch.randn(C, L, 3, 3, device=dev) * 0.05, torch.randn(C, L, 3, 3, device=dev) * 0.05
        stp, Dk = ops.dynk_fwd(st, A_w, A_b, Wg, Wb)
        dD = torch.randn_like(Dk)
        dst = torch.zeros_like(st)
        us = timeit(lambda: ops.dynk_fwd(st, A_w, A_b, Wg, Wb), a.iters)
        print("dynk_fwd (stp + D)        %8.1f us" % us)
        us = timeit(lambda: ops.dynk_bwd(dD, st, stp, A_w, Wg, Wb, dst), a.iters)
        print("dynk_bwd (dW, dstp, dA+dst: 3 launches) %8.1f us" % us)
    if not a.only or "c1" in a.only:
        px = B * H * W
        depth = torch.randn(B, H, W, 1, device=dev)
        wm = ops.pack_hwio(torch.randn(3, 3, 1, 128, device=dev) * 0.3)
        bm = torch.randn(128, device=dev)
        us = timeit(lambda: ops.conv2d_fwd(depth, wm, bm, act=1), a.iters)
        print("mask conv 1->128 fwd      %8.1f us  %7.1f GB/s" % (us, px * 128 * 4 / us / 1e3))
        y = ops.conv2d_fwd(depth, wm, bm, act=1)
        dy = torch.randn_like(y)
        us = timeit(lambda: ops.conv2d_wgrad_act(depth, dy, y, (3, 3, 1, 128), 1), a.iters)
        print("mask conv wgrad           %8.1f us  %7.1f GB/s" % (us, px * 128 * 4 * 2 / us / 1e3))
        del y, dy
    if not a.only or "conv" in a.only:
        shapes = [(128, 160, 64, 64), (128, 160, 128, 128), (128, 160, 32, 64), (128, 160, 64, 256),
                  (256, 320, 64, 32), (256, 320, 32, 32), (256, 320, 32, 128), (512, 640, 32, 32), (512, 640, 32, 128)]
        for (h, w, ci, co) in shapes:
            x = torch.randn(B, h, w, ci, device=dev)
            wt = ops.pack_hwio(torch.randn(3, 3, ci, co, device=dev) * 0.05)
            bias = torch.randn(co, device=dev)
            y = ops.conv2d_fwd(x, wt, bias)
            fl = 2.0 * 9 * ci * co * B * h * w
            us = timeit(lambda: ops.conv2d_fwd(x, wt, bias), a.iters)
            us_d = timeit(lambda: ops.conv2d_dgrad(y, wt, x.shape), a.iters)
            us_w = timeit(lambda: ops.conv2d_wgrad(x, y, tuple(wt.shape[1:])), a.iters)
            print("conv3x3 %3dx%3d %3d->%3d  fwd %8.1f us %6.1f TF | dgrad %8.1f us %6.1f TF | wgrad(+bias) %8.1f us %6.1f TF"
                  % (h, w, ci, co, us, fl / us / 1e6, us_d, fl / us_d / 1e6, us_w, fl / us_w / 1e6))
            del x, y
        x = torch.randn(B, 1024, 1280, 32, device=dev)
        wt = ops.pack_hwio(torch.randn(9, 9, 32, 3, device=dev) * 0.02)
        bias = torch.randn(3, device=dev)
        y = ops.conv2d_fwd(x, wt, bias, pad=4)
        fl = 2.0 * 81 * 32 * 3 * B * 1024 * 1280
        us = timeit(lambda: ops.conv2d_fwd(x, wt, bias, pad=4), a.iters)
        us_d = timeit(lambda: ops.conv2d_dgrad(y, wt, x.shape, pad=4), a.iters)
        us_w = timeit(lambda: ops.conv2d_wgrad(x, y, tuple(wt.shape[1:]), pad=4), a.iters)
        print("conv9x9 1024x1280 32->3   fwd %8.1f us %6.1f TF | dgrad %8.1f us %6.1f TF | wgrad(+bias) %8.1f us %6.1f TF"
              % (us, fl / us / 1e6, us_d, fl / us_d / 1e6, us_w, fl / us_w / 1e6))


if __name__ == "__main__":
    main()
