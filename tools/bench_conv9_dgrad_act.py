#!/usr/bin/env python3
"""The backward of the HR tail at the x8 bench shape (B frames of 1024 x 1280, 9x9 32 <- 3 behind LeakyReLU + PixelShuffle(2)):
the plain fp16 x 2 split dgrad, dasr_conv2d_epilogue_bwd on its output, and the fused dasr_conv9_dgrad_act_split2 launch that
replaces both.  HIP events, isolated, median of 3 rounds of 3.  The fused result and its amax must EQUAL the two-kernel
result at this size (asserted).  A build without the fused entry point prints the first two lines only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dasr_amd  # noqa
from dasr_amd import ops


def timeit(fn, iters=3):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    dev = torch.device("cuda")
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    H, W, ci, co, act = 1024, 1280, 32, 3, ops.ACT_LRELU
    torch.manual_seed(5)
    x_act = torch.randn(B, H, W, ci, device=dev)
    wp = ops.pack_hwio(torch.randn(9, 9, ci, co, device=dev) * 0.02)
    dy = torch.randn(B, H, W, co, device=dev)
    wm, dm = ops.absmax(wp[0]), ops.absmax(dy)
    fused_op = getattr(ops, "conv9_dgrad_act_split2", None)
    dx = ops.conv9_dgrad_split2(dy, dm, wp, wm, x_act.shape)
    buf2, buf1 = ops.amax_buffer(dx), ops.amax_buffer(dx)
    two = ops.conv2d_epilogue_bwd(dx, x_act, H // 2, W // 2, 4 * ci, act, 2, amax=buf2)
    if fused_op is not None:
        one = fused_op(dy, dm, wp, wm, x_act, act, 2, amax=buf1)
        assert torch.equal(one, two), "fused launch differs from dgrad + epilogue backward"
        assert ops.amax_value(buf1) == ops.amax_value(buf2) == two.abs().max().item(), "amax differs"
        print("B=%d: fused result and amax bit-equal to dgrad + epilogue backward (max |dprev| %.6g)" % (B, ops.amax_value(buf1)))
        del one
    cases = [("fp16x2 dgrad", lambda: ops.conv9_dgrad_split2(dy, dm, wp, wm, x_act.shape, out=None)),
             ("epilogue bwd ps2", lambda: ops.conv2d_epilogue_bwd(dx, x_act, H // 2, W // 2, 4 * ci, act, 2, amax=buf2))]
    if fused_op is not None:
        cases.append(("fused dgrad+act", lambda: fused_op(dy, dm, wp, wm, x_act, act, 2, amax=buf1)))
    r = {}
    for _ in range(3):
        for k, fn in cases:
            r.setdefault(k, []).append(timeit(fn))
    for k, v in r.items():
        print("B=%d 9x9 32<-3 @%dx%d %-18s median %9.1f us  (rounds %s)" % (B, H, W, k, sorted(v)[1], " ".join("%.1f" % t for t in v)))
    if fused_op is not None:
        print("B=%d two kernels %.1f us -> fused %.1f us" % (B, sorted(r["fp16x2 dgrad"])[1] + sorted(r["epilogue bwd ps2"])[1],
                                                             sorted(r["fused dgrad+act"])[1]))


if __name__ == "__main__":
    main()
