#!/usr/bin/env python3
"""The 32-produced-channel fp16 x 2 split dgrads of the HR tail at the x8 bench shapes (B frames; 32 -> 32 and 32 -> 128 layers at
256 x 320 and 512 x 640): the plain dgrad, dasr_conv2d_epilogue_bwd on its output (flat and PixelShuffle(2) form), and the fused
dasr_conv3x3_dgrad_act_split2 launch that replaces the pair.  HIP events, isolated launches, three alternating rounds of five;
median and min-max.  The fused results and their amax must EQUAL the two-kernel results at these sizes (asserted).
Usage: python tools/bench_split_dgrad_act.py [B]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dasr_amd  # noqa
from dasr_amd import ops


def timeit(fn, iters=5):
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
    ci, act = 32, ops.ACT_LRELU
    for (H, W) in ((256, 320), (512, 640)):
        for co in (32, 128):
            torch.manual_seed(5)
            x_act = torch.randn(B, H, W, ci, device=dev)
            ws = ops.conv3x3_split2_weights(ops.pack_hwio(torch.randn(3, 3, ci, co, device=dev) * 0.02))
            dy = torch.randn(B, H, W, co, device=dev)
            dm = ops.absmax(dy)
            dx = ops.conv3x3_dgrad_split2(dy, dm, ws, x_act.shape)
            bufs = [ops.amax_buffer(dx) for _ in range(4)]
            shp = {1: (H, W, ci), 2: (H // 2, W // 2, 4 * ci)}
            for r in (1, 2):
                two = ops.conv2d_epilogue_bwd(dx, x_act, *shp[r], act, r, amax=bufs[0])
                one = ops.conv3x3_dgrad_act_split2(dy, dm, ws, x_act, act, r, amax=bufs[1])
                assert torch.equal(one, two), "fused launch differs from dgrad + epilogue backward"
                assert ops.amax_value(bufs[0]) == ops.amax_value(bufs[1]) == two.abs().max().item(), "amax differs"
                del one, two
            cases = [("dgrad", lambda: ops.conv3x3_dgrad_split2(dy, dm, ws, x_act.shape)),
                     ("epilogue bwd flat", lambda: ops.conv2d_epilogue_bwd(dx, x_act, *shp[1], act, 1, amax=bufs[0])),
                     ("epilogue bwd ps2", lambda: ops.conv2d_epilogue_bwd(dx, x_act, *shp[2], act, 2, amax=bufs[1])),
                     ("fused flat", lambda: ops.conv3x3_dgrad_act_split2(dy, dm, ws, x_act, act, 1, amax=bufs[2])),
                     ("fused ps2", lambda: ops.conv3x3_dgrad_act_split2(dy, dm, ws, x_act, act, 2, amax=bufs[3]))]
            t = {}
            for _ in range(3):
                for k, fn in cases:
                    t.setdefault(k, []).append(timeit(fn))
            med = {k: sorted(v)[1] for k, v in t.items()}
            tag = "B=%d 3x3 %d<-%d @%dx%d" % (B, ci, co, H, W)
            for k, v in t.items():
                print("%s %-18s median %8.1f us  (min %.1f max %.1f)" % (tag, k, med[k], min(v), max(v)))
            for form, epi in (("flat", "epilogue bwd flat"), ("ps2", "epilogue bwd ps2")):
                print("%s %s: two kernels %.1f us -> fused %.1f us  (bit-equal)" % (tag, form, med["dgrad"] + med[epi], med["fused " + form]))
            del x_act, dy, dx
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
