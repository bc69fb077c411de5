#!/usr/bin/env python3
"""Cost of soft depth masks on one GPU, two measurements:

  frames   frames/s of video.FrameUpscaler(use_graph=True).upscale (wall clock including the transfers, every call ends in a
           stream synchronise) with one-hot masks and with soft masks (--soft-masks WIDTH), in bench_video.py's default
           configuration (the x8 net on a 128x160 frame), fp32 and bf16.  Both upscalers live in one process; after
           --warmup frames each, --rounds rounds of --frames frames ALTERNATE between them.  Per side: frames/s of every
           round, and their min / median / max.
  kernels  the binning alone at the c2 LR size (16 x 128 x 160, K = 10): --iters calls of ops.depth_to_masks_soft and of
           ops.depth_to_masks (planes and region bytes) into preallocated outputs, alternating in blocks, device events
           around each block.  A call is two launches (min / max pass, binning); per-kernel durations come from running this
           mode under `rocprofv3 --kernel-trace --stats`.  The byte floor 4 (1 + K) B HW (+ 4 B HW for the min / max
           pass) is computed here from the shapes.

--soft-pair (frames): a third upscaler in the same alternating rounds, soft masks with the pair-gather SEAN forward
(FrameUpscaler(soft_pair=True)), with the share of the one-hot / soft gap it closes.
--out merges the result into a JSON file."""
import argparse
import json
import os
import sys
import time


def mmm(v):
    s = sorted(v)
    return dict(min=round(s[0], 3), median=round(s[len(s) // 2], 3), max=round(s[-1], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--mode", default="frames", choices=("frames", "kernels"))
    ap.add_argument("--soft-masks", type=float, default=1.0, metavar="WIDTH")
    ap.add_argument("--soft-pair", action="store_true",
                    help="frames: a third upscaler, soft masks with the pair-gather forward (soft_pair=True), in the same rounds")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch

    import dasr_amd  # noqa: F401
    from dasr_amd import networks, ops, synth
    from dasr_amd.video import FrameUpscaler
    assert torch.cuda.is_available(), "bench_soft_prep.py needs the GPU"
    dev = torch.device("cuda")
    K = 10
    result = dict(device=torch.cuda.get_device_name(0), soft_masks=a.soft_masks)

    if a.mode == "frames":
        scale, h, w = 8, 128, 160
        gen = np.random.default_rng(0)
        pool = [(gen.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8), gen.random(size=(1, 1, h, w), dtype=np.float32))
                for _ in range(8)]
        result.update(config="x8", lr_hw=[h, w], frames=a.frames, rounds=a.rounds, warmup=a.warmup, use_graph=True)
        for dtype in a.dtypes.split(","):
            opt = {"network_G": dict(networks.X8_NETWORK_G, upscale=scale), "datasets": {"train": {"depthMaskNum": K}}}
            net = networks.define_G(opt)
            synth.closed_form_fill_(net.state_dict().items())
            net = net.to(dev).set_compute_dtype(dtype)
            ups = {"onehot": FrameUpscaler(net, num_masks=K, use_graph=True),
                   "soft": FrameUpscaler(net, num_masks=K, use_graph=True, soft_masks=a.soft_masks)}
            if a.soft_pair:
                ups["soft_pair"] = FrameUpscaler(net, num_masks=K, use_graph=True, soft_masks=a.soft_masks, soft_pair=True)

            def run(up, n):
                t0 = time.perf_counter()
                for i in range(n):
                    up.upscale(*pool[i % len(pool)])
                return n / (time.perf_counter() - t0)

            for up in ups.values():
                run(up, a.warmup)
            torch.cuda.synchronize()
            fps = {k: [] for k in ups}
            for _ in range(a.rounds):
                for k, up in ups.items():
                    fps[k].append(round(run(up, a.frames), 3))
            differ = int((ups["onehot"].upscale(*pool[0]) != ups["soft"].upscale(*pool[0])).sum())
            result[dtype] = {k: dict(mmm(v), rounds_fps=v, graph_replays=ups[k].replays) for k, v in fps.items()}
            result[dtype]["soft_over_onehot_median"] = round(result[dtype]["soft"]["median"] / result[dtype]["onehot"]["median"], 4)
            result[dtype]["output_bytes_that_differ"] = differ
            if a.soft_pair:
                r = result[dtype]
                ms = {k: 1e3 / r[k]["median"] for k in ups}
                r["pair_over_soft_median"] = round(r["soft_pair"]["median"] / r["soft"]["median"], 4)
                r["gap_closed"] = round((ms["soft"] - ms["soft_pair"]) / (ms["soft"] - ms["onehot"]), 4)   # of the ms per frame
                r["pair_slowest_round_beats_soft_fastest"] = r["soft_pair"]["min"] > r["soft"]["max"]
                r["pair_output_bytes_that_differ_from_soft"] = int((ups["soft"].upscale(*pool[0]) != ups["soft_pair"].upscale(*pool[0])).sum())
    else:
        B, h, w = 16, 128, 160
        HW = h * w
        d = torch.from_numpy(np.random.default_rng(1).random(size=(B, 1, h, w), dtype=np.float32)).to(dev)
        soft_out = torch.empty((B, K, h, w), device=dev)
        hard_out = (torch.empty((B, K, h, w), device=dev), torch.empty((B, h, w), dtype=torch.uint8, device=dev))
        calls = {"soft": lambda: ops.depth_to_masks_soft(d, K, a.soft_masks, out=soft_out),
                 "soft_fixed_range": lambda: ops.depth_to_masks_soft(d, K, a.soft_masks, True, out=soft_out),
                 "onehot_planes_and_region": lambda: ops.depth_to_masks(d, K, None, out=hard_out)}
        for fn in calls.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                us[k].append(round(e0.elapsed_time(e1) * 1e3 / a.iters, 3))
        floor = 4 * (1 + K) * B * HW
        result.update(shape=[B, h, w], K=K, iters=a.iters, rounds=a.rounds,
                      us_per_call={k: dict(mmm(v), rounds_us=v) for k, v in us.items()},
                      note="us_per_call: device events around a block of back-to-back calls (launch gaps included); "
                           "soft and onehot calls are two launches (min / max pass + binning), soft_fixed_range is one",
                      byte_floor=dict(binning_bytes=floor, minmax_bytes=4 * B * HW,
                                      us_at_6p29_TBps=round((floor + 4 * B * HW) / 6.29e6, 3)))
    print(json.dumps(result), flush=True)
    if a.out:
        data = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                data = json.load(fh)
        data[a.mode] = result
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
