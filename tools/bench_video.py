#!/usr/bin/env python3
"""Per-frame latency of video inference on one GPU, wall clock including the transfers, four ways:

  a  the path validate.test offers: host img2tensor, fp32 upload, validate.test, fp32 download, tensor2img
  b  video.FrameUpscaler(use_graph=False).upscale
  c  video.FrameUpscaler(use_graph=True).upscale          (captured graph, replayed)
  d  video.FrameUpscaler(use_graph=True).upscale_iter     (two-slot pipeline; per frame = time between two results)

for one configuration (--config x8: the x8 net on a 128x160 frame; x2: the x2 net on a 540x960 frame; --dtype fp32|bf16;
--soft-masks WIDTH: soft depth masks of that blend width in every arm, default one-hot; its entry's key ends in _softWIDTH;
--soft-pair with it: the pair-gather SEAN forward in arms b, c, d (arm a, the reference's call, keeps the general path; the
byte-equality with b then holds to one unit); key ..._pair).
tools/bench_soft_prep.py compares the two mask kinds in one process, alternating.
--self-ensemble: arms b, c and d run a second time with FrameUpscaler(self_ensemble=True) (validate.test_x8 per frame: eight
flip / transpose members, two forwards of batch 4) as arms b_x8ens, c_x8ens, d_x8ens, alternating with the plain arms in the
same process, and the entry - plain arms, ensemble arms and the ratio of their medians - goes under a key that ends in _x8ens.
Every arm gets --warmup frames, then --rounds rounds of --frames frames; the arms alternate within a round.  Each timed
call ends in a device synchronise (a: the download; b, c: the stream synchronise of upscale; d: the download event of the
frame handed out).  Median and p95 over all timed frames of an arm, and the median of each round, go into one entry of
--out (a JSON file, one entry per configuration, merged with what is there).  One process per configuration, no profiler.
Each configuration is one GPU step and runs under its own time limit; the table of DESIGN.md section 5 is

  timeout -k 10 240 python tools/bench_video.py --config x8 --dtype fp32 --out profiles/video_latency.json && \
  timeout -k 10 240 python tools/bench_video.py --config x8 --dtype bf16 --out profiles/video_latency.json && \
  timeout -k 10 240 python tools/bench_video.py --config x2 --dtype fp32 --out profiles/video_latency.json && \
  timeout -k 10 240 python tools/bench_video.py --config x2 --dtype bf16 --out profiles/video_latency.json"""
import argparse
import json
import os
import sys
import time

CONFIGS = {"x8": dict(scale=8, h=128, w=160), "x2": dict(scale=2, h=540, w=960)}


def stats(ms):
    s = sorted(ms)
    return dict(median_ms=round(s[len(s) // 2], 3), p95_ms=round(s[min(len(s) - 1, int(0.95 * len(s)))], 3), n=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--config", default="x8", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default="abcd")
    ap.add_argument("--soft-masks", type=float, default=None, metavar="WIDTH",
                    help="soft depth masks of this blend width (prep.depth_to_soft_masks) in every arm; default: one-hot")
    ap.add_argument("--soft-pair", action="store_true",
                    help="with --soft-masks: the pair-gather SEAN forward (FrameUpscaler(soft_pair=True)) in arms b, c, d")
    ap.add_argument("--self-ensemble", action="store_true",
                    help="also time arms b, c, d with FrameUpscaler(self_ensemble=True); the entry's key ends in _x8ens")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch

    import dasr_amd  # noqa: F401
    from dasr_amd import networks, prep, synth, validate
    from dasr_amd.video import FrameUpscaler
    assert torch.cuda.is_available(), "bench_video.py needs the GPU"
    dev = torch.device("cuda")
    c = CONFIGS[a.config]
    K, scale, h, w = 10, c["scale"], c["h"], c["w"]
    opt = {"network_G": dict(networks.X8_NETWORK_G, upscale=scale), "datasets": {"train": {"depthMaskNum": K}}}
    net = networks.define_G(opt)
    synth.closed_form_fill_(net.state_dict().items())
    net = net.to(dev).set_compute_dtype(a.dtype)

    gen = np.random.default_rng(0)
    pool = [(gen.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8), gen.random(size=(1, 1, h, w), dtype=np.float32))
            for _ in range(8)]

    def arm_a(f, d):
        img = f[0].astype(np.float32) / 255.                                   # img2tensor, utils/util.py:596-605
        lq = torch.from_numpy(np.ascontiguousarray(np.transpose(img[:, :, [2, 1, 0]], (2, 0, 1))))[None].to(dev)
        dd = torch.from_numpy(d).to(dev)
        mk = prep.depth_to_masks(dd, K) if soft is None else prep.depth_to_soft_masks(dd, K, width=soft)
        sr = validate.test(net, lq, dd, mk)
        return validate.tensor2img(sr[0])[None]                                # download + clamp / transpose / round on the host

    soft = a.soft_masks
    pair = dict(soft_pair=True) if a.soft_pair else {}       # (ValueError from the upscaler without --soft-masks)
    up_b = FrameUpscaler(net, num_masks=K, use_graph=False, soft_masks=soft, **pair)
    up_c = FrameUpscaler(net, num_masks=K, use_graph=True, soft_masks=soft, **pair)
    up_d = FrameUpscaler(net, num_masks=K, use_graph=True, soft_masks=soft, **pair)

    def per_call(fn):
        def run(n):
            ms = []
            for i in range(n):
                f, d = pool[i % len(pool)]
                t0 = time.perf_counter()
                fn(f, d)
                ms.append((time.perf_counter() - t0) * 1e3)
            return ms
        return run

    def pipelined(up):
        def run(n):
            # n + 2 frames in, the first two intervals (the pipeline filling) dropped: n steady-state intervals
            ms, t0 = [], time.perf_counter()
            for _ in up.upscale_iter(pool[i % len(pool)] for i in range(n + 2)):
                t1 = time.perf_counter()
                ms.append((t1 - t0) * 1e3)
                t0 = t1
            return ms[2:]
        return run

    arms = {"a": per_call(arm_a), "b": per_call(up_b.upscale), "c": per_call(up_c.upscale), "d": pipelined(up_d)}
    arms = {k: v for k, v in arms.items() if k in a.arms}
    f0, d0 = pool[0]
    ref = up_b.upscale(f0, d0)
    same = {k: bool(np.array_equal(fn(f0, d0), ref)) for k, fn in (("a", arm_a), ("c", up_c.upscale)) if k in arms}
    ens = {}
    if a.self_ensemble:
        ens = {k: FrameUpscaler(net, num_masks=K, use_graph=k != "b", soft_masks=soft, self_ensemble=True, **pair)
               for k in "bcd" if k in a.arms}
        for k, up in ens.items():
            arms[k + "_x8ens"] = pipelined(up) if k == "d" else per_call(up.upscale)
        if "b" in ens:
            ref8 = ens["b"].upscale(f0, d0)
            same["b_x8ens_differs_from_b"] = bool(not np.array_equal(ref8, ref))
            if "c" in ens:
                same["c_x8ens"] = bool(np.array_equal(ens["c"].upscale(f0, d0), ref8))       # (equal to b_x8ens)
    for run in arms.values():
        run(a.warmup)
    torch.cuda.synchronize()
    allms, rounds = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, run in arms.items():
            ms = run(a.frames)
            torch.cuda.synchronize()
            allms[k] += ms
            rounds[k].append(stats(ms)["median_ms"])
    entry = dict(config=a.config, dtype=a.dtype, soft_masks=soft, soft_pair=bool(a.soft_pair), scale=scale, lr_hw=[h, w], frames=a.frames, rounds=a.rounds,
                 warmup=a.warmup, outputs_equal_to_b=same,
                 graph_replays=dict(dict(c=up_c.replays, d=up_d.replays),
                                    **{k + "_x8ens": up.replays for k, up in ens.items() if k != "b"}),
                 arms={k: dict(stats(v), round_medians_ms=rounds[k]) for k, v in allms.items()},
                 device=torch.cuda.get_device_name(0), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    if ens:
        med = {k: v["median_ms"] for k, v in entry["arms"].items()}
        entry["self_ensemble"] = True
        entry["x8ens_over_plain"] = {k: round(med[k + "_x8ens"] / med[k], 2) for k in ens if k in med}
    print(json.dumps(entry), flush=True)
    if a.out:
        data = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                data = json.load(fh)
        data["%s_%s%s" % (a.config, a.dtype, ("" if soft is None else "_soft%g" % soft) + ("_pair" if a.soft_pair else "") +
                             ("_x8ens" if ens else ""))] = entry
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(data, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
