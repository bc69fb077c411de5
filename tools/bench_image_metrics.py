#!/usr/bin/env python3
"""Cost of the test script's metrics on one GPU against the host:

  device  ops.image_metrics_u8 on --frames uint8 BGR frames of --height x --width x 3 with --crop (16 x 1024 x 1280 x 3,
          crop 8 by default) into preallocated outputs: after --warmup calls, --rounds blocks of --iters back-to-back calls,
          device events around each block.  A call is two launches (tiles, per-frame sum) and one workspace allocation from
          torch's caching allocator; launch gaps are included.
  host    the float64 numpy restatement of the reference's functions (tests/image_metrics_checks.py: ref_figures) on ONE
          frame of the same size, wall clock, --host-runs times.  It is a restatement written for exactness, not for speed
          (a full 121-tap window per moment, calculate_ssim's three identical passes): an upper bound of what a host costs.
  check   the four figures of that frame from the device against the restatement (absolute differences).

The fp64 operation count of a frame is computed here from the shapes.  --out writes the JSON."""
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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--crop", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch

    import dasr_amd  # noqa: F401
    from dasr_amd import ops, validate
    from tests import image_metrics_checks as ic
    assert torch.cuda.is_available(), "bench_image_metrics.py needs the GPU"
    dev = torch.device("cuda")
    B, H, W, crop = a.frames, a.height, a.width, a.crop
    gen = np.random.default_rng(0)
    # a smooth image plus noise as GT, SR = GT + small noise: what a test set looks like to the arithmetic (the kernel's
    # time does not depend on the values)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 127.0 + 80.0 * np.sin(0.011 * xx)[None, :, :, None] * np.cos(0.013 * yy)[None, :, :, None]
    gt = np.clip(base + gen.integers(-20, 21, size=(B, H, W, 3)), 0, 255).astype(np.uint8)
    sr = np.clip(gt.astype(np.int64) + gen.integers(-6, 7, size=gt.shape), 0, 255).astype(np.uint8)
    sr_d, gt_d = torch.from_numpy(sr).to(dev), torch.from_numpy(gt).to(dev)
    out = (torch.empty((B,), dtype=torch.int64, device=dev), torch.empty((B, 3), dtype=torch.float64, device=dev))
    for _ in range(a.warmup):
        ops.image_metrics_u8(sr_d, gt_d, crop, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ops.image_metrics_u8(sr_d, gt_d, crop, out=out)
        e1.record()
        e1.synchronize()
        ms.append(round(e0.elapsed_time(e1) / a.iters, 4))
    got = validate.image_metrics(sr_d[:1], gt_d[:1], crop)[0]

    host_s = []
    for _ in range(a.host_runs):
        t0 = time.perf_counter()
        want = ic.ref_figures(sr[0], gt[0], crop)
        host_s.append(round(time.perf_counter() - t0, 3))
    diff = {k: abs(got[k] - want[k]) for k in ic.FIGURES}
    assert all(d <= ic.GATE for d in diff.values()), diff

    Hc, Wc = H - 2 * crop, W - 2 * crop
    th, tw = -(-(Hc - 10) // ic.T_H), -(-(Wc - 10) // ic.T_W)
    # per tile and plane: (T_H + 10) x T_W row-pass outputs and T_H x T_W column-pass outputs of 5 moments x 11 taps; the
    # row pass forms three products per tap besides; four planes (B, G, R, luma)
    fma = 4 * th * tw * 55 * ((ic.T_H + 10) * ic.T_W + ic.T_H * ic.T_W)
    mul = 4 * th * tw * 33 * (ic.T_H + 10) * ic.T_W
    med = sorted(ms)[len(ms) // 2]
    result = dict(device=torch.cuda.get_device_name(0), shape=[B, H, W, 3], crop=crop, iters=a.iters, rounds=a.rounds,
                  warmup=a.warmup, device_ms_per_call=dict(mmm(ms), rounds_ms=ms),
                  device_ms_per_frame_median=round(med / B, 4),
                  fp64_per_frame=dict(fma=fma, mul=mul, tflops_at_median=round((2 * fma + mul) * B / (med * 1e-3) / 1e12, 3)),
                  input_bytes_per_frame=2 * H * W * 3,
                  host_restatement_s_per_frame=dict(mmm(host_s), runs_s=host_s),
                  host_over_device_per_frame=round(sorted(host_s)[len(host_s) // 2] / (med * 1e-3 / B), 1),
                  figures_frame0=got, abs_difference_to_restatement=diff,
                  note="one machine, one run; device: events around blocks of back-to-back calls (two launches and an "
                       "allocator call each, launch gaps included); host: the exactness-first numpy restatement of the "
                       "tests on one core-bound process, not an optimised host implementation")
    print(json.dumps(result), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
