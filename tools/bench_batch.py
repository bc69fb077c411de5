#!/usr/bin/env python3
"""Time of making one training batch from uint8 HR frames on one GPU (csrc/batch.hip, data.BatchMaker):

  kernels   dasr_batch_lr_u8, dasr_batch_gt_u8, dasr_batch_plane_f32 (the depth map), each alone: device events around
            --launches back-to-back launches, per-launch time = the span / launches, median over --rounds; next to it the
            bytes the kernel has to move (HR bytes read once, outputs written once; computed from the shapes below) and
            the time those bytes take at the 8 TB/s HBM peak
  make      BatchMaker.make from host numpy frames (pinned staging, upload, the three kernels, the masks), wall clock
            around a call that ends in a device synchronise, median over --rounds * --calls
  host      the path this replaces, the same way: torch CPU `/ 255`, the resize as two dense matrix products built from
            the same tap tables (a vectorised stand-in for imresize_np, which loops in Python over rows and columns),
            augment, BGR -> RGB, HWC -> CHW, fp32 upload of LR / GT / depth, masks binned on the device

for --config c2 (16 frames 1024 x 1280 -> 128 x 160, x8: the benchmark's batch) or x2 (4 frames 1080 x 1920 -> 540 x 960, x2).
The arms alternate within a round.  Not a pass / fail gate.  One entry per configuration is merged into --out:

  timeout -k 10 300 python tools/bench_batch.py --config c2 --out profiles/batch_prep.json && \\
  timeout -k 10 300 python tools/bench_batch.py --config x2 --out profiles/batch_prep.json"""
import argparse
import json
import os
import sys
import time

CONFIGS = {"c2": dict(scale=8, B=16, H=1024, W=1280), "x2": dict(scale=2, B=4, H=1080, W=1920)}
HBM_PEAK = 8.0e12          # bytes / s


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch

    import dasr_amd  # noqa: F401
    from dasr_amd import data, ops, prep
    assert torch.cuda.is_available(), "bench_batch.py needs the GPU"
    dev = torch.device("cuda")
    c = CONFIGS[a.config]
    s, B, H, W = c["scale"], c["B"], c["H"], c["W"]
    h, w, K = H // s, W // s, 10
    gen = np.random.default_rng(0)
    pool = [(gen.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8), gen.random(size=(B, 1, h, w), dtype=np.float32),
             gen.integers(0, 4, size=(B,)).astype(np.uint8)) for _ in range(2)]

    # ---- kernels alone ---------------------------------------------------------------------------------------------------
    frames = torch.from_numpy(pool[0][0]).to(dev)
    depth = torch.from_numpy(pool[0][1]).to(dev)
    flags = torch.from_numpy(pool[0][2]).to(dev)
    tables = tuple(torch.from_numpy(np.array(t)).to(dev) for t in
                   (data.resize_tables(H, s)[0], data.resize_tables(H, s)[1], data.resize_tables(W, s)[0], data.resize_tables(W, s)[1]))
    lq = torch.empty((B, 3, h, w), device=dev)
    gt = torch.empty((B, 3, H, W), device=dev)
    dm = torch.empty((B, 1, h, w), device=dev)
    hr_bytes = B * H * W * 3
    kernels = {
        "dasr_batch_lr_u8": (lambda: ops.batch_lr_u8(frames, s, tables, flags=flags, out=lq), hr_bytes + lq.numel() * 4),
        "dasr_batch_gt_u8": (lambda: ops.batch_gt_u8(frames, s, flags=flags, out=gt), hr_bytes + gt.numel() * 4),
        "dasr_batch_plane_f32": (lambda: ops.batch_plane(depth, flags=flags, out=dm), 2 * dm.numel() * 4),
    }
    ktimes = {k: [] for k in kernels}
    for k, (fn, _) in kernels.items():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (fn, _) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ktimes[k].append(e0.elapsed_time(e1) / a.launches)
    kout = {}
    for k, (_, nbytes) in kernels.items():
        ms = median(ktimes[k])
        floor_ms = nbytes / HBM_PEAK * 1e3
        kout[k] = dict(median_ms=round(ms, 4), rounds_ms=[round(v, 4) for v in ktimes[k]], bytes=nbytes,
                       ms_at_8TBps=round(floor_ms, 4), achieved_TBps=round(nbytes / (ms * 1e-3) / 1e12, 3),
                       share_of_hbm_peak=round(floor_ms / ms, 3))

    # ---- make() against the host path ------------------------------------------------------------------------------------
    mk = data.BatchMaker(s, K, device=dev)

    def arm_make(f, d, fl):
        out = mk.make(f, d, fl)
        torch.cuda.synchronize()
        return out

    def dense(n):
        wt, first, _, _ = data.resize_tables(n, s)
        m = np.zeros((n // s, n), dtype=np.float32)
        for k in range(4 * s):
            i = first + k
            i = np.where(i < 0, -i - 1, i)
            i = np.where(i >= n, 2 * n - 1 - i, i)
            np.add.at(m, (np.arange(n // s), i), wt[:, k])
        return torch.from_numpy(m)

    mh, mw = dense(H), dense(W)

    def arm_host(f, d, fl):
        img = torch.from_numpy(f).float() / 255.                                   # read_img, [B,H,W,3] BGR
        chw = img.permute(0, 3, 1, 2).flip(1)                                      # RGB, CHW
        lr = torch.matmul(torch.matmul(mh, chw), mw.t())                           # H pass, then W pass
        outs = []
        for t in (lr, chw, torch.from_numpy(d)):
            parts = []
            for b in range(B):
                x = t[b]
                if fl[b] & 1:
                    x = x.flip(2)
                if fl[b] & 2:
                    x = x.flip(1)
                parts.append(x)
            outs.append(torch.stack(parts).contiguous().to(dev))
        masks = prep.depth_to_masks(outs[2], K)
        torch.cuda.synchronize()
        return outs[0], outs[1], outs[2], masks

    arms = {"make": arm_make, "host": arm_host}
    got = {k: [t.clone() for t in fn(*pool[0])] for k, fn in arms.items()}
    agree = dict(gt_equal=bool(torch.equal(got["make"][1], got["host"][1])),
                 depth_equal=bool(torch.equal(got["make"][2], got["host"][2])),
                 masks_equal=bool(torch.equal(got["make"][3], got["host"][3])),
                 lr_max_abs_diff=float((got["make"][0] - got["host"][0]).abs().max()))
    for fn in arms.values():
        for i in range(a.warmup):
            fn(*pool[i % 2])
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            for i in range(a.calls):
                t0 = time.perf_counter()
                fn(*pool[i % 2])
                times[k].append((time.perf_counter() - t0) * 1e3)
    entry = dict(config=a.config, scale=s, batch=B, hr_hw=[H, W], lr_hw=[h, w], launches=a.launches, rounds=a.rounds,
                 calls=a.calls, warmup=a.warmup, hr_bytes=hr_bytes, kernels=kout, outputs_vs_host=agree,
                 make_ms=dict(median=round(median(times["make"]), 3), min=round(min(times["make"]), 3), n=len(times["make"])),
                 host_ms=dict(median=round(median(times["host"]), 3), min=round(min(times["host"]), 3), n=len(times["host"])),
                 host_threads=torch.get_num_threads(), device=torch.cuda.get_device_name(0))
    print(json.dumps(entry), flush=True)
    if a.out:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                out = json.load(fh)
        out[a.config] = entry
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
