#!/usr/bin/env python3
"""The criterion-parametrised loss kernels (dasr_loss_{sums,bwd}[_soft]_crit) on one GPU at the c2 size (16 frames of
1024 x 1280, x8, K = 10).  Writes one JSON file (default profiles/criteria_bench.json) and prints it.

Without --worker this is the driver: it starts the GPU work as a child process under a time limit of its own
(``timeout -k 10 <seconds>``) and stops if it fails.

  default    (pixel l1, region smoothl1, no second criterion) through the argument-policy kernels ("new") against the
             fixed-policy ones ("existing": dasr_loss_sums / dasr_loss_bwd and their _soft twins): what the parametrisation costs.  Region bytes and soft
             masks; forward and backward; three windows of --iters launches a side, alternating, timed with device events.
             Achieved bytes/s against the algorithmic traffic (forward: read sr, hr; backward: read sr, hr, write dsr).
  criteria   each non-default combination, forward + backward, against the PyTorch formulation (criterion_sums_torch under
             autograd) on the same device and tensors; the largest gradient difference over the largest PyTorch entry.
No ratio is asserted: the figures are for DESIGN.md section 4.16."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("l2", "smoothl1", None), ("cb", "smoothl1", None), ("l1", "l1", None), ("l1", "l2", None), ("l2", "l2", None),
          ("cb", "l1", None), ("l1", "smoothl1", "l1"), ("l1", "smoothl1", "l2"), ("cb", "l2", "smoothl1")]


def worker(a):
    import torch

    import dasr_amd  # noqa: F401
    from dasr_amd import harness, ops, prep, synth
    assert torch.cuda.is_available(), "bench_criteria.py needs the GPU"
    dev = torch.device("cuda")
    B, h, w, s, K = a.frames, a.lr[0], a.lr[1], a.scale, 10
    gen = torch.Generator(device=dev).manual_seed(5)
    hr = torch.rand((B, 3, h * s, w * s), device=dev, generator=gen)
    sr = (hr + 0.3 * torch.randn((B, 3, h * s, w * s), device=dev, generator=gen)).clamp(-1, 2)
    sr.view(-1)[::97] += 2.0                                 # both smooth-L1 branches
    depth = synth.seeded_batch(0, B, h, w, s, K)[2].to(dev)
    onehot = prep.depth_to_masks(depth, K)
    assert prep.attach_region(onehot)
    from dasr_amd import graph
    region = graph.attached_region(onehot)
    soft = (0.7 * onehot + 0.3 * torch.rand(onehot.shape, device=dev, generator=gen)).contiguous()
    n = sr.numel()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, iters):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def versus(f_new, f_old, iters_new, iters_old):
        window(f_new, 2)
        window(f_old, 2)
        new, old = [], []
        for _ in range(3):
            new.append(window(f_new, iters_new))
            old.append(window(f_old, iters_old))
        return [round(v, 4) for v in new], [round(v, 4) for v in old]

    res = dict(shape=[B, 3, h * s, w * s], K=K, iters=a.iters, default={}, criteria={})
    for name, aux, f_sums, f_bwd in (("onehot", region, ops.loss_sums, ops.loss_bwd), ("soft", soft, ops.loss_sums_soft, ops.loss_bwd_soft)):
        dsums = (0.5 + torch.rand(2 * K + 1, device=dev, generator=gen)) / n
        new, old = versus(lambda: ops.loss_sums_crit(sr, hr, aux, K, "l1", "smoothl1"), lambda: f_sums(sr, hr, aux, K), a.iters, a.iters)
        mid = sorted(new)[1]
        res["default"][name + "_fwd"] = dict(new_ms=new, existing_ms=old, new_gbytes_per_s=round(2 * n * 4 / (mid * 1e-3) / 1e9, 1),
                                             existing_gbytes_per_s=round(2 * n * 4 / (sorted(old)[1] * 1e-3) / 1e9, 1))
        new, old = versus(lambda: ops.loss_bwd_crit(sr, hr, aux, dsums, K, "l1", "smoothl1"), lambda: f_bwd(sr, hr, aux, dsums, K),
                          a.iters, a.iters)
        res["default"][name + "_bwd"] = dict(new_ms=new, existing_ms=old,
                                             new_gbytes_per_s=round(3 * n * 4 / (sorted(new)[1] * 1e-3) / 1e9, 1),
                                             existing_gbytes_per_s=round(3 * n * 4 / (sorted(old)[1] * 1e-3) / 1e9, 1))
    for name, aux, masks in (("onehot", region, onehot), ("soft", soft, soft)):
        for p, ka, kb in COMBOS:
            nsum = (3 if kb else 2) * K + 1
            dsums = (0.5 + torch.rand(nsum, device=dev, generator=gen)) / n
            dsums[K:2 * K] = 0
            out = {}

            def fused():
                out["sums"] = ops.loss_sums_crit(sr, hr, aux, K, p, ka, kb)
                out["dsr"] = ops.loss_bwd_crit(sr, hr, aux, dsums, K, p, ka, kb)

            def torch_form():
                x = sr.detach().requires_grad_(True)
                sums = harness.criterion_sums_torch(x, hr, masks, p, ka, kb)
                (sums * dsums).sum().backward()
                out["ref"] = x.grad

            new, old = versus(fused, torch_form, a.iters, a.torch_iters)
            diff = ((out["dsr"] - out["ref"]).abs().max() / out["ref"].abs().max()).item()
            fwd = sorted(window(lambda: ops.loss_sums_crit(sr, hr, aux, K, p, ka, kb), a.iters) for _ in range(3))[1]
            bwd = sorted(window(lambda: ops.loss_bwd_crit(sr, hr, aux, dsums, K, p, ka, kb), a.iters) for _ in range(3))[1]
            res["criteria"]["%s %s/%s/%s" % (name, p, ka, kb or "-")] = dict(
                fused_ms=new, torch_ms=old, fwd_ms=round(fwd, 4), bwd_ms=round(bwd, 4),
                fwd_gbytes_per_s=round(2 * n * 4 / (fwd * 1e-3) / 1e9, 1), bwd_gbytes_per_s=round(3 * n * 4 / (bwd * 1e-3) / 1e9, 1),
                grad_max_diff_over_max=diff)
            out.clear()
    res["torch_peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--lr", type=int, nargs=2, default=(128, 160))
    ap.add_argument("--scale", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="time limit of the GPU child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criteria_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.worker:
        print(json.dumps(worker(a)), flush=True)
        return
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--frames", str(a.frames),
           "--lr", str(a.lr[0]), str(a.lr[1]), "--scale", str(a.scale), "--iters", str(a.iters), "--torch-iters", str(a.torch_iters)]
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(p.stdout, flush=True)
        raise SystemExit("bench_criteria.py: the GPU child ended with status %d" % p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
