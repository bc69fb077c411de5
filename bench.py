#!/usr/bin/env python3
"""bench.py — LR frames/s of the DepthNet hot path (fwd + losses + bwd + Adam) at x8, 128x160 LR.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One process per GPU; weak scaling (16 frames per GPU, BASELINE.json configs[1] at N=1).  Prints ONE JSON
line on rank 0.  `value` = frames all ranks processed / max-over-ranks wall time of exactly K steps, inputs
resident in HBM; `ms_per_step` = that wall time / K.

A plain run does what this figure needs and nothing else: set-up, W warm-up steps, the K timed steps, the result line.
`--dump-outputs DIR` then writes what the last timed step computed (see dump_outputs) so that two builds can be
compared output for output: the inputs are seeded, and the last timed step of such a run starts from the run's starting
parameters, so the same arguments give the same inputs and, to rounding, the same outputs in every run (the `loss` of
the result line is then that step's, too).

`--full` adds everything else the benchmark measures or checks, each in passes of its own after the timed region:
`roofline` (the DGB dynamic-conv + DFN modulation forward kernel, dasr_sean_fwd, timed with HIP events on its launch
stream: inside the timed steps and in one extra un-overlapped step), `roofline_b32` (the same kernel, forward only at
batch 32), `roofline_dominant` (the fp32 path's dominant convolution), the bf16 configurations' MFMA roofline, the
device-side getDepthMask against the host rule, and `cpu_baseline` (the CPU oracle on the host cores, rank 0 at N=1
only, bounded sample).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)     # (a step is 35-150 ms: the defaults finish in seconds; the CPU baseline is
    ap.add_argument("--warmup", type=int, default=3)     #  what takes the minute)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS), help="BASELINE.json config (default c2 = configs[1])")
    ap.add_argument("--batch", type=int, default=0, help="frames per GPU (default: the config's: c2 16, c3 32, c4 16, c5 1)")
    ap.add_argument("--mode", default="train", choices=("train", "infer"),
                    help="train (default): fwd + losses + bwd + Adam; infer: eval + no_grad forward with folded weights "
                         "(F_model_depthCond.test, F_model_depthCond.py:228-234) - never the driver's default")
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"),
                    help="cpu: the kernel emulator + gloo (tests of the launch / rank plumbing only; no timing claims)")
    ap.add_argument("--graph", default="auto", choices=("auto", "on", "off"),
                    help="capture the training step into one hipGraph (harness.Trainer(use_graph=True)).  auto = off: "
                         "measured on MI355X at c4 (x8, 16 frames, bf16) the replay of the ~2000-node two-stream graph is "
                         "no faster than eager launches (40.2 vs 38.8 ms/step: the step is GPU-bound, the host runs 6 ms ahead)")
    ap.add_argument("--split-pieces", type=int, default=None, choices=(2, 3),
                    help="A/B: 3 = three bf16 pieces / six products, 2 = two scaled fp16 pieces / three products (graph.SPLIT_PIECES)")
    ap.add_argument("--no-split", action="store_true",
                    help="A/B: fp32 path without the split-bf16 convolutions (graph.SPLIT_BF16 = False: exact-fp32 MFMA kernels)")
    ap.add_argument("--no-prepack", action="store_true",
                    help="A/B: one launch per packed kernel instead of the two multi-tensor launches per step (graph.PREPACK = False)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure: kernel rooflines (HIP-event timers, one "
                         "extra un-overlapped step, the forward-only batch-32 pass), device-side depth masks against the host "
                         "rule, the CPU oracle baseline.  Off by default: a plain run sets up, warms up, times the steps and prints")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline")
    ap.add_argument("--no-b32", action="store_true", help="with --full: skip the forward-only batch-32 roofline pass")
    ap.add_argument("--wgrad-stream", action="store_true",
                    help="experiment: weight gradients on a third stream (graph.WGRAD_STREAM; measured slower at c2)")
    ap.add_argument("--serial", action="store_true",
                    help="profiling aid: depth branch on the main stream (no co-running kernels, so a rocprofv3 kernel trace "
                         "shows isolated kernel durations); the reported value is then NOT the product configuration")
    return ap.parse_args(argv)


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) without a launcher: start torch.distributed.run as a CHILD process - one rank per
    GPU, rendezvous on 127.0.0.1 - and relay its output and exit code.  Nothing in this process has touched the GPU at
    this point (torch is not even imported), and nothing is exec'ed."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("[bench] launching %d ranks: %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


LR_H, LR_W, SCALE, K_REGIONS = 128, 160, 8, 10
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
MFMA_BF16_PEAK_TFS = 2500.0  # dense bf16 MFMA peak (same guide; AMD's 5 PF headline includes 2:1 sparsity)

# BASELINE.json configs.  c2 = configs[1] is the headline (the default, what the driver runs); c3 = configs[2] is the
# bf16 parity / roofline case, selected explicitly with --config c3 and never the default.
CONFIGS = {
    "c2": dict(scale=8, lr_hw=(128, 160), batch=16, dtype="f32",
               workload="Kvasir x8 synthetic, batch=%d per GPU, fp32, DepthNet nb=16 nf=64 L=256 K=10 (BASELINE.json "
                        "configs[1]); step = fwd + L1 + dynamic loss + bwd + Adam"),
    "c4": dict(scale=8, lr_hw=(128, 160), batch=16, dtype="bf16",
               workload="Kvasir x8 synthetic, batch=%d per GPU (BASELINE.json configs[3]: 128 over 8 GPUs), bf16 activations + "
                        "bf16-MFMA trunk convs (fp32 master weights / statistics / accumulators), DepthNet nb=16 nf=64 L=256 "
                        "K=10; step = fwd + L1 + dynamic loss + bwd + Adam"),
    "c5": dict(scale=2, lr_hw=(1080, 1920), batch=1, dtype="f32", which=list(range(16)),
               workload="EndoScene x2 synthetic, batch=%d per GPU (BASELINE.json configs[4]: 8 over 8 GPUs), one 1080x1920 LR "
                        "frame, fp32, DepthNet nb=16 nf=64 L=256 K=10, DGBs 0..15; step = fwd + L1 + dynamic loss + bwd + Adam"),
    "tiny": dict(scale=8, lr_hw=(16, 20), batch=1, dtype="f32", which=[0, 1], nb=4, latent=32,
                 workload="plumbing check only (tests/test_bench_launch.py): x8, batch=%d per rank, 16x20 LR, DepthNet nb=4 L=32"),
    "c3": dict(scale=4, lr_hw=(256, 320), batch=32, dtype="bf16",
               workload="Kvasir x4 synthetic, batch=%d per GPU, bf16 activations + bf16-MFMA trunk convs (fp32 master "
                        "weights / statistics / accumulators), DepthNet nb=16 nf=64 L=256 K=10, LR 256x320 (BASELINE.json "
                        "configs[2]); step = fwd + L1 + dynamic loss + bwd + Adam"),
}
# algorithmic FLOPs of the trunk per frame, forward + backward
TRUNK_GFLOP_PER_FRAME = {"c2": 848.0, "c3": 2685.0, "c4": 848.0}


def sean_algorithmic_bytes(B, H, W, C, K, residual):
    """3 activation reads (t, gamma2, beta2) + 1 write of C floats + K mask floats per LR pixel
    per SEAN call = 4*(4C) + 4K = 1064 B/px at C=64, K=10 (+ one more C-read for the residual variant)."""
    per_px = 4 * (4 * C + (C if residual else 0)) + 4 * K
    return per_px * B * H * W


def sean_kernel_bytes(B, H, W, C, K, residual):
    """What the one-hot gather kernel really moves: the same activation traffic but ONE region byte per pixel instead
    of the K mask floats (the planes are read once per forward by dasr_mask_compress / never with prep.depth_to_masks):
    1025 B/px, 1281 B/px with the residual read."""
    return (4 * (4 * C + (C if residual else 0)) + 1) * B * H * W


class SeanTimer:
    """Wraps ops.sean_fwd with HIP events recorded on the launch stream (torch's current stream)."""

    def __init__(self):
        self.pairs = []
        self.enabled = False
        self._orig = ops.sean_fwd

    def install(self):
        orig = self._orig

        def timed(t, mean, var, gb2, mask, region, flag, D, bias_g, bias_b, alpha_g, alpha_b, residual, relu, **kw):
            if not self.enabled:
                return orig(t, mean, var, gb2, mask, region, flag, D, bias_g, bias_b, alpha_g, alpha_b, residual, relu, **kw)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(t, mean, var, gb2, mask, region, flag, D, bias_g, bias_b, alpha_g, alpha_b, residual, relu, **kw)
            e1.record()
            B, H, W, C = t.shape
            self.pairs.append((e0, e1, sean_algorithmic_bytes(B, H, W, C, mask.shape[1], residual is not None),
                               (B, H, W, C, mask.shape[1], residual is not None)))
            return out

        ops.sean_fwd = timed

    def summary(self):
        if not self.pairs:
            return None
        ms = [p[0].elapsed_time(p[1]) for p in self.pairs]
        nbytes = [p[2] for p in self.pairs]
        avg_ms = sum(ms) / len(ms)
        avg_bytes = sum(nbytes) / len(nbytes)
        return avg_ms, avg_bytes, len(ms)

    def per_variant(self):
        """{residual?: (avg ms, launches, §8d bytes, kernel bytes)} of the recorded launches."""
        out = {}
        for res in (False, True):
            sel = [p for p in self.pairs if p[3][5] == res]
            if sel:
                ms = sum(p[0].elapsed_time(p[1]) for p in sel) / len(sel)
                out[res] = (ms, len(sel), sean_algorithmic_bytes(*sel[0][3]), sean_kernel_bytes(*sel[0][3]))
        return out


class ConvTimer:
    """HIP events around the forward launches of the trunk's dominant convolution (the gamma_o | beta_o 128 -> 128
    convs: 55 % of the trunk's forward FLOPs), on their launch stream."""

    def __init__(self):
        self.pairs = []
        self.enabled = False
        self._orig = ops.conv2d_fwd

    def install(self):
        orig = self._orig

        def timed(x, w, *a, **k):
            hot = self.enabled and x.dim() == 4 and x.shape[3] == 128 and w.shape[4] == 128 and w.shape[1] == 3
            if not hot:
                return orig(x, w, *a, **k)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(x, w, *a, **k)
            e1.record()
            B, H, W, _ = x.shape
            self.pairs.append((e0, e1, 2.0 * 9 * 128 * 128 * B * H * W))
            return out

        ops.conv2d_fwd = timed
        from dasr_amd import graph as g
        g.ops.conv2d_fwd = timed


class SplitTimer:
    """HIP events around the launches of the fp32 path's dominant kernel - k_conv3x3_split<4, NP> on the 128 -> 128
    gamma_o | beta_o convolution, forward: an fp32 convolution as NP-piece products on the 16-bit matrix cores
    (dasr_conv3x3_fwd_split2: two fp16 pieces, three MFMA products per term; dasr_conv3x3_fwd_split: three bf16 pieces, six)."""

    def __init__(self):
        self.pairs = []
        self.enabled = False
        self.products = None

    def install(self):
        from dasr_amd import graph as g

        def wrap(orig, products, xi, ci):
            def timed(*a, **k):
                x, Cout = a[xi], a[ci]
                if not (self.enabled and x.shape[3] == 128 and Cout == 128):
                    return orig(*a, **k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = orig(*a, **k)
                e1.record()
                B, H, W, _ = x.shape
                self.pairs.append((e0, e1, 2.0 * 9 * 128 * 128 * B * H * W))
                self.products = products
                return out
            return timed

        ops.conv3x3_fwd_split = wrap(ops.conv3x3_fwd_split, 6, 0, 3)          # (x, ws, bias, Cout, ...)
        ops.conv3x3_fwd_split2 = wrap(ops.conv3x3_fwd_split2, 3, 0, 4)        # (x, xmax, ws, bias, Cout, ...)
        g.ops.conv3x3_fwd_split = ops.conv3x3_fwd_split
        g.ops.conv3x3_fwd_split2 = ops.conv3x3_fwd_split2

    def summary(self):
        if not self.pairs:
            return None
        ms = [a.elapsed_time(b) for a, b, _ in self.pairs]
        avg_ms = sum(ms) / len(ms)
        fl = self.pairs[0][2]
        n = self.products
        tf = n * fl / (avg_ms * 1e-3) / 1e12
        what = ("two scaled fp16 pieces per operand, three fp16 MFMA products per term (dasr_conv3x3_fwd_split2)" if n == 3 else
                "three bf16 pieces per operand, six bf16 MFMA products per term (dasr_conv3x3_fwd_split)")
        return {"bound": "mfma", "kernel": "k_conv3x3_split<4,%d>: fp32 128->128 gamma_o|beta_o conv, forward - %s" % (3 if n == 6 else 2, what),
                "achieved": round(tf, 1), "peak": MFMA_BF16_PEAK_TFS, "unit": "TFLOP/s",
                "frac": round(tf / MFMA_BF16_PEAK_TFS, 4), "traffic": None, "launches_timed": len(ms),
                "avg_launch_us": round(avg_ms * 1e3, 2), "algorithmic_flops_per_launch": n * fl,
                "fp32_equivalent_tflops": round(fl / (avg_ms * 1e-3) / 1e12, 1),
                "measured": "HIP events on the launch stream, one extra un-overlapped step after the timed region; "
                            "FLOPs = %d 16-bit products x 2*9*128*128 per pixel (the fp32-equivalent rate counts one); peak = the "
                            "dense bf16 / fp16 MFMA rate" % n}


def arithmetic_note(dtype):
    """How the configuration computes, in words (config.arithmetic): `dtype` names storage and accumulation; the fp32 path's
    convolutions run as split products on the 16-bit matrix cores at fp32 accuracy unless --no-split."""
    from dasr_amd import graph as g
    if dtype != "f32":
        return "bf16 activations and bf16 MFMA operands, fp32 accumulators / statistics / master weights"
    if not g.SPLIT_BF16:
        return "fp32 tensors, exact-fp32 MFMA convolutions (v_mfma_f32_32x32x2_f32)"
    if g.SPLIT_PIECES == 2:
        return ("fp32 tensors and fp32 accumulation; 3x3 trunk convolutions%s as fp16 x 2 split products (two scaled fp16 pieces per "
                "operand, three MFMA products per term): error against float64 below the exact-fp32 MFMA kernels', same parity "
                "gates (DESIGN.md 4.11); --no-split runs the exact-fp32 kernels" % (" and the 9x9 output convolution" if g.SPLIT_CONV9 else ""))
    return ("fp32 tensors and fp32 accumulation; 3x3 trunk convolutions as bf16 x 3 split products (three bf16 pieces per operand, six "
            "MFMA products per term): fp32-grade (DESIGN.md 4.11); --no-split runs the exact-fp32 kernels")


def mfma_roofline(net, args, B, elapsed, timer_conv, config):
    """bf16 configs (c3, c4): the step is bound by the bf16 matrix cores.  `achieved` = algorithmic FLOPs of one launch of the
    dominant kernel (k_conv3x3_bf16 on the 128 -> 128 gamma_o|beta_o convolution, 2*9*128*128 FLOP per pixel) / its
    average launch duration, measured with HIP events in one extra un-overlapped forward after the timed region; the
    whole step's trunk FLOPs (2685 GFLOP per frame fwd+bwd) over the step time are reported next to it."""
    from dasr_amd import graph as _graph
    lq, dm, mk = net._bench_inputs
    side = _graph.SIDE_STREAM
    _graph.SIDE_STREAM = False
    try:
        with torch.no_grad():
            timer_conv.pairs = []
            timer_conv.enabled = True
            net(lq, dm, mk)
            torch.cuda.synchronize()
            timer_conv.enabled = False
    finally:
        _graph.SIDE_STREAM = side
    if not timer_conv.pairs:
        return None
    ms = [a.elapsed_time(b) for a, b, _ in timer_conv.pairs]
    flops = timer_conv.pairs[0][2]
    avg_ms = sum(ms) / len(ms)
    ach = flops / (avg_ms * 1e-3) / 1e12
    step_tf = TRUNK_GFLOP_PER_FRAME[config] * 1e9 * B * args.steps / elapsed / 1e12
    return {"bound": "mfma", "kernel": "k_conv3x3_bf16_v2<NT=4> (dasr_conv2d_fwd_bf16, 128->128 gamma_o|beta_o conv, forward; "
                                       "persistent LDS-DMA kernel)",
            "achieved": round(ach, 1), "peak": MFMA_BF16_PEAK_TFS, "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFS, 4),
            "traffic": None, "launches_timed": len(ms), "avg_launch_us": round(avg_ms * 1e3, 2),
            "algorithmic_flops_per_launch": flops,
            "measured": "HIP events on the launch stream, one un-overlapped forward pass after the timed region",
            "whole_step": {"trunk_gflop_per_frame_fwd_bwd": TRUNK_GFLOP_PER_FRAME[config], "achieved_tflops": round(step_tf, 1),
                           "frac_of_bf16_mfma_peak": round(step_tf / MFMA_BF16_PEAK_TFS, 4),
                           "note": "the 9x9 output conv and the fp32 encoder run on the fp32 matrix cores; SEAN, "
                                   "statistics and epilogue-backward kernels are HBM-bound"}}


def host_cores():
    """CPU cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = os.cpu_count() or 1
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:  # cgroup v2
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except Exception:
            pass
    return n


def cpu_baseline(frames=4, steps=3, max_warmup=5):
    """CPU oracle (as-written PyTorch restatement of the reference, oracle/depthnet_oracle.py) on the host
    cores: forward + losses + backward + Adam on `frames` frame(s) of the same x8 workload.  Warm-up steps run until two
    consecutive ones agree within 10 % (thread pools, allocator and oneDNN primitive caches settle over the first
    steps), then `steps` timed steps; `value` is their median."""
    from oracle import depthnet_oracle as O
    cores = min(host_cores(), 32)
    torch.set_num_threads(cores)
    cfg = O.make_cfg()
    sd = O.new_state_dict(cfg)
    synth.closed_form_fill_(sd.items())
    for v in sd.values():
        v.requires_grad_(True)
    w = torch.ones(K_REGIONS, requires_grad=True)
    optim = torch.optim.Adam(list(sd.values()) + [w], lr=1e-3, betas=(0.9, 0.99))
    lq, gt, dm, mk = synth.seeded_batch(0, frames, LR_H, LR_W, SCALE, K_REGIONS)

    def one_step(tag):
        t0 = time.perf_counter()
        optim.zero_grad(set_to_none=True)
        sr = O.depthnet_forward(sd, cfg, lq, dm, mk)
        t1 = time.perf_counter()
        total, _, _, _ = O.total_loss(sr, gt, mk, w)
        total.backward()
        optim.step()
        t2 = time.perf_counter()
        print("[bench] cpu baseline %s: forward %.2f s, loss+backward+Adam %.2f s (%d threads)"
              % (tag, t1 - t0, t2 - t1, cores), file=sys.stderr, flush=True)
        return t2 - t0, t1 - t0

    warm = []
    for i in range(max_warmup):
        warm.append(one_step("warm-up %d" % (i + 1))[0])
        if len(warm) >= 2 and abs(warm[-1] - warm[-2]) <= 0.10 * warm[-1]:
            break
    timed = [one_step("timed step %d/%d" % (i + 1, steps)) for i in range(steps)]
    times = sorted(t for t, _ in timed)
    med = times[len(times) // 2]
    fwd = sorted(f for _, f in timed)[len(timed) // 2]
    return {"value": round(frames / med, 4), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "%d frame(s) x8 128x160; %d warm-up step(s) (until two agreed within 10 %%: %s s) + %d timed "
                      "fwd+loss+bwd+Adam steps of the CPU oracle (median; all: %s s); forward-only %.3f frames/s"
                      % (frames, len(warm), "/".join("%.1f" % t for t in warm), steps,
                         "/".join("%.1f" % t for t in times), frames / fwd)}


DUMP_MAX_ELEMS = 1 << 22      # per array: 4 Mi float32 = 16 MiB


def dump_outputs(out_dir, sr, log):
    """What the caller of the timed path holds after its last timed step, as <out_dir>/<name>.npy:

      sr.npy    float32  the generator's output of that step (the forward of net(lq, depthMap, depthMask), which the training
                         step feeds to its losses and the inference step returns), flattened in NCHW order; above
                         DUMP_MAX_ELEMS elements a fixed sample of it (sorted indices drawn once from a generator seeded
                         with 0, so every run and every build picks the same elements)
      loss.npy  float64  [l_all, l_pix, l_dynamic], the log optimize_parameters returns (training mode only)

    The inputs are the same in every run, the parameters of the dumped step included: in a training run main() puts the
    parameters the run started from back in front of the last timed step (the weight-gradient slabs are summed with atomics
    and Adam turns that rounding noise into +-lr steps, so parameters that went through the earlier steps differ from run to
    run by far more than rounding: 2.8e-3 on average in sr.npy after 3 + 10 steps).  Measured on MI355X, three runs of one
    build at c2, 3 + 10 steps: sr.npy bit-identical, loss.npy within 2.4e-7; `--mode infer` is bit-identical as well.
    """
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    if sr is not None:
        flat = sr.detach().float().reshape(-1)
        if flat.numel() > DUMP_MAX_ELEMS:
            g = torch.Generator(device="cpu")
            g.manual_seed(0)
            idx = torch.randint(flat.numel(), (DUMP_MAX_ELEMS,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        np.save(os.path.join(out_dir, "sr.npy"), flat.cpu().numpy().astype(np.float32))
    if log:
        np.save(os.path.join(out_dir, "loss.npy"),
                np.array([float(log[k]) for k in ("l_all", "l_pix", "l_dynamic")], dtype=np.float64))


def main():
    args = parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be at least 1 and --warmup at least 0")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))

    global torch, dist, harness, networks, ops, prep, synth
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # (dmabuf IPC: RCCL between ranks needs it on this driver; before HIP starts)
    import torch
    import torch.distributed as dist
    cpu = args.device == "cpu"
    if cpu:                                   # the CPU kernel emulator: test plumbing, never a measurement
        sys.path.insert(0, ROOT)
        import dasr_amd  # noqa: F401
        from dasr_amd import build as _build
        os.environ["DASR_HIPEMU_LIB"] = _build.build_emu()
    import dasr_amd  # noqa: F401,F811
    from dasr_amd import harness, networks, ops, prep, synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (python bench.py --gpus N does it "
                         "itself)" % (args.gpus, world))
    if cpu:
        dev = torch.device("cpu")
        torch.set_num_threads(max(1, host_cores() // max(1, world)))
    else:
        assert torch.cuda.is_available(), "bench.py needs the MI355X"
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    sync = (lambda: None) if cpu else torch.cuda.synchronize
    group = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if cpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        group = dist.group.WORLD

    cfg = CONFIGS[args.config]
    if args.wgrad_stream:
        from dasr_amd import graph as _graph_mod2
        _graph_mod2.WGRAD_STREAM = True
    if args.no_split:
        from dasr_amd import graph as _graph_mod3
        _graph_mod3.SPLIT_BF16 = False
    if args.no_prepack:
        from dasr_amd import graph as _graph_mod5
        _graph_mod5.PREPACK = False
    if args.split_pieces is not None:
        from dasr_amd import graph as _graph_mod4
        _graph_mod4.SPLIT_PIECES = args.split_pieces
    if args.serial:
        from dasr_amd import graph as _graph_mod
        _graph_mod.SIDE_STREAM = False
        print("[bench] --serial: depth branch on the main stream (profiling aid, not the product configuration)",
              file=sys.stderr, flush=True)
    global LR_H, LR_W, SCALE
    (LR_H, LR_W), SCALE = cfg["lr_hw"], cfg["scale"]
    opt = {"network_G": dict(networks.X8_NETWORK_G, upscale=SCALE), "datasets": {"train": {"depthMaskNum": K_REGIONS}}}
    if "which" in cfg:
        opt["network_G"]["which_ResBlk_depth"] = list(cfg["which"])
    if "nb" in cfg:
        opt["network_G"]["nb"] = cfg["nb"]
    if "latent" in cfg:
        opt["network_G"]["depth_latent_ch"] = cfg["latent"]
    net = networks.define_G(opt)
    synth.closed_form_fill_(net.state_dict().items())
    net = net.to(dev)
    if cfg["dtype"] == "bf16":
        net.set_compute_dtype(torch.bfloat16)          # explicit: fp32 is what every other path of this repo runs
    use_graph = (not cpu) and world == 1 and args.graph == "on"
    trainer = harness.Trainer(net, K_REGIONS, group=group, use_graph=use_graph)
    if use_graph and args.warmup < 4:
        args.warmup = 4                        # three eager steps + the capture happen before the timed region
    B = args.batch or cfg["batch"]
    lq, gt, dm, mk_host = synth.seeded_batch(rank * B, B, LR_H, LR_W, SCALE, K_REGIONS)
    lq, gt, dm = lq.to(dev), gt.to(dev), dm.to(dev)
    # the depth masks are derived from the depth map ON THE DEVICE (prep.depth_to_masks = getDepthMask, pinned to the
    # reference's function by tests/golden/depth_masks.npz): same planes as the host rule, plus the region bytes the
    # one-hot kernels read, so no rank ever reads a flag back from the GPU inside a step
    if cpu:
        mk = mk_host
    else:
        mk = prep.depth_to_masks(dm, K_REGIONS)
        if args.full:
            assert torch.equal(mk.cpu(), mk_host), "device-side getDepthMask differs from the host rule"
    del mk_host
    object.__setattr__(net, "_bench_inputs", (lq, dm, mk))

    timer = SeanTimer()
    timer_conv = ConvTimer()
    timer_split = SplitTimer()
    extras = args.full and not cpu                 # the kernel timers and the passes after the timed region: --full only
    if extras:
        timer.install()
        if cfg["dtype"] == "f32":
            timer_split.install()
        if cfg["dtype"] == "bf16":
            timer_conv.install()
    infer = args.mode == "infer"
    if infer:
        net.eval()

    def step():
        if infer:
            with torch.no_grad():
                return net(lq, dm, mk)
        return trainer.optimize_parameters(lq, gt, dm, mk)

    def barrier():
        if world > 1:
            dist.barrier()

    def note(msg):
        if rank == 0:
            print("[bench] " + msg, file=sys.stderr, flush=True)

    # --dump-outputs, training: the weight gradients are summed with atomics and Adam turns their rounding noise into +-lr
    # steps, so after a few steps the parameters of two runs differ by far more than rounding.  The dumped step therefore
    # starts from the parameters the run started from (one multi-tensor copy in front of the last timed step; the snapshot
    # is taken here, before the warm-up): what it computes is a function of the seeded inputs and the closed-form fill
    # alone.  Runs without --dump-outputs do none of this.
    start_params = None
    if args.dump_outputs and not infer:
        start_params = [p.detach().clone() for p in trainer.params]
    note("inputs resident; %d warm-up step(s)" % args.warmup)
    for i in range(args.warmup):
        step()
        sync()
        note("warm-up step %d done" % (i + 1))
    sync()
    barrier()
    sync()
    timer.enabled = extras
    last_sr, hook = [], None
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.dump_outputs and i == args.steps - 1:
            if start_params is not None:
                with torch.no_grad():
                    torch._foreach_copy_(trainer.params, start_params)
            if rank == 0:                          # keep the last step's forward output for the dump
                hook = net.register_forward_hook(lambda _mod, _inp, out: last_sr.append(out.detach()))
        step()
    host_enqueue = time.perf_counter() - t0       # the host has issued every launch of the timed steps (no sync in a step)
    sync()
    barrier()
    sync()
    elapsed = time.perf_counter() - t0
    note("host enqueue %.1f ms/step of %.1f ms/step" % (host_enqueue / args.steps * 1e3, elapsed / args.steps * 1e3))
    timer.enabled = False
    el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = el.item()
    loss = float(trainer.log["l_all"]) if not infer else float("nan")
    if hook is not None:
        hook.remove()
    if args.dump_outputs and rank == 0:
        # (a replayed hipGraph step runs no Python forward: then the log alone is what the caller holds)
        dump_outputs(args.dump_outputs, last_sr[0] if last_sr else None, None if infer else trainer.log)
        note("outputs of the last timed step written to %s" % args.dump_outputs)
    del last_sr

    # Roofline of the dynamic-conv forward kernel.  In the timed steps the kernel shares the GPU with the side
    # stream's convolutions (graph.SIDE_STREAM), which stretches its duration and says nothing about the kernel, so
    # ONE extra, untimed step is run with the side stream off and the same HIP-event timers: that is `achieved`;
    # the duration seen inside the timed (overlapped) steps is reported next to it.
    overlapped = timer.summary()
    timer.pairs = []
    from dasr_amd import graph as _graph
    _side = _graph.SIDE_STREAM
    roof = None
    if extras:
        _graph.SIDE_STREAM = False
        timer.enabled = True
        timer_split.enabled = True
        if use_graph and not infer:
            trainer._eager_step(lq, gt, dm, mk)    # (a replay carries no Python-side timers: this one step runs eagerly)
        else:
            step()
        sync()
        timer.enabled = False
        timer_split.enabled = False
        _graph.SIDE_STREAM = _side
    s = timer.summary()
    if s is not None:
        avg_ms, avg_bytes, n = s
        achieved = avg_bytes / (avg_ms * 1e-3) / 1e9
        roof = {"bound": "hbm", "kernel": "k_sean_fwd_onehot (dasr_sean_fwd: DGB dynamic conv + DFN modulation, forward)",
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None, "launches_timed": n,
                "avg_launch_us": round(avg_ms * 1e3, 2), "algorithmic_bytes_per_launch": int(avg_bytes),
                "measured": "HIP events on the launch stream, one extra un-overlapped step after the timed region"}
        pv = timer.per_variant()
        for res, (ms, n, alg, true_b) in pv.items():
            roof["residual" if res else "no_residual"] = {
                "avg_launch_us": round(ms * 1e3, 2), "launches": n, "frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "frac_kernel_minimum": round(true_b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        if overlapped is not None:
            o_ms, o_bytes, o_n = overlapped
            roof["in_timed_region"] = {"avg_launch_us": round(o_ms * 1e3, 2), "launches": o_n,
                                       "achieved": round(o_bytes / (o_ms * 1e-3) / 1e9, 1),
                                       "note": "co-running with the side-stream convolutions"}
        pmc = os.path.join(ROOT, "profiles", "sean_fwd_pmc.json")
        if os.path.exists(pmc):
            try:
                rec = json.load(open(pmc))
                if rec.get("B") == B:          # counters were collected at this launch size
                    roof["traffic"] = int(rec.get("hbm_bytes_per_launch"))
                    roof["traffic_source"] = ("profiles/sean_fwd_pmc.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes "
                                              "of this command at this launch size (tools/pmc_sean.py), NOT collected in "
                                              "this run - counters cannot be read from inside the process")
            except Exception:
                pass

    # The north-star point: the same kernel at batch 32 (north_star: ">= 70 % of HBM roofline on the DGB dynamic-conv
    # forward at batch 32").  One un-overlapped FORWARD-ONLY pass (no tape, side stream off) on rank 0, per variant
    # (13 launches without / 13 with the residual read); both byte counts are reported: SURVEY §8d's (K mask floats as
    # delivered) and the kernel's true minimum (one region byte).
    roof32 = None
    if rank == 0 and extras and not infer and not args.no_b32 and args.config == "c2":
        note("forward-only pass at batch 32 for roofline_b32")
        trainer = None
        net.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        B32 = 32
        lq32, _, dm32, _ = synth.seeded_batch(1000, B32, LR_H, LR_W, SCALE, K_REGIONS)
        lq32, dm32 = lq32.to(dev), dm32.to(dev)
        mk32 = prep.depth_to_masks(dm32, K_REGIONS)
        _graph.SIDE_STREAM = False
        try:
            with torch.no_grad():
                net(lq32, dm32, mk32)                       # warm-up
                torch.cuda.synchronize()
                timer.pairs = []
                timer.enabled = True
                for _ in range(3):
                    net(lq32, dm32, mk32)
                torch.cuda.synchronize()
                timer.enabled = False
        finally:
            _graph.SIDE_STREAM = _side
        pv = timer.per_variant()
        if pv:
            roof32 = {"bound": "hbm", "kernel": "k_sean_fwd_onehot", "batch": B32, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "measured": "HIP events, 3 un-overlapped forward-only passes after the timed region"}
            tot_ms = tot_alg = tot_true = 0.0
            for res, (ms, n, alg, true_b) in pv.items():
                key = "residual" if res else "no_residual"
                roof32[key] = {"avg_launch_us": round(ms * 1e3, 2), "launches": n, "bytes_survey_8d": alg,
                               "bytes_kernel_minimum": true_b,
                               "achieved": round(alg / (ms * 1e-3) / 1e9, 1),
                               "frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                               "frac_kernel_minimum": round(true_b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
                tot_ms += ms * n
                tot_alg += alg * n
                tot_true += true_b * n
            roof32["achieved"] = round(tot_alg / (tot_ms * 1e-3) / 1e9, 1)
            roof32["frac"] = round(roof32["achieved"] / HBM_PEAK_GBS, 4)
            roof32["frac_kernel_minimum"] = round(tot_true / (tot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            pmc32 = os.path.join(ROOT, "profiles", "sean_fwd_pmc_b32.json")
            roof32["traffic"] = None
            if os.path.exists(pmc32):
                try:
                    roof32["traffic"] = int(json.load(open(pmc32)).get("hbm_bytes_per_launch"))
                except Exception:
                    pass
        del lq32, dm32, mk32

    if cfg["dtype"] == "bf16" and extras:
        roof = mfma_roofline(net, args, B, elapsed, timer_conv, args.config)
    # rank 0 alone ran the batch-32 pass: the other ranks wait here, so nobody tears the process group down under it
    barrier()

    if rank == 0:
        out = {
            "metric": ("LR frames/sec fwd+bwd at x%d (%dx%d LR)" if not infer else
                       "LR frames/sec inference forward (eval + no_grad, folded weights) at x%d (%dx%d LR)") % (SCALE, LR_H, LR_W),
            "value": round(world * B * args.steps / elapsed, 3),
            "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": cfg["dtype"], "data": "synthetic",
            "config": {"workload": cfg["workload"] % B,
                       "global_batch": world * B, "lr_hw": [LR_H, LR_W], "scale": SCALE,
                       "parallelism": "dp%d" % world, "mode": args.mode, "device": args.device, "full": bool(args.full),
                       "hip_graph": bool(use_graph), "arithmetic": arithmetic_note(cfg["dtype"])},
            "loss": round(loss, 6) if loss == loss else None,
            "roofline": roof,
            "roofline_b32": roof32,
            "roofline_dominant": timer_split.summary(),
        }
        if world == 1 and extras and not infer and not args.no_cpu_baseline and args.config == "c2":
            note("GPU part done (%.1f ms/step); timing the CPU oracle baseline" % (1e3 * elapsed / args.steps))
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
