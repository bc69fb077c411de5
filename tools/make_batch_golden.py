#!/usr/bin/env python3
"""Generate tests/golden/batch_*.npz from the REFERENCE loader code (build container only).

Run:  python tools/make_batch_golden.py          (needs the reference checkout; CPU; a few seconds)

``codes/data/util.py`` and ``codes/data/LQGTker_Depth_dataset.py`` import cv2 / lmdb, which are not installed here, so the
modules cannot be imported.  The functions this needs - ``cubic``, ``calculate_weights_indices``, ``imresize_np``,
``augment`` and ``getDepthMask`` - use torch, numpy, math and random only: their ``FunctionDef`` nodes are taken from the
files' ASTs where they lie and compiled on their own at run time (as oracle/make_golden.py does for ``getDepthMask``).
Nothing of the files is copied; the fixtures hold data only: the inputs generated here and what the reference computed.

Per case ``batch_<H>x<W>x<s>.npz``: ``hr`` uint8 [H,W,3] BGR (random bytes with rectangles of pure 0 and 255), ``lr``
float32 [h,w,3] = imresize_np(hr / 255, 1/s, True), ``depth`` float32 [1,h,w], ``masks`` / ``masks_fixed`` uint8 [K,h,w]
= getDepthMask per-sample / fixed range, and for the cases listed in AUGMENTED ``aug_flags`` plus ``aug_lr`` /
``aug_gt`` / ``aug_depth`` / ``aug_masks`` = the reference's augment of [LR, GT, depth, masks] under those flags (HWC,
BGR, as augment returns them).  ``batch_augment_flags.npz``: for (use_flip, use_rot) in OPTIONS and random.seed(k),
k = 0..31, the flags augment applied (decoded from what it did to an index image) and the next random.random() after it.

Reproducibility.  The reference's ``imresize_np`` sums its taps with ``Tensor.mv``, a BLAS call whose summation order
depends on the CPU and the BLAS build: on another machine about half of the ``lr`` values come out 1-2 ulp away.  A fixture
that can be regenerated only where it was made is no recipe, so this tool pins the one thing that varies: while the
reference's function runs, ``Tensor.mv`` is replaced by ``pinned_mv`` below - the same fp32 matrix-vector product with separately rounded IEEE
multiplies and adds in one fixed order, a balanced pairwise tree over the taps (numpy elementwise arithmetic, which no CPU
evaluates differently).  Everything else is the reference's code, run single-threaded with ATen's unvectorised
kernels (ATEN_CPU_CAPABILITY=default, set before torch is imported) so that its elementwise weight computation does not
depend on the CPU's vector width either.  ``lr`` is therefore "imresize_np with its dot products summed pairwise";
the tests measure the reference's fp32 rounding (e_ref) on exactly that.  The zip members carry a fixed date.  With
this, a second run - here or on another x86-64 machine - writes the same bytes."""
import os
os.environ["ATEN_CPU_CAPABILITY"] = "default"          # before torch is imported (see Reproducibility above)
os.environ["OMP_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = "1"
import ast
import io
import contextlib
import math
import random
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DASR_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

CASES = [(48, 64, 8), (36, 48, 3), (39, 51, 3), (40, 56, 2), (48, 48, 4), (264, 152, 8), (16, 24, 8)]
AUGMENTED = {(48, 64, 8): 3, (48, 48, 4): 7}          # case -> flags of the stored augmented four-tuple
OPTIONS = [(True, True), (True, False), (False, True), (False, False)]
K = 10


def pinned_mv(self, vec):
    """``self.mv(vec)`` in fp32 with a fixed order: the products self[:, k] * vec[k], each rounded, are added pairwise -
    neighbours first, then neighbouring sums, an odd one carried up - the balanced tree a vectorised BLAS kernel
    approximates (no fused multiply-add, no dependence on blocking or vector width)."""
    m, v = self.detach().numpy().astype(np.float32, copy=False), vec.detach().numpy().astype(np.float32, copy=False)
    terms = [m[:, k] * v[k] for k in range(m.shape[1])]
    while len(terms) > 1:
        nxt = [terms[i] + terms[i + 1] for i in range(0, len(terms) - 1, 2)]
        if len(terms) % 2:
            nxt.append(terms[-1])
        terms = nxt
    return torch.from_numpy(np.ascontiguousarray(terms[0], dtype=np.float32))


@contextlib.contextmanager
def pinned_summation():
    real = torch.Tensor.mv
    torch.Tensor.mv = pinned_mv
    try:
        yield
    finally:
        torch.Tensor.mv = real


def reference_functions(path, names, ns):
    tree = ast.parse(open(path).read(), path)
    for name in names:
        fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
        assert len(fn) == 1, (path, name, len(fn))
        exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns


def save(name, **arrays):
    """np.savez_compressed with a fixed member date (numpy stamps the current time)."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue(), compresslevel=9)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def hr_image(H, W, s, gen):
    """Random bytes, with saturated rectangles next to each other and at the borders so that the resize overshoots."""
    img = gen.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    a, b = max(2, H // 4), max(2, W // 4)
    img[:a, :b] = 255
    img[:a, b:2 * b] = 0
    img[H - a:, W - b:] = 0
    img[H - a:, W - 2 * b:W - b] = 255
    img[H // 2 - a // 2:H // 2 + a // 2, W // 2 - b // 2:W // 2, 1] = 255
    img[H // 2 - a // 2:H // 2 + a // 2, W // 2:W // 2 + b // 2, 1] = 0
    return img


def apply_flags(img, flags):
    if flags & 1:
        img = img[:, ::-1, :]
    if flags & 2:
        img = img[::-1, :, :]
    if flags & 4:
        img = img.transpose(1, 0, 2)
    return img


def main():
    ns = {"torch": torch, "np": np, "math": math, "random": random}
    reference_functions(os.path.join(REF, "codes", "data", "util.py"),
                        ("cubic", "calculate_weights_indices", "imresize_np", "augment"), ns)
    reference_functions(os.path.join(REF, "codes", "data", "LQGTker_Depth_dataset.py"), ("getDepthMask",), ns)
    imresize_np, augment, get_masks = ns["imresize_np"], ns["augment"], ns["getDepthMask"]
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)

    for n, (H, W, s) in enumerate(CASES):
        gen = np.random.default_rng(7000 + n)
        hr = hr_image(H, W, s, gen)
        gt = hr.astype(np.float32) / 255.                                   # read_img
        with pinned_summation():
            lr = imresize_np(gt, 1 / s, True)
        h, w = H // s, W // s
        assert lr.shape == (h, w, 3) and lr.dtype == np.float32
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        depth = (0.5 + 0.45 * np.sin(0.37 * yy + 0.2 * n) * np.cos(0.29 * xx) + 0.04 * gen.random((h, w))).astype(np.float32)
        depth[0, 0], depth[h - 1, w - 1] = -0.05, 1.02                      # outside [0, 1): no bin in fixed-range mode
        depth = depth[None]
        arrays = dict(hr=hr, lr=lr, depth=depth)
        for key, fixed in (("masks", False), ("masks_fixed", True)):
            m = get_masks(None, torch.from_numpy(depth.copy()), depthFixedRange=fixed, depthMaskNum=K)
            assert tuple(m.shape) == (K, h, w)
            arrays[key] = m.numpy().astype(np.uint8)
        flags = AUGMENTED.get((H, W, s))
        if flags is not None:
            seed = next(k for k in range(1000) if _flags_of(augment, k, True, True)[0] == flags)
            random.seed(seed)
            tup = augment([lr, gt, depth.transpose(1, 2, 0), arrays["masks"].astype(np.float32).transpose(1, 2, 0)], True, True,
                          "LQGTker_Depth")
            arrays.update(aug_flags=np.uint8(flags), aug_lr=tup[0], aug_gt=tup[1], aug_depth=tup[2],
                          aug_masks=np.ascontiguousarray(tup[3]).astype(np.uint8))
        save("batch_%dx%dx%d" % (H, W, s), **arrays)

    flags = np.zeros((len(OPTIONS), 32), dtype=np.uint8)
    nxt = np.zeros((len(OPTIONS), 32), dtype=np.float64)
    for o, (use_flip, use_rot) in enumerate(OPTIONS):
        for k in range(32):
            flags[o, k], nxt[o, k] = _flags_of(augment, k, use_flip, use_rot)
    save("batch_augment_flags", options=np.array(OPTIONS, dtype=np.uint8), flags=flags, next_random=nxt)


def _flags_of(augment, seed, use_flip, use_rot):
    """What augment does under random.seed(seed), decoded from an index image, and the generator's next value."""
    index = np.arange(6, dtype=np.float32).reshape(2, 3, 1)
    random.seed(seed)
    got = augment([index], use_flip, use_rot, "LQGTker_Depth")[0]
    nxt = random.random()
    match = [f for f in range(8) if apply_flags(index, f).shape == got.shape and np.array_equal(apply_flags(index, f), got)]
    assert len(match) == 1, match
    return match[0], nxt


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
