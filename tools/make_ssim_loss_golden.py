#!/usr/bin/env python3
"""Generate tests/golden/ssim_loss.npz from the REFERENCE's SSIM criterion (build container only).

Run:  python tools/make_ssim_loss_golden.py          (needs the reference checkout: DASR_REFERENCE, or ../reference; CPU; a second)

``codes/models/modules/ssim_loss.py`` imports torch, numpy and math only, so the module is loaded from where it lies
(importlib, at generation time only); nothing of it is copied.  The fixture holds data only - what the reference's
``SSIM()`` computed on the image pairs of tests/ssim_loss_checks.pairs():

    <name>.value     its fp32 run (the criterion as the reference trainer evaluates it)
    <name>.value64   its float64 run
    <name>.grad64    d value64 / d img1, float64 [B,C,H,W]

The inputs are RNG-free (tests/ssim_loss_checks.make_pair) and are not stored.  The zip members carry a fixed date."""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DASR_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden")


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


def main():
    sys.path.insert(0, ROOT)
    import dasr_amd  # noqa: F401  (registers the package alias the tests import)
    from tests.ssim_loss_checks import pairs
    spec = importlib.util.spec_from_file_location("ref_ssim_loss", os.path.join(REF, "codes", "models", "modules", "ssim_loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.set_num_threads(1)
    arrays = {}
    for name, (a, b) in pairs().items():
        arrays[name + ".value"] = np.float64(float(ref.SSIM()(a, b)))
        x = a.double().requires_grad_(True)
        v = ref.SSIM()(x, b.double())
        v.backward()
        arrays[name + ".value64"] = np.float64(v.item())
        arrays[name + ".grad64"] = x.grad.numpy()
        print(name, tuple(a.shape), v.item(), float(x.grad.abs().max()))
    save("ssim_loss", **arrays)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
