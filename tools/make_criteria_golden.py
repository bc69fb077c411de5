#!/usr/bin/env python3
"""Generate tests/golden/criteria.npz from the REFERENCE's criteria (build container only).

Run:  python tools/make_criteria_golden.py          (needs the reference checkout: DASR_REFERENCE, or ../reference; CPU; seconds)

``codes/models/modules/mask_loss.py`` and ``loss.py`` import torch and numpy only, so the modules are loaded from where they
lie (importlib, at generation time only); nothing of them is copied.  The fixture holds data only - the inputs of
tests/criteria_checks.make_inputs at the golden shape (B = 2, C = 3, LR 5 x 7, scale 2, K = 10) and what the reference's
modules computed on them, term by term (the total of any combination is a sum of terms, F_model_depthCond.py:163-190):

    sr, hr, masks.<kind>         the inputs, fp32 (kind: onehot | soft | onehot_empty | soft_empty)
    pix.<crit>                   pixel_weight * cri_pix(sr, hr)                          crit: l1 | l2 | cb
    dyn.<kind>.<crit>            dynamic_weight_mask_loss(...)(sr, hr, masks)[2]          crit: l1 | l2 | smoothl1
    mask.<kind>.<crit>           mask_loss(...).get_mask_loss(sr, hr, masks) after np.random.seed(mask_seed)
    each with .value32 / .grad32 (the fp32 run: value, d value / d sr) and .value64 / .grad64 (the float64 run)
    mask_seed, mask_index        the seed and the region the reference drew with it
    pixel_weight, dynamic_weight, mask_weight

The '*_empty' kinds (one empty region) carry the l1 / l2 dynamic terms only: the reference's smoothl1 is 0/0 there, and the
static mask fixture draws a non-empty region, which is checked here.  The zip members carry a fixed date."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DASR_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "codes", "models", "modules", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, ROOT)
    import dasr_amd  # noqa: F401  (registers the package alias the tests import)
    from tests import criteria_checks as cc
    from tools.make_ssim_loss_golden import save
    ref_mask, ref_loss = _load("mask_loss"), _load("loss")
    torch.set_num_threads(1)
    s, K, terms = cc.golden_terms()
    W = cc.WEIGHTS
    pix = {"l1": torch.nn.L1Loss, "l2": torch.nn.MSELoss, "cb": ref_loss.CharbonnierLoss}
    arrays = dict(mask_seed=np.int64(cc.MASK_SEED), **{k: np.float64(v) for k, v in W.items()})
    sr, hr, _ = cc.make_inputs(s, K, "onehot")
    arrays["sr"], arrays["hr"] = sr.numpy(), hr.numpy()
    for kind in cc.GOLDEN_KINDS:
        assert all(torch.equal(a, b) for a, b in zip(cc.make_inputs(s, K, kind)[:2], (sr, hr)))
        arrays["masks." + kind] = cc.make_inputs(s, K, kind)[2].numpy()
    for name, (kind, _) in terms.items():
        what, crit = name.split(".")[0], name.split(".")[-1]
        masks = cc.make_inputs(s, K, kind or "onehot")[2]
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            x = sr.to(dtype).clone().requires_grad_(True)
            h, m = hr.to(dtype), masks.to(dtype)
            if what == "pix":
                v = W["pixel_weight"] * pix[crit]()(x, h)
            elif what == "dyn":
                mod = ref_mask.dynamic_weight_mask_loss(dict(dynamic_criterion=crit, dynamic_weight=W["dynamic_weight"]),
                                                        num_trainable_para=K).to(dtype)
                v = mod(x, h, m)[2]
            else:
                np.random.seed(cc.MASK_SEED)
                index = int(np.random.randint(0, K, 1)[0])
                np.random.seed(cc.MASK_SEED)
                assert float(masks[:, index].abs().sum()) > 0, "the static mask fixture must draw a non-empty region"
                arrays["mask_index"] = np.int64(index)
                v = ref_mask.mask_loss(dict(mask_criterion=crit, mask_weight=W["mask_weight"])).get_mask_loss(x, h, m)
            v.backward()
            assert torch.isfinite(v) and torch.isfinite(x.grad).all(), name
            arrays[name + ".value" + tag] = np.float64(v.item())
            arrays[name + ".grad" + tag] = x.grad.numpy()
        print(name, arrays[name + ".value32"], arrays[name + ".value64"])
    save("criteria", **arrays)


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
