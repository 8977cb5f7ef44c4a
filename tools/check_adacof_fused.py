#!/usr/bin/env python3
"""Development aid: every case of tests/adacof_fused_ref.py (planar, rgbx, rgbx + logits) against the float64 reference.

The kernel choice of `vfi_adacof_fused` / `vfi_adacof_fused_rgbx` depends on VFI_ADACOF_VARIANT and VFI_ADACOF_MARGIN, which
the library reads once per process: run this in a fresh process per setting.  One `ok` / `FAIL` line per case and mode, then
`worst abs error` (t1, t2, frame); the exit status is 1 if any case fails a bound or has a non-finite output."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
import torch

import adacof_fused_ref as R

dev = torch.device("cuda:0")
print("VFI_ADACOF_VARIANT =", os.environ.get("VFI_ADACOF_VARIANT"), " VFI_ADACOF_MARGIN =", os.environ.get("VFI_ADACOF_MARGIN"))
worst, fails = 0.0, 0
for case in R.CASES:
    for mode, img, excess, merr, finite in R.run_case(case, dev):
        good = R.passes(img, excess, finite)
        if not finite or not img <= worst:          # (max() would drop a NaN)
            worst = img if finite else float("inf")
        fails += not good
        print("ok  " if good else "FAIL", R.case_id(case), mode, f"images {img:.2e} mask {merr:.2e} (excess {excess:.2e})",
              "" if finite else "non-finite output")
print("cases done, worst abs error", worst)
sys.exit(1 if fails else 0)
