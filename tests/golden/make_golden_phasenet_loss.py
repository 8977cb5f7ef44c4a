#!/usr/bin/env python3
"""Generates tests/golden/phasenet_loss.npz FROM THE REFERENCE ITSELF: the three values `get_loss` of the reference's
src/train/loss.py:5-26 returns, in float64, on seeded inputs.

Runs only in the build container (needs the reference checkout, VFI_REFERENCE; loss.py needs only torch).  The reference's
file is loaded and run as it is.  The fixture holds data only: the inputs (float32 values) and the three results.

Inputs: two pyramid levels of phases, (2*4, 1, 5, 7) and (2*4, 1, 7, 10) (two images, four orientations), and an output /
target pair of (2, 3, 12, 16).  The target phases are phase_o + d with |wrap(d)| drawn from [0.05, pi - 0.05] and d shifted
by 2 pi k, k in {-1, 0, 1}, so neither the cut of atan2 at +-pi nor the kink of |.| at 0 is within reach of float32
rounding; the output - target differences are at least 0.01 in magnitude for the same reason.

    python tests/golden/make_golden_phasenet_loss.py
"""
import importlib.util
import math
import os
import types

import numpy as np
import torch

REF = os.environ.get("VFI_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "phasenet_loss.npz")


def main():
    spec = importlib.util.spec_from_file_location("reference_train_loss", os.path.join(REF, "src", "train", "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    g = torch.Generator().manual_seed(2025)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo
    sign = lambda shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    arrays = {}
    for i, shape in enumerate([(8, 1, 5, 7), (8, 1, 7, 10)]):
        phase_o = u(shape, -math.pi, math.pi).float()
        d = sign(shape) * u(shape, 0.05, math.pi - 0.05) + 2 * math.pi * (torch.randint(0, 3, shape, generator=g) - 1).double()
        arrays[f"phase_o{i}"] = phase_o
        arrays[f"phase_t{i}"] = (phase_o.double() + d).float()
    output = u((2, 3, 12, 16), 0.0, 1.0).float()
    arrays["output"] = output
    arrays["target"] = (output.double() + sign(output.shape) * u(output.shape, 0.01, 0.5)).float()

    d64 = {k: v.double() for k, v in arrays.items()}
    vals_o = types.SimpleNamespace(phase=[d64["phase_o0"], d64["phase_o1"]])
    vals_t = types.SimpleNamespace(phase=[d64["phase_t0"], d64["phase_t1"]])
    total, l_1_p, phase_loss_p = ref.get_loss(vals_o, vals_t, d64["output"], d64["target"], types.SimpleNamespace(nbands=4))
    np.savez_compressed(OUT, total_loss=np.float64(total), l_1_p=np.float64(l_1_p), phase_loss_p=np.float64(phase_loss_p),
                        weighting_factor=np.float64(0.005), nbands=np.int64(4), **{k: v.numpy() for k, v in arrays.items()})
    print(OUT, float(total), float(l_1_p), float(phase_loss_p), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
