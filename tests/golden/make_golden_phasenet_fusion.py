#!/usr/bin/env python3
"""Generates tests/golden/phasenet_fusion_walk.npz FROM THE REFERENCE ITSELF: the outputs of the reference's
src/phase_net/phase_net.py `PhaseNet(pyr, device, num_img)` for num_img = 3 and 4 (eval mode, CPU, float64) on seeded weights and
seeded inputs -- normalize_vals, then forward at m = 8 and m = 3 -- and the results of its src/train/utils.py `separate_vals` /
`get_concat_layers_inf` for lists of three and four values on an integer-coded pyramid.

Runs only in the build container (needs the reference checkout, VFI_REFERENCE).  The reference's phase_net.py is loaded and run
as it is (its num_img == 3 branch prints; that output is dropped); utils.py imports after make_golden.py's empty placeholder
modules for packages its exercised functions never touch.  The fixture holds data only.

Weights: tests/phasenet_fusion_ref.py `net_state(SEED, num_img)`; inputs: `raw_inputs(SEED, 2, 12, 16, 10, num_img)` -- batch 2,
eight band levels from 3x3 to 12x16, so the last block serves two of them.  Stored per num_img: the raw inputs (float32 values),
the maxima, the normalised low level and coarsest band, every output at m = 8, the outputs at m = 3, and the state dict's key
names and shapes.

    python tests/golden/make_golden_phasenet_fusion.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import phasenet_fusion_ref as FR  # noqa: E402
from make_golden import REF, _placeholders  # noqa: E402

OUT = os.path.join(HERE, "phasenet_fusion_walk.npz")
SEED, N, H, WD, HEIGHT = 23, 2, 12, 16, 10


def load_reference():
    _placeholders()
    from src.train import utils as rutils
    spec = importlib.util.spec_from_file_location("reference_phase_net", os.path.join(REF, "src", "phase_net", "phase_net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, rutils


def walk_arrays(ref, rutils, num_img):
    pyr = types.SimpleNamespace(height=HEIGHT, nbands=4)
    net = ref.PhaseNet(pyr, "cpu", num_img=num_img).double()
    sd = FR.net_state(SEED, num_img)
    net.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()})
    net.eval()
    inp = FR.raw_inputs(SEED + num_img, N, H, WD, HEIGHT, num_img)
    d = FR.to_dtype(inp)
    vals = rutils.DecompValues(high_level=torch.zeros(inp["high_shape"], dtype=torch.float64), phase=d["phase"],
                               amplitude=d["amp"], low_level=d["low"])
    L = HEIGHT - 2
    t = f"n{num_img}_"
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        normed = net.normalize_vals(vals)
        out8, out3 = net(normed, L), net(normed, 3)
    arrays = {t + "low": inp["low"].numpy(), t + "max_low": net.max_low_level.numpy(), t + "norm_low": normed.low_level.numpy(),
              t + "norm_phase0": normed.phase[0].numpy(), t + "norm_amp0": normed.amplitude[0].numpy(),
              t + "out_low": out8.low_level.numpy(), t + "out_high": out8.high_level.numpy(), t + "m3_low": out3.low_level.numpy(),
              t + "keys": np.array(list(net.state_dict().keys())),
              t + "shapes": np.array([",".join(str(s) for s in v.shape) for v in net.state_dict().values()])}
    for i in range(L):          # inputs and maxima coarsest first (the network's order); outputs finest first (its result's)
        arrays.update({f"{t}phase{i}": inp["phase"][i].numpy(), f"{t}amp{i}": inp["amp"][i].numpy(),
                       f"{t}max_amp{i}": net.max_amplitudes[i].numpy(),
                       f"{t}out_phase{i}": out8.phase[i].numpy(), f"{t}out_amp{i}": out8.amplitude[i].numpy()})
    for i in range(L):
        if torch.is_tensor(out3.phase[i]):
            arrays.update({f"{t}m3_phase{i}": out3.phase[i].numpy(), f"{t}m3_amp{i}": out3.amplitude[i].numpy()})
        else:
            assert out3.phase[i] == 0 and out3.amplitude[i] == 0 and i < L - 3
    return arrays


def layout_arrays(rutils, num):
    """separate_vals / get_concat_layers_inf on a pyramid whose every element carries its own code (exact in float32)."""
    h, w, height = 8, 12, 5
    sizes = FR.W.level_sizes(h, w, height - 2)
    bands, low = sizes[:-1], sizes[-1]
    c = 3
    code = lambda n, a, b, base: (base + torch.arange(n * a * b, dtype=torch.float32).reshape(n, 1, a, b))
    vals = rutils.DecompValues(high_level=code(num * c, h, w, 1e5), low_level=code(num * c, *low, 2e5),
                               phase=[code(num * c * 4, a, b, 1e6 * (k + 1)) for k, (a, b) in enumerate(bands)],
                               amplitude=[code(num * c * 4, a, b, -1e6 * (k + 1)) for k, (a, b) in enumerate(bands)])
    lst = rutils.separate_vals(vals, num)
    cat = rutils.get_concat_layers_inf(types.SimpleNamespace(height=height, nbands=4), lst)
    t = f"layout{num}_"
    arrays = {t + "shape": np.array([h, w, height, c])}
    for name, v in [("vals_", vals), ("cat_", cat)] + [(f"sep{i}_", s) for i, s in enumerate(lst)]:
        arrays.update({t + name + "high": v.high_level.numpy(), t + name + "low": v.low_level.numpy()})
        for k in range(len(bands)):
            arrays.update({f"{t}{name}phase{k}": v.phase[k].numpy(), f"{t}{name}amp{k}": v.amplitude[k].numpy()})
    return arrays


def main():
    ref, rutils = load_reference()
    arrays = {"seed": np.int64(SEED), "shape": np.array([N, H, WD, HEIGHT])}
    for num_img in (3, 4):
        arrays.update(walk_arrays(ref, rutils, num_img))
        arrays.update(layout_arrays(rutils, num_img))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
