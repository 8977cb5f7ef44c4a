#!/usr/bin/env python3
"""Generates tests/golden/phasenet_walk_grad.npz FROM THE REFERENCE ITSELF: loss and parameter gradients of the reference's
src/phase_net/phase_net.py `PhaseNet.forward` (eval mode, CPU, float64) on seeded weights and seeded normalised inputs.

Runs only in the build container (needs the reference checkout, VFI_REFERENCE).  The reference's phase_net.py is loaded and
run as it is; its one import, `src.train.utils.DecompValues`, is given as the namedtuple it is (utils.py itself pulls in image
libraries the forward never touches).  The fixture holds data only.

Weights: tests/phasenet_walk_ref.py `net_state(SEED)`; inputs: `seeded_inputs(SEED, 1, 12, 16, 10)` -- eight band levels, so the
last block serves two of them; targets: `walk_targets` around the reference's own outputs.  Stored: the inputs and targets
(float32 values), the loss at m = 8 and at m = 3, the full gradient of every bias / BatchNorm / head tensor, and for each
convolution weight its L2 norm and its dot product with a seeded vector (`probe`).

    python tests/golden/make_golden_phasenet_walk.py
"""
import collections
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import phasenet_walk_ref as W  # noqa: E402

REF = os.environ.get("VFI_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "phasenet_walk_grad.npz")
SEED, N, H, WD, HEIGHT = 11, 1, 12, 16, 10


def load_reference():
    values = collections.namedtuple("values", "high_level, phase, amplitude, low_level")
    for name in ("src", "src.train", "src.train.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["src.train.utils"].DecompValues = values
    spec = importlib.util.spec_from_file_location("reference_phase_net", os.path.join(REF, "src", "phase_net", "phase_net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, values


def main():
    ref, values = load_reference()
    net = ref.PhaseNet(types.SimpleNamespace(height=HEIGHT, nbands=4), "cpu").double()
    net.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in W.net_state(SEED).items()})
    net.eval()
    inp = W.seeded_inputs(SEED, N, H, WD, HEIGHT)
    d = W.to_dtype(inp)
    net.max_amplitudes, net.max_low_level = d["max_amp"], d["max_low"]
    vals = values(high_level=torch.zeros(inp["high_shape"], dtype=torch.float64), phase=d["phase"], amplitude=d["amp"],
                  low_level=d["low"])
    L = HEIGHT - 2

    def run(m):
        out = net(vals, m)
        return out.low_level, list(out.phase[::-1][:m]), list(out.amplitude[::-1][:m])       # coarsest first
    low, phases, amps = run(L)
    tgt = W.walk_targets(SEED + 1, low, phases, amps)
    t64 = W.to_dtype(tgt)
    loss = W.walk_loss(low, phases, amps, t64)
    net.zero_grad()
    loss.backward()
    low3, ph3, am3 = run(3)
    loss3 = W.walk_loss(low3, ph3, am3, {"low": t64["low"], "phase": t64["phase"][:3], "amp": t64["amp"][:3]})

    arrays = {"loss": np.float64(loss.detach()), "loss_m3": np.float64(loss3.detach()), "seed": np.int64(SEED),
              "shape": np.array([N, H, WD, HEIGHT]), "low": inp["low"].numpy(), "max_low": inp["max_low"].numpy(),
              "tgt_low": tgt["low"].numpy()}
    for i in range(L):
        arrays.update({f"phase{i}": inp["phase"][i].numpy(), f"amp{i}": inp["amp"][i].numpy(), f"max_amp{i}": inp["max_amp"][i].numpy(),
                       f"tgt_phase{i}": tgt["phase"][i].numpy(), f"tgt_amp{i}": tgt["amp"][i].numpy()})
    g = torch.Generator().manual_seed(SEED + 2)
    for k, p in net.named_parameters():
        if p.dim() == 4 and "prediction_map" not in k:
            probe = torch.randn(p.shape, generator=g, dtype=torch.float64)
            arrays["norm:" + k] = np.float64(p.grad.norm())
            arrays["dot:" + k] = np.float64((p.grad * probe).sum())
        else:
            arrays["grad:" + k] = p.grad.numpy()
    np.savez_compressed(OUT, **arrays)
    print(OUT, float(loss.detach()), float(loss3.detach()), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
