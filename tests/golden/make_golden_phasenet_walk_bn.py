#!/usr/bin/env python3
"""Generates tests/golden/phasenet_walk_bn.npz FROM THE REFERENCE ITSELF: loss, parameter gradients and running statistics of
the reference's src/phase_net/phase_net.py `PhaseNet.forward` in TRAINING mode (batch-statistics BatchNorm, as
src/train/trainer.py:107-134 runs it), CPU, float64, on seeded weights and seeded normalised inputs.

Runs only in the build container (needs the reference checkout, VFI_REFERENCE); no network access.  The reference's
phase_net.py is loaded and run as it is, the way make_golden_phasenet_walk.py does.  The fixture holds data only.

Weights: tests/phasenet_walk_ref.py `net_state(SEED)`; inputs: `seeded_inputs(SEED, 2, 12, 16, 10)` -- two samples, so the
statistics span the batch and the low level has more than one value per channel; eight band levels, so the last block
serves two of them.  Stored: the inputs and targets (float32 values), the loss at m = 8 and at m = 3 (each from freshly loaded
weights), the full gradient of every bias / BatchNorm / head tensor, for each convolution weight its L2 norm and its dot
product with a seeded vector, and every block's running_mean, running_var and num_batches_tracked after the one forward at
m = 8 (the momentum, the unbiased factor, and the two updates of the shared block).

    python tests/golden/make_golden_phasenet_walk_bn.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import phasenet_walk_ref as W  # noqa: E402
from make_golden_phasenet_walk import load_reference  # noqa: E402

OUT = os.path.join(HERE, "phasenet_walk_bn.npz")
SEED, N, H, WD, HEIGHT = 11, 2, 12, 16, 10


def main():
    ref, values = load_reference()
    inp = W.seeded_inputs(SEED, N, H, WD, HEIGHT)
    d = W.to_dtype(inp)
    vals = values(high_level=torch.zeros(inp["high_shape"], dtype=torch.float64), phase=d["phase"], amplitude=d["amp"],
                  low_level=d["low"])
    L = HEIGHT - 2

    def fresh():
        net = ref.PhaseNet(types.SimpleNamespace(height=HEIGHT, nbands=4), "cpu").double()
        net.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in W.net_state(SEED).items()})
        net.train()
        net.max_amplitudes, net.max_low_level = d["max_amp"], d["max_low"]
        return net

    def run(net, m):
        out = net(vals, m)
        return out.low_level, list(out.phase[::-1][:m]), list(out.amplitude[::-1][:m])       # coarsest first
    net = fresh()
    assert net.training and net.layers[0].feature_map[1].training
    low, phases, amps = run(net, L)
    tgt = W.walk_targets(SEED + 1, low, phases, amps)
    t64 = W.to_dtype(tgt)
    loss = W.walk_loss(low, phases, amps, t64)
    loss.backward()
    low3, ph3, am3 = run(fresh(), 3)
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
    for k, b in net.named_buffers():
        arrays["buffer:" + k] = b.detach().numpy()
    np.savez_compressed(OUT, **arrays)
    print(OUT, float(loss.detach()), float(loss3.detach()), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
