#!/usr/bin/env python3
"""Generates tests/golden/phasenet_fusion_grad.npz FROM THE REFERENCE ITSELF: loss, parameter gradients and running statistics of
the reference's src/phase_net/phase_net.py `PhaseNet(pyr, device, num_img = 3 | 4).forward`, CPU, float64, in eval mode
(BatchNorm on its running statistics) and in training mode (batch statistics, as src/train/trainer.py:107-134 runs it), on
seeded weights and seeded normalised inputs.

Runs only in the build container (needs the reference checkout, VFI_REFERENCE); no network access.  The reference's
phase_net.py is loaded and run as it is, the way make_golden_phasenet_walk_bn.py does (its num_img == 3 branch prints; that
output is dropped).  The fixture holds data only.

Weights: tests/phasenet_fusion_ref.py `net_state(SEED, num_img)`; inputs: tests/phasenet_fusion_grad_ref.py
`seeded_inputs(SEED + num_img, 2, 12, 16, 10, num_img)` -- two samples, eight band levels from 3x3 to 12x16, so the last block
serves two of them.  Stored per num_img (prefix `n3_` / `n4_`) the inputs, and per mode (`eval_` / `train_`) the targets (a fixed
distance from that mode's outputs), the loss at m = 8 and at m = 3 (each from freshly loaded weights), the full gradient of every
bias / BatchNorm / head tensor, for each convolution weight its L2 norm and its dot product with a seeded vector, and every
block's running_mean, running_var and num_batches_tracked after the one forward at m = 8.

    python tests/golden/make_golden_phasenet_fusion_grad.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import phasenet_fusion_grad_ref as FG  # noqa: E402
import phasenet_fusion_ref as FR  # noqa: E402
import phasenet_walk_ref as W  # noqa: E402
from make_golden_phasenet_walk import load_reference  # noqa: E402

OUT = os.path.join(HERE, "phasenet_fusion_grad.npz")
SEED, N, H, WD, HEIGHT = 29, 2, 12, 16, 10


def arrays_for(ref, values, num_img):
    inp = FG.seeded_inputs(SEED + num_img, N, H, WD, HEIGHT, num_img)
    d = W.to_dtype(inp)
    vals = values(high_level=torch.zeros(inp["high_shape"], dtype=torch.float64), phase=d["phase"], amplitude=d["amp"],
                  low_level=d["low"])
    L = HEIGHT - 2
    t = f"n{num_img}_"
    arrays = {t + "low": inp["low"].numpy(), t + "max_low": inp["max_low"].numpy()}
    for i in range(L):
        arrays.update({f"{t}phase{i}": inp["phase"][i].numpy(), f"{t}amp{i}": inp["amp"][i].numpy(),
                       f"{t}max_amp{i}": inp["max_amp"][i].numpy()})

    def fresh(train):
        net = ref.PhaseNet(types.SimpleNamespace(height=HEIGHT, nbands=4), "cpu", num_img=num_img).double()
        net.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in FR.net_state(SEED, num_img).items()})
        net.train(train)
        assert net.layers[0].feature_map[1].training == train
        net.max_amplitudes, net.max_low_level = d["max_amp"], d["max_low"]
        return net

    def run(net, m):
        with contextlib.redirect_stdout(io.StringIO()):
            out = net(vals, m)
        return out.low_level, list(out.phase[::-1][:m]), list(out.amplitude[::-1][:m])       # coarsest first

    for mode, train in (("eval_", False), ("train_", True)):
        p = t + mode
        net = fresh(train)
        low, phases, amps = run(net, L)
        tgt = W.walk_targets(SEED + 1 + num_img + 10 * train, low, phases, amps)
        t64 = W.to_dtype(tgt)
        loss = W.walk_loss(low, phases, amps, t64)
        loss.backward()
        low3, ph3, am3 = run(fresh(train), 3)
        loss3 = W.walk_loss(low3, ph3, am3, {"low": t64["low"], "phase": t64["phase"][:3], "amp": t64["amp"][:3]})
        arrays.update({p + "loss": np.float64(loss.detach()), p + "loss_m3": np.float64(loss3.detach()),
                       p + "tgt_low": tgt["low"].numpy()})
        for i in range(L):
            arrays.update({f"{p}tgt_phase{i}": tgt["phase"][i].numpy(), f"{p}tgt_amp{i}": tgt["amp"][i].numpy()})
        g = torch.Generator().manual_seed(SEED + 2)
        for k, q in net.named_parameters():
            if q.dim() == 4 and "prediction_map" not in k:
                probe = torch.randn(q.shape, generator=g, dtype=torch.float64)
                arrays[p + "norm:" + k] = np.float64(q.grad.norm())
                arrays[p + "dot:" + k] = np.float64((q.grad * probe).sum())
            else:
                arrays[p + "grad:" + k] = q.grad.numpy()
        for k, b in net.named_buffers():
            arrays[p + "buffer:" + k] = b.detach().numpy()
    return arrays


def main():
    ref, values = load_reference()
    arrays = {"seed": np.int64(SEED), "shape": np.array([N, H, WD, HEIGHT])}
    for num_img in (3, 4):
        arrays.update(arrays_for(ref, values, num_img))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
