#!/usr/bin/env python3
"""Generates tests/golden/adacofnet_smoothness.npz FROM THE REFERENCE ITSELF: g_Spatial and g_Occlusion as the training
branch of the reference's AdaCoFNet.forward computes them (src/adacof/models/adacofnet.py:202-217, CharbonnierFunc of
src/adacof/utility.py:67-68), in float64, on seeded maps.

Runs only in the build container (needs the reference checkout, VFI_REFERENCE).  The reference's forward is run as it is:
an AdaCoFNet object is made without its constructor, its kernel estimator is replaced by a stub that returns the seeded
maps and its sampler by one that returns seeded sides, and `cupy` (imported by the reference's sampler module, unused
here) is stubbed.  The fixture holds data only: the maps (float32 values), the two terms and frame1.

    python tests/golden/make_golden_adacofnet_smoothness.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("VFI_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adacofnet_smoothness.npz")


def main():
    sys.path.insert(0, REF)
    if "cupy" not in sys.modules:      # the sampler module decorates a launcher with cupy.memoize at import
        stub = types.ModuleType("cupy")
        stub.memoize = lambda **kw: (lambda fn: fn)
        sys.modules["cupy"] = stub
    from src.adacof.models import adacofnet as ref

    g = torch.Generator().manual_seed(2024)
    n, f2, h, w = 1, 9, 32, 64
    r32 = lambda *s: torch.randn(s, generator=g).float()
    maps = {}
    for side in "12":
        maps["w" + side] = torch.softmax(r32(n, f2, h, w) * 2, 1)
        maps["a" + side] = r32(n, f2, h, w) * 3
        maps["b" + side] = r32(n, f2, h, w) * 3
    maps["occ"] = torch.sigmoid(r32(n, 1, h, w) * 2)
    sides = [torch.rand((n, 3, h, w), generator=g).float() for _ in range(2)]
    d = {k: v.double() for k, v in maps.items()}

    net = object.__new__(ref.AdaCoFNet)
    torch.nn.Module.__init__(net)
    net.kernel_size, net.kernel_pad, net.dilation = 3, 1, 1
    net.get_kernel = lambda f0, f2_: (d["w1"], d["a1"], d["b1"], d["w2"], d["a2"], d["b2"], d["occ"])
    net.modulePad = lambda x: x
    it = iter(sides)
    net.moduleAdaCoF = lambda *a: next(it).double()
    net.train(True)
    frames = torch.zeros((n, 3, h, w), dtype=torch.float64)
    out = net(frames, frames)
    np.savez_compressed(OUT, t1=sides[0].numpy(), t2=sides[1].numpy(), frame1=out["frame1"].numpy(),
                        g_Spatial=np.float64(out["g_Spatial"]), g_Occlusion=np.float64(out["g_Occlusion"]),
                        **{k: v.numpy() for k, v in maps.items()})
    print(OUT, float(out["g_Spatial"]), float(out["g_Occlusion"]), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
