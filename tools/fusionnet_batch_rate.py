#!/usr/bin/env python3
"""Cost of FusionNet's training batch: `fusion_net_inputs` on B samples against B calls of
`FusionInterpolator` on the same pairs (which also run FusionNet itself), and one training step on its outputs.  Seeded
weights, HIP events around whole calls."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from oracle import pipeline_cpu  # noqa: E402
from vfi_amd.adacof.models import Model  # noqa: E402
from vfi_amd.fusion_net.fusion_net import FusionNet  # noqa: E402
from vfi_amd.fusion_net.interpolate_twoframe import FusionInterpolator  # noqa: E402
from vfi_amd.fusion_net.train_batch import fusion_net_inputs  # noqa: E402
from vfi_amd.phase_net.phase_net import PhaseNet  # noqa: E402
from vfi_amd.train.pyramid import Pyramid  # noqa: E402
from vfi_amd.train.utils import calc_pyr_height, preprocess  # noqa: E402


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, (h, w) = args.batch, args.size
    weights = pipeline_cpu.seeded_weights(0)
    adacof = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    adacof.load(weights["adacof"])
    adacof.eval()
    fusion = FusionNet().to(dev)
    fusion.load_state_dict(weights["fusionnet"])
    pyr = Pyramid(height=calc_pyr_height(torch.empty(3, h, w, device="meta")), nbands=4, scale_factor=np.sqrt(2), device=dev)
    phase_net = PhaseNet(pyr, dev, num_img=2)
    phase_net.load_state_dict(weights["phasenet"])
    g = torch.Generator().manual_seed(0)
    rgb1, rgb2, target = (torch.rand((b, 3, h, w), generator=g).to(dev) for _ in range(3))
    lab1, lab2 = preprocess(rgb1, dev), preprocess(rgb2, dev)
    fusion.eval()
    run = FusionInterpolator(adacof, fusion, weights["phasenet"], dev)
    t_one = timed(lambda: [run(rgb1[i], rgb2[i]) for i in range(b)], args.iters, 2)
    t_in = timed(lambda: fusion_net_inputs(adacof, phase_net, pyr, lab1, lab2, rgb1, rgb2), args.iters, 2)
    ins = fusion_net_inputs(adacof, phase_net, pyr, lab1, lab2, rgb1, rgb2)
    fusion.train(True)

    def step():
        fusion.zero_grad(set_to_none=True)
        torch.nn.functional.l1_loss(torch.clip(fusion(*ins, variant=0), 0, 1), target).backward()
    t_step = timed(step, args.iters, 2)
    print(f"FusionNet training batch, B = {b}, {h}x{w}")
    print(f"  {b} calls of FusionInterpolator (FusionNet included)   {t_one:9.3f} ms = {t_one / b:.3f} ms per sample")
    print(f"  fusion_net_inputs on the batch                        {t_in:9.3f} ms = {t_in / b:.3f} ms per sample")
    print(f"  FusionNet forward + L1 + backward on its outputs      {t_step:9.3f} ms")


if __name__ == "__main__":
    main()
