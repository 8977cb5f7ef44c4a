#!/usr/bin/env python3
"""Optimiser step rates: vfi_amd.optim's SGD (momentum 0.9), Adam, Adamax and RMSprop next to
torch.optim's default step, and its fused=True step where torch has one (Adam, SGD), on two parameter sets: the AdaCoF
network's and the GAN discriminator's at patch 256 (one 134 M element matrix and a few small tensors).

All optimisers of a kind step the SAME parameter and gradient tensors (each keeps its own state), alternating within every
repeat, so a drift of the clock or a neighbour on the machine moves them together.  One sample is a window of `--steps`
steps between two HIP events, host work included (a step is what the trainer waits for).  Every window starts on an idle
queue (a synchronise in front of it: no path hides its enqueueing behind the previous path's kernels) and the order of the
paths rotates from repeat to repeat; `--repeats` samples after `--warmup` untimed steps; printed: the median ms per step,
the spread (min .. max), and for every path the effective TB/s over the algorithmic bytes of one fused pass (read p, g and the state, write p and the state: 28 B per element for Adam and
Adamax, 20 B for RMSprop and SGD with momentum), to be read against the copy rate of profiles/r04_hbm_rates.txt
(4.75-5.3 TB/s)."""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from vfi_amd import optim  # noqa: E402

KINDS = {"SGD": (dict(lr=1e-3, momentum=0.9), 20, True), "Adam": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), 28, True),
         "Adamax": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), 28, False), "RMSprop": (dict(lr=1e-3, eps=1e-8), 20, False)}


def shapes_of(which):
    if which == "adacof":
        from vfi_amd.adacof.models.adacofnet import AdaCoFNet
        net = AdaCoFNet(types.SimpleNamespace(kernel_size=5, dilation=1, gpu_id=0))
    else:
        from vfi_amd.adacof.losses.discriminator import Discriminator
        net = Discriminator(types.SimpleNamespace(patch_size=256), "GAN")
    return [tuple(p.shape) for p in net.parameters() if p.requires_grad]


def window(opt, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def measure(shapes, steps, repeats, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    params = [(torch.randn(s, device=dev, generator=g) * 0.05).requires_grad_(True) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    numel = sum(p.numel() for p in params)
    for kind, (kw, bytes_per, has_fused) in KINDS.items():
        paths = {"device": getattr(optim, kind)(params, **kw), "torch": getattr(torch.optim, kind)(params, **kw)}
        if has_fused:
            paths["torch fused"] = getattr(torch.optim, kind)(params, fused=True, **kw)
        for _ in range(warmup):
            for opt in paths.values():
                opt.step()
        torch.cuda.synchronize()
        samples = {name: [] for name in paths}
        names = list(paths)
        for r in range(repeats):
            for name in names[r % len(names):] + names[:r % len(names)]:
                samples[name].append(window(paths[name], steps))
        for name, ms in samples.items():
            med = statistics.median(ms)
            print(f"    {kind:8s} {name:12s} {med:8.4f} ms / step  ({min(ms):.4f} .. {max(ms):.4f})  "
                  f"{bytes_per * numel / med * 1e-9:5.2f} TB/s effective")
        del paths
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=100, help="steps per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", nargs="+", default=("adacof", "discriminator"), choices=("adacof", "discriminator"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_rate.py needs a HIP device: a CPU run gives no rate")
    dev = torch.device("cuda:0")
    for which in a.sets:
        shapes = shapes_of(which)
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        print(f"{which}: {len(shapes)} tensors, {n / 1e6:.1f} M parameters, {a.steps} steps per window, {a.repeats} repeats")
        measure(shapes, a.steps, a.repeats, a.warmup, dev)


if __name__ == "__main__":
    main()
