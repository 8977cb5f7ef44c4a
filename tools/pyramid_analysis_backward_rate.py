#!/usr/bin/env python3
"""Time of vfi_pyr_analyze_backward (the gradient of Pyramid.filter / SCFpyr_PyTorch.build with respect to the image:
every band level's (d phase, d amplitude) or complex coefficient gradient, d high, d low) for N = 3 images at 256x256,
720p and 1080p, next to vfi_pyr_synthesize of the same N and size, whose passes it runs.

Timing: HIP events around back-to-back calls on one stream, every shape warmed up first, each window sized to at least
0.3 s of device work, and the three calls alternated over several rounds in one process; the table gives each call's
median and the spread (min .. max) of its rounds.  Needs a HIP device: there is no CPU path."""
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from oracle import layout_cpu  # noqa: E402
from vfi_amd.steerable.SCFpyr_PyTorch import BAND_MAJOR, COMPLEX_COEFF, SCFpyr_PyTorch  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rate(h, w, n=3, rounds=5, min_window_ms=300.0):
    dev = torch.device("cuda:0")
    height = layout_cpu.calc_pyr_height(h, w)
    nlev, nb = height - 2, 4
    plan = SCFpyr_PyTorch(height, nb, math.sqrt(2), dev).plan(h, w, n)
    mask = (1 << nlev) - 1
    g = torch.Generator(device="cpu").manual_seed(h)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    randn = lambda t: torch.randn(t.shape, generator=g).to(dev)
    img = torch.rand((n, h, w), generator=g).to(dev)
    hi, lo = new(n, 1, h, w), new(n, 1, *plan.sizes[nlev])
    phase = [new(n * nb, 1, *plan.sizes[k]) for k in range(nlev)]
    amp = [new(n * nb, 1, *plan.sizes[k]) for k in range(nlev)]
    plan.analyze(img, hi, phase, amp, None, lo, 1.0, mask, 0)
    gh, gl = randn(hi), randn(lo)
    gp, ga = [randn(p) for p in phase], [randn(a) for a in amp]
    gc = [randn(new(nb, n, *plan.sizes[k], 2)) for k in range(nlev)]
    out = new(n, h, w)
    calls = {
        "synthesis": lambda: plan.synthesize(hi, phase, amp, None, lo, mask, 0, out),
        "backward (phase, amplitude)": lambda: plan.analyze_backward(gh, gp, ga, phase, amp, None, gl, 1.0, mask, 0, out),
        "backward (complex)": lambda: plan.analyze_backward(gh, gc, None, None, None, None, gl, 1.0, mask, BAND_MAJOR | COMPLEX_COEFF, out),
    }
    iters = {}
    for name, fn in calls.items():      # warm up (the first backward builds the plan's tables), then size the window
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(10, int(math.ceil(min_window_ms / max(window(fn, 10), 1e-3))))
    times = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, iters[name]))
    med = {name: statistics.median(t) for name, t in times.items()}
    cells = "  ".join(f"{name} {med[name]:.3f} ms ({min(t):.3f} .. {max(t):.3f})" for name, t in times.items())
    print(f"{h}x{w} N={n} height={height}: {cells}  polar / synthesis {med['backward (phase, amplitude)'] / med['synthesis']:.2f}  "
          f"complex / synthesis {med['backward (complex)'] / med['synthesis']:.2f}", flush=True)
    return med


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("pyramid_analysis_backward_rate: no HIP device")
    for size in [(256, 256), (720, 1280), (1080, 1920)]:
        rate(*size)
