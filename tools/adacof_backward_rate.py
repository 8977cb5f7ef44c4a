#!/usr/bin/env python3
"""Rate of vfi_adacof_backward (all three gradients, one launch) at a 1080x1920 output, C = 3, offsets ~N(0, 2)
clipped to +-8 (the forward's measurement setup), for F = 5, d = 1 and F = 11, d = 2.  Timed with HIP events over
back-to-back launches; effective TB/s over the algorithmic bytes (the 3 F*F planes read, the 3 F*F planes written,
the C deltas; the frame gathers, served by the caches, are not counted)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from vfi_amd import _lib  # noqa: E402


def rate(f, dil, n=1, c=3, h=1080, w=1920, iters=20, warm=3):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(f)
    hin, win = h + (f - 1) * dil, w + (f - 1) * dil
    x = torch.rand((n, c, hin, win), generator=g).to(dev)
    wt = torch.softmax(torch.randn((n, f * f, h, w), generator=g), 1).to(dev)
    a = (torch.randn((n, f * f, h, w), generator=g) * 2).clamp(-8, 8).to(dev)
    b = (torch.randn((n, f * f, h, w), generator=g) * 2).clamp(-8, 8).to(dev)
    go = torch.randn((n, c, h, w), generator=g).to(dev)
    gw, ga, gb = (torch.empty_like(wt) for _ in range(3))
    d = _lib.dptr
    args = (d(go), d(x), d(wt), d(a), d(b), d(gw), d(ga), d(gb), n, c, hin, win, h, w, f, dil, _lib.stream_ptr())
    for _ in range(warm):
        _lib.call("vfi_adacof_backward", *args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _lib.call("vfi_adacof_backward", *args)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    byt = float(n) * h * w * (4 * c + 2 * 3 * f * f * 4)
    print(f"vfi_adacof_backward {h}x{w} C={c} F={f} d={dil}: {ms:.3f} ms  algorithmic {byt / 1e9:.2f} GB "
          f"-> {byt / ms / 1e9:.2f} TB/s", flush=True)
    return ms


if __name__ == "__main__":
    rate(5, 1)
    rate(11, 2)
