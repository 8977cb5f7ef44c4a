#!/usr/bin/env python3
"""LPIPS cost: the metric at the evaluation crop (1 x 512 x 512, no grad), one loss step at the
training shape (batch 4, 256 x 256: forward, backward to the image), and the head alone at the five tap shapes of a
512 x 512 crop -- forward and backward entry, the bytes each moves once (both maps read; the gradient and `above` besides)
and the rate that makes -- beside the same head composed from torch ops on the same device.

`--vgg-weights` / `--lpips-weights` take the pretrained files; without them seeded weights are used (the time does not
depend on the values)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
from vfi_amd import ops, vgg16  # noqa: E402
from vfi_amd.evaluation import lpips  # noqa: E402


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


def seeded_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, idx in enumerate(vgg16.CONV_INDICES):
        cin, cout = vgg16.CHANNELS[i], vgg16.CHANNELS[i + 1]
        sd[f"features.{idx}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn((cout,), generator=g) * 0.05
    return sd, [torch.rand((c,), generator=g) for c in lpips.TAP_CHANNELS]


def main(vgg_weights=None, lpips_weights=None, iters=10, warm=3):
    dev = torch.device("cuda:0")
    sd, heads = seeded_weights()
    net = lpips.LPIPS(vgg_weights or sd, lpips_weights or heads).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    pair = lambda b, s: tuple(torch.rand((b, 3, s, s), generator=g).to(dev) for _ in range(2))

    x, y = pair(1, 512)
    with torch.no_grad():
        t = timed(lambda: net(x, y), iters, warm)
    print(f"metric, 1 x 3 x 512 x 512, no grad: {t:8.3f} ms")

    x, y = pair(4, 256)
    x.requires_grad_(True)
    t_f = timed(lambda: net(x, y), iters, warm)

    def step():
        x.grad = None
        net(x, y).mean().backward()
    t_s = timed(step, iters, warm)
    print(f"loss step, 4 x 3 x 256 x 256: forward {t_f:8.3f} ms, backward to the image {t_s - t_f:8.3f} ms")

    print("the head alone at the taps of a 512 x 512 crop (N = 1): HIP entry | torch ops")
    for c, s in zip(lpips.TAP_CHANNELS, (512, 256, 128, 64, 32)):
        a, b = (torch.relu(torch.randn((1, c, s, s), generator=g)).to(dev) for _ in range(2))
        w = torch.rand((c,), generator=g).to(dev)
        up = torch.ones(1, device=dev)
        above = torch.randn((1, c, s, s), generator=g).to(dev)
        out = torch.empty_like(a)
        mb = a.numel() * 4 / 2 ** 20
        t_hf = timed(lambda: ops.lpips_head_forward(a, b, w), iters, warm)
        t_hb = timed(lambda: ops.lpips_head_backward(a, b, w, up, above=above, out=out), iters, warm)
        ag = a.clone().requires_grad_(True)
        with torch.no_grad():
            t_tf = timed(lambda: lpips.head_torch(a, b, w), iters, warm)

        def tstep():
            ag.grad = None
            v = lpips.head_torch(ag, b, w)
            v.backward(up)
            return (ag.grad + above) * (ag > 0)
        t_ts = timed(tstep, iters, warm)
        print(f"  C={c:3d} {s:3d}x{s:<3d} forward {t_hf * 1e3:7.1f} us ({2 * mb:6.1f} MiB, {2 * mb / 2 ** 20 / (t_hf * 1e-3):5.2f} TiB/s) | "
              f"{t_tf * 1e3:8.1f} us;  backward {t_hb * 1e3:7.1f} us ({4 * mb:6.1f} MiB, {4 * mb / 2 ** 20 / (t_hb * 1e-3):5.2f} TiB/s) | "
              f"forward + backward {t_ts * 1e3:8.1f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vgg-weights", default=None, help="torchvision vgg16 state dict (default: seeded weights)")
    ap.add_argument("--lpips-weights", default=None, help="LPIPS head weights (default: seeded weights)")
    a = ap.parse_args()
    main(a.vgg_weights, a.lpips_weights)
