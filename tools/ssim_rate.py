#!/usr/bin/env python3
"""SSIM-loss cost: `SSIMLoss` forward (no grad) and forward + backward to the prediction at the
trainers' crop (4 x 3 x 256 x 256) and at one 1080p frame (1 x 3 x 1080 x 1920, pooled by 4), beside (a) the unfused
sequence of `evaluate_image.ssim`, forward only, image by image, and (b) the same formula from torch ops with torch
autograd on the same device.  The two entries alone are timed as well, with the bytes each moves once (x and y read; the
gradient written besides) and the rate that makes.  HIP events, 10 iterations after 3."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from vfi_amd import ops  # noqa: E402
from vfi_amd.evaluation import evaluate_image as ei  # noqa: E402
from vfi_amd.evaluation import ssim as ssim_mod  # noqa: E402


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
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds


def main(iters=10, warm=3):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    crit = ssim_mod.SSIMLoss()
    for shape in ((4, 3, 256, 256), (1, 3, 1080, 1920)):
        x = torch.rand(shape, generator=g).to(dev)
        y = (x + 0.05 * torch.randn(shape, generator=g).to(dev)).clamp(0, 1)
        f = ssim_mod.pool_factor(*shape[2:])
        xg = x.clone().requires_grad_(True)

        def step():
            xg.grad = None
            crit(xg, y).backward()

        def torch_step():
            xg.grad = None
            (1 - ssim_mod.ssim_torch(xg, y)).mean().backward()

        with torch.no_grad():
            t_f = timed(lambda: crit(x, y), iters, warm)
            t_a = timed(lambda: [ei.ssim(x[i], y[i]) for i in range(shape[0])], iters, warm)
            t_tf = timed(lambda: (1 - ssim_mod.ssim_torch(x, y)).mean(), iters, warm)
        t_s = timed(step, iters, warm)
        t_ts = timed(torch_step, iters, warm)
        print(f"{'x'.join(map(str, shape))} (f = {f}): SSIMLoss forward {t_f:8.1f} us, forward + backward {t_s:8.1f} us | "
              f"(a) evaluate_image.ssim, {shape[0]} image(s) {t_a:8.1f} us | (b) torch ops forward {t_tf:8.1f} us, "
              f"forward + backward {t_ts:8.1f} us")

        # the entries alone, on what they are given (the pooled images when f > 1)
        xp, yp = (ops.avg_pool(x, f), ops.avg_pool(y, f)) if f > 1 else (x, y)
        up = torch.ones(shape[0], device=dev)
        out = torch.empty_like(xp)
        mib = xp.numel() * 4 / 2 ** 20
        t_ef = timed(lambda: ops.ssim_loss_forward(xp, yp), iters, warm)
        t_eb = timed(lambda: ops.ssim_loss_backward(xp, yp, up, out=out), iters, warm)
        print(f"  entries on {'x'.join(map(str, xp.shape))}: forward {t_ef:7.1f} us ({2 * mib:6.2f} MiB, "
              f"{2 * mib / 2 ** 20 / (t_ef * 1e-6):5.3f} TiB/s), backward {t_eb:7.1f} us ({3 * mib:6.2f} MiB, "
              f"{3 * mib / 2 ** 20 / (t_eb * 1e-6):5.3f} TiB/s)")
        if f > 1:
            gp = torch.empty_like(xp)
            t_p = timed(lambda: ops.avg_pool(x, f), iters, warm)
            t_pb = timed(lambda: ops.avg_pool_backward(gp, shape[2:], f), iters, warm)
            print(f"  pooling by {f}: avg_pool {t_p:7.1f} us per image pair half, avg_pool_backward {t_pb:7.1f} us "
                  f"({(x.numel() + xp.numel()) * 4 / 2 ** 20:6.2f} MiB each)")


    # enough work to leave the launch latency behind: what the two kernels sustain
    xp = torch.rand((32, 3, 256, 256), generator=g).to(dev)
    yp = (xp + 0.05 * torch.randn(xp.shape, generator=g).to(dev)).clamp(0, 1)
    up, out, mib = torch.ones(32, device=dev), torch.empty_like(xp), xp.numel() * 4 / 2 ** 20
    t_ef = timed(lambda: ops.ssim_loss_forward(xp, yp), iters, warm)
    t_eb = timed(lambda: ops.ssim_loss_backward(xp, yp, up, out=out), iters, warm)
    print(f"  entries on 32x3x256x256: forward {t_ef:7.1f} us ({2 * mib:6.2f} MiB, {2 * mib / 2 ** 20 / (t_ef * 1e-6):5.3f} TiB/s), "
          f"backward {t_eb:7.1f} us ({3 * mib:6.2f} MiB, {3 * mib / 2 ** 20 / (t_eb * 1e-6):5.3f} TiB/s)")


if __name__ == "__main__":
    main()
