#!/usr/bin/env python3
"""Cost of PhaseNet with three and four input images on 1080x1920 Lab frames (N = 3 colours): a band
level's head at the finest level's shape -- vfi_phasenet_predict_n in one pass against the two-launch composition
(vfi_conv2d(tanh) + vfi_phasenet_emit_n), in the same run, next to the two-image head -- and the whole inference forward of
the coarse-to-fine walk for num_img = 2, 3 and 4.  Per-call HIP events."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
import phasenet_fusion_ref as FR  # noqa: E402
from vfi_amd import ops  # noqa: E402
from vfi_amd.phase_net.core import PhaseNetCore  # noqa: E402
from vfi_amd.train.pyramid import Pyramid  # noqa: E402
from vfi_amd.train.utils import calc_pyr_height  # noqa: E402


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


def head(h, w, num_img, n=3, iters=20, warm=5):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(num_img)
    p = FR.pred_channels(num_img)[1]
    fp = torch.randn((n, 64 + p, h, w), generator=g).to(dev)
    x = torch.rand((n, 64 + p + 8 * num_img, h, w), generator=g).to(dev)
    amp_in, mx = x[:, 64 + p + 4 * num_img:], torch.ones(n, device=dev)
    pc = ops.PackedConv(torch.randn((p, 64, 1, 1), generator=g) / 8.0, torch.randn((p,), generator=g) * 0.1, device=dev)
    t_one = timed(lambda: ops.phasenet_predict_n(fp[:, :64], pc, amp_in, mx, num_img, pred=fp[:, 64:]), iters, warm)

    def composed():
        ops.conv2d(fp[:, :64], pc, "zeros", "tanh", out=fp[:, 64:])
        ops.phasenet_emit_n(fp[:, 64:], amp_in, mx, num_img)
    t_two = timed(composed, iters, warm)
    planes = 64 + p + 8 + (12 if num_img == 3 else 8)         # features and blended amplitudes read; pred, phase, amp written
    print(f"head, num_img={num_img} N={n} {h}x{w}: one pass {t_one:.3f} ms ({4e-9 * n * h * w * planes / (t_one * 1e-3):.0f} GB/s of "
          f"{planes} planes), conv + emit_n {t_two:.3f} ms, ratio {t_two / t_one:.2f}")
    return t_one


def forward(h, w, num_img, n=3, iters=5, warm=2):
    dev = torch.device("cuda:0")
    height = calc_pyr_height(torch.empty(1, h, w))
    core = PhaseNetCore(height, dev, num_img=num_img)
    core.load_state_dict(FR.net_state(0, num_img))
    pyr = Pyramid(height=height, nbands=4, scale_factor=math.sqrt(2), device=dev)
    imgs = torch.rand((num_img * n, h, w), generator=torch.Generator().manual_seed(1)).to(dev)
    vals, bufs = pyr.filter(imgs, concat_frames=num_img, phase_scale=1.0 / math.pi, pred_channels=core.pred_channels)
    nv = core.normalize_vals(vals, concat=bufs)
    del pyr
    with torch.no_grad():
        t = timed(lambda: core(nv), iters, warm)
    print(f"PhaseNet forward, num_img={num_img} N={n} {h}x{w}, height {height}: {t:.3f} ms")
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    args = ap.parse_args()
    h, w = args.size
    t_head = {k: head(h, w, k) for k in (2, 3, 4)}
    print(f"head one pass: num_img=3 / num_img=2 = {t_head[3] / t_head[2]:.3f} (planes moved: 96 / 88 = {96 / 88:.3f}; read alone: "
          f"76 / 72 = {76 / 72:.3f}), num_img=4 / num_img=2 = {t_head[4] / t_head[2]:.3f}")
    torch.cuda.empty_cache()
    t_fwd = {}
    for k in (2, 3, 4):
        t_fwd[k] = forward(h, w, k)
        torch.cuda.empty_cache()
    print(f"forward: num_img=3 / num_img=2 = {t_fwd[3] / t_fwd[2]:.3f}, num_img=4 / num_img=2 = {t_fwd[4] / t_fwd[2]:.3f}")


if __name__ == "__main__":
    main()
