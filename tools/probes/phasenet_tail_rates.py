"""Probe: vfi_phasenet_level_tail against vfi_phasenet_predict + vfi_resize_bilinear at the 1080p level pairs (N = 3), isolated
launches: time of both and the achieved rate of the new one (profiles/r06_phasenet_tail.txt)."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from vfi_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")


def size(d, k):
    return int(math.ceil(d / math.sqrt(2.0) ** k - 1e-9))


def timed(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


n = 3
pc = ops.PackedConv(torch.randn((8, 64, 1, 1)) / 8.0, torch.randn((8,)) * 0.1, device=dev)
mx = (torch.rand((n,)) + 0.5).to(dev)
tot_old = tot_new = 0.0
for k in range(1, 10):
    h, w, ho, wo = size(1080, k), size(1920, k), size(1080, k - 1), size(1920, k - 1)
    fp = torch.randn((n, 72, h, w), device=dev)
    x = torch.rand((n, 88, h, w), device=dev)
    xn = torch.empty((n, 88, ho, wo), device=dev)
    amp_in = x[:, 80:]
    p, a = torch.empty((n * 4, 1, h, w), device=dev), torch.empty((n * 4, 1, h, w), device=dev)

    def old():
        _lib.call("vfi_phasenet_predict", fp.data_ptr(), fp.stride(0), pc.packed.data_ptr(), pc.bias.data_ptr(), amp_in.data_ptr(), x.stride(0),
                  mx.data_ptr(), fp[:, 64:].data_ptr(), fp.stride(0), p.data_ptr(), a.data_ptr(), n, 64, h, w, _lib.stream_ptr())
        ops.resize_bilinear(fp, (ho, wo), align_corners=False, out=xn[:, :72])

    def new():
        ops.phasenet_level_tail(fp, pc, amp_in, mx, xn[:, :72])

    t_old, t_new = timed(old), timed(new)
    tot_old += t_old
    tot_new += t_new
    byts = 4.0 * n * ((64 + 8 + 8) * h * w + 72 * ho * wo)
    print(f"{h}x{w} -> {ho}x{wo}: old {t_old * 1e3:.1f} us  new {t_new * 1e3:.1f} us  new {byts / t_new * 1e-6:.0f} GB/s", flush=True)
print(f"sum: old {tot_old:.3f} ms  new {tot_new:.3f} ms")
