#!/usr/bin/env python3
"""Y4M-inclusive clip rate at 1080p (read + H2D + decode + interpolate + encode + D2H + write), the counterpart of
clip_io_rate.py for vfi_amd.fusion_net.interpolate_stream.  With --kernels also the two conversion
kernels alone: time per call and effective TB/s over the bytes they move.

usage: clip_stream_rate.py [frames=13] [frames_in_flight=2] [--kernels]"""
import os
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
import bench  # noqa: E402
from vfi_amd import ops  # noqa: E402
from vfi_amd.fusion_net import interpolate_stream as st  # noqa: E402

H, W = 1080, 1920
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(argv[0]) if len(argv) > 0 else 13
fif = int(argv[1]) if len(argv) > 1 else 2
dev = torch.device("cuda:0")
fmt = (ops.YUV_420, ops.YUV_SITING_CENTRE, ops.YUV_BT709, ops.YUV_LIMITED)


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


if "--kernels" in sys.argv:
    # rotate over enough buffers that no call finds its bytes in the 256 MiB Infinity Cache
    sets = 24
    rgbs = [torch.rand((3, H, W), device=dev) for _ in range(sets)]
    frames = [ops.rgb_to_yuv(x, fmt) for x in rgbs]
    labs = [torch.empty((6, H, W), device=dev) for _ in range(sets)]
    labs2 = [torch.empty((6, H, W), device=dev) for _ in range(sets)]
    nb, plane = frames[0].numel(), 12 * H * W
    it = [0]

    def nxt():
        it[0] = (it[0] + 1) % sets
        return it[0]
    for name, outs, fn in (
            ("yuv_to_rgb rgb", 1, lambda i: ops.yuv_to_rgb(frames[i], H, W, fmt, rgb=rgbs[i])),
            ("yuv_to_rgb rgb+lab", 2, lambda i: ops.yuv_to_rgb(frames[i], H, W, fmt, rgb=rgbs[i], lab=(labs[i][:3], None))),
            ("yuv_to_rgb rgb+lab+lab", 3, lambda i: ops.yuv_to_rgb(frames[i], H, W, fmt, rgb=rgbs[i], lab=(labs[i][:3], labs2[i][3:]))),
            ("rgb_to_yuv", 1, lambda i: ops.rgb_to_yuv(rgbs[i], fmt, out=frames[i]))):
        sec = timed(lambda: fn(nxt()))
        moved = nb + outs * plane
        print(f"  {name:24s} {W}x{H} 4:2:0  {sec * 1e6:7.1f} us  {moved / 1e6:6.1f} MB  {moved / sec * 1e-12:5.2f} TB/s")
    # a plain device copy of the decoder's largest traffic (read + write counted), as the yardstick of the same run
    bufs = [(torch.empty(3 * plane // 8, device=dev), torch.empty(3 * plane // 8, device=dev)) for _ in range(sets)]
    sec = timed(lambda: (lambda p: p[1].copy_(p[0]))(bufs[nxt()]))
    print(f"  {'plain copy (torch)':24s} {W}x{H}        {sec * 1e6:7.1f} us  {3 * plane / 1e6:6.1f} MB  {3 * plane / sec * 1e-12:5.2f} TB/s")
    sys.exit(0)

runners, _ = bench.build_runner(dev, fif)
with tempfile.TemporaryDirectory() as td:
    path, out = os.path.join(td, "in.y4m"), os.path.join(td, "out.y4m")
    pairs = bench.synthetic_pairs(1, H, W, dev)
    base = pairs[0][0]
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420jpeg\n".encode())
        for i in range(n):
            f.write(b"FRAME\n")
            f.write(ops.rgb_to_yuv(torch.roll(base, 3 * i, dims=2), fmt).cpu().numpy().tobytes())
    args = types.SimpleNamespace(gpu_id=0, matrix="bt709", range="limited", keep_rate=False)

    def run():
        with open(path, "rb") as s, open(out, "wb") as d:
            return st.interpolate_stream(args, s, d, runners=runners, frames_in_flight=fif)
    run()                                                             # warm-up (plans, packed weights)
    t0 = time.perf_counter()
    done = run()
    dt = time.perf_counter() - t0
    assert os.path.getsize(out) > (2 * n - 1) * W * H * 3 // 2
    print(f"clip of {n} frames at {W}x{H} from/to Y4M: {done} interpolated frames in {dt:.2f} s = {done / dt:.2f} frames/s "
          f"({fif} frames in flight)")
