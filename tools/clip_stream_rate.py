#!/usr/bin/env python3
"""Y4M-inclusive clip rate at 1080p (read + H2D + decode + interpolate + encode + D2H + write), the counterpart of
clip_io_rate.py for vfi_amd.fusion_net.interpolate_stream (DESIGN.md sections 30 and 31).  With --kernels instead the
conversion and scene-cut kernels alone: time per call and effective TB/s over the bytes they move.

usage: clip_stream_rate.py [frames=13] [frames_in_flight=2] [--factor 2|4|8] [--scene_threshold T] [--kernels]"""
import argparse
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
ap = argparse.ArgumentParser()
ap.add_argument("frames", type=int, nargs="?", default=13)
ap.add_argument("frames_in_flight", type=int, nargs="?", default=2)
ap.add_argument("--factor", type=int, choices=(2, 4, 8), default=2)
ap.add_argument("--scene_threshold", type=float, default=None)
ap.add_argument("--kernels", action="store_true")
opts = ap.parse_args()
n, fif = opts.frames, opts.frames_in_flight
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


if opts.kernels:
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
    # the scene-cut calls: the statistic over two luma planes, and the pick with and without a cut (a cut copies the frame).
    # They touch the 24 frames only, 75 MB, which stay in the Infinity Cache -- as in the clip loop, where both calls read
    # bytes that were uploaded or encoded just before.  luma_sad's time includes its 8-byte memset.
    words = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(sets)]
    big = torch.full((1,), 1 << 40, dtype=torch.int64, device=dev)
    for name, moved, fn in (
            ("luma_sad", 2 * H * W, lambda i: ops.luma_sad(frames[i], frames[(i + 1) % sets], H * W, out=words[i])),
            ("frame_pick, no cut", 16, lambda i: ops.frame_pick(frames[i], frames[(i + 1) % sets], words[i], None, 1 << 50)),
            ("frame_pick, cut", 2 * nb, lambda i: ops.frame_pick(frames[i], frames[(i + 1) % sets], big, None, 1))):
        sec = timed(lambda: fn(nxt()))
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
    args = types.SimpleNamespace(gpu_id=0, matrix="bt709", range="limited", keep_rate=False, factor=opts.factor,
                                 scene_threshold=opts.scene_threshold)

    def run():
        with open(path, "rb") as s, open(out, "wb") as d:
            return st.interpolate_stream(args, s, d, runners=runners, frames_in_flight=fif)
    run()                                                             # warm-up (plans, packed weights)
    t0 = time.perf_counter()
    done = run()
    dt = time.perf_counter() - t0
    frames_out = opts.factor * (n - 1) + 1
    assert os.path.getsize(out) > frames_out * W * H * 3 // 2
    extra = ""
    if opts.factor != 2 or opts.scene_threshold is not None:
        extra = f", factor {opts.factor}, {frames_out / dt:.2f} output frames/s"
    if opts.scene_threshold is not None:
        extra += f", threshold {opts.scene_threshold:g}: {len(args.scene_cuts)} scene cuts"
    print(f"clip of {n} frames at {W}x{H} from/to Y4M: {done} interpolated frames in {dt:.2f} s = {done / dt:.2f} frames/s "
          f"({fif} frames in flight{extra})")
