#!/usr/bin/env python3
"""The input side of training from clips on synthetic C420jpeg clips of 448x256 and 1920x1080, crops of
256x256, batches of 8:

* samples/s of ClipTripletLoader alone (pread threads, pinned staging, upload, vfi_yuv_triplet_batch_prepare) for 1, 2, 4
  and 8 threads on each source size, and of TripletLoader on PNG triplets of 448x256 in the same run;
* vfi_yuv_triplet_batch_prepare alone at B = 8 on each source size: us between device events over rotating sets of source
  and output buffers that together exceed the 256 MiB Infinity Cache, with the bytes it moves (1.5 source bytes read and 24
  written per output pixel, chroma halo not counted) and the rate that gives;
* the path it replaces, in the same run: 24 whole-frame vfi_yuv_to_rgb launches into float intermediates plus the slicing
  copies (crop, flips, slot) into the same outputs.

Loader figures are a host clock around whole passes that end in a device synchronise, after a warm-up pass; --repeats passes
are printed one by one, the configurations alternating, so the spread shows.  Frames are seeded noise: nothing here depends
on the picture."""
import argparse
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tools")]
from train_input_rate import wall, write_dataset  # noqa: E402
from vfi_amd import ops  # noqa: E402
from vfi_amd.train.clipreader import ClipTripletLoader, DBreader_Y4M  # noqa: E402
from vfi_amd.train.datareader import DBreader_Vimeo90k, TripletLoader  # noqa: E402

CROP = (256, 256)
SIZES = ((256, 448), (1080, 1920))
FMT = (0, 0, 0, 0)                      # C420jpeg, BT.709, limited range
CACHE = 256 << 20


def write_clip(path, h, w, frames, seed=0):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip C420jpeg\n" % (w, h))
        for _ in range(frames):
            f.write(b"FRAME\n")
            f.write(rng.integers(16, 236, h * w * 3 // 2, dtype=np.uint8).tobytes())


def events_us(fn, sets, rounds, warm=1):
    """us per call of fn(k), k cycling over `sets` buffer sets, between two device events"""
    for _ in range(warm):
        for k in range(sets):
            fn(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        for k in range(sets):
            fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (rounds * sets)


def kernel_alone(dev, h, w, b, repeats):
    g = torch.Generator().manual_seed(0)
    n = h * w * 3 // 2
    out_bytes = 2 * 9 * b * CROP[0] * CROP[1] * 4
    sets = CACHE // (b * 3 * n + out_bytes) + 2                     # the sets together exceed the cache
    srcs = [torch.randint(16, 236, (b, 3, n), generator=g, dtype=torch.uint8).to(dev) for _ in range(sets)]
    rgbs = [torch.empty((3, b, 3) + CROP, device=dev) for _ in range(sets)]
    labs = [torch.empty((3, 3 * b) + CROP, device=dev) for _ in range(sets)]
    params = torch.stack([torch.randint(0, h - CROP[0] + 1, (b,), generator=g, dtype=torch.int32),
                          torch.randint(0, w - CROP[1] + 1, (b,), generator=g, dtype=torch.int32),
                          torch.randint(0, 8, (b,), generator=g, dtype=torch.int32)], 1)
    rows = params.tolist()
    whole_rgb = [torch.empty((3, h, w), device=dev) for _ in range(3 * b)]       # the replaced path's intermediates
    whole_lab = [torch.empty((3, h, w), device=dev) for _ in range(3 * b)]

    def one_launch(k):
        ops.yuv_triplet_batch_prepare(srcs[k], FMT, params, CROP, (h, w), rgb=rgbs[k], lab=labs[k])

    def replaced(k):
        lab5 = labs[k].view(3, b, 3, *CROP)
        for s, (i, j, flags) in enumerate(rows):
            for f in range(3):
                q = 3 * s + f
                ops.yuv_to_rgb(srcs[k][s, f], h, w, FMT, rgb=whole_rgb[q], lab=(whole_lab[q], None))
                slot = 2 if f == 1 else int((f == 2) != bool(flags & 4))
                for whole, out in ((whole_rgb[q], rgbs[k]), (whole_lab[q], lab5)):
                    a = whole[:, i:i + CROP[0], j:j + CROP[1]]
                    dims = [d for d, bit in ((2, 1), (1, 2)) if flags & bit]
                    out[slot, s].copy_(a.flip(dims) if dims else a)
    one_launch(0)
    want = (rgbs[0].clone(), labs[0].clone())
    replaced(0)
    same = torch.equal(rgbs[0], want[0]) and torch.equal(labs[0], want[1])
    moved = 3 * b * CROP[0] * CROP[1] * (1.5 + 24)
    print(f"  {w}x{h}, B={b}, rgb and lab, {sets} buffer sets of {(b * 3 * n + out_bytes) / 2**20:.0f} MiB; "
          f"the replaced path gives the same bits: {same}")
    for rep in range(repeats):
        a = events_us(one_launch, sets, 4)
        r = events_us(replaced, sets, 1)
        print(f"    round {rep}: one launch {a:8.1f} us ({moved / a * 1e-3:6.0f} GB/s of {moved / 1e6:.1f} MB)   "
              f"{3 * b} yuv_to_rgb + slicing copies {r:9.1f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("the kernel alone (us between events per call):")
    for h, w in SIZES:
        kernel_alone(dev, h, w, args.batch, args.repeats)
    with tempfile.TemporaryDirectory() as root:
        feeds = {}
        for h, w in SIZES:
            d = os.path.join(root, f"{w}x{h}")
            os.makedirs(d)
            write_clip(os.path.join(d, "clip.y4m"), h, w, args.samples + 2)
            ds = DBreader_Y4M(d, random_crop=CROP)
            assert len(ds) == args.samples
            for n in args.workers:
                feeds[f"ClipTripletLoader {w}x{h}, {n} threads"] = (lambda ds=ds, n=n: ClipTripletLoader(ds, args.batch, workers=n, device=dev))
        png = os.path.join(root, "png")
        write_dataset(png, args.samples)
        vimeo = DBreader_Vimeo90k(png, random_crop=CROP)
        for n in args.workers:
            feeds[f"TripletLoader PNG 448x256, {n} threads"] = (lambda n=n: TripletLoader(vimeo, args.batch, workers=n, device=dev))
        print(f"the loaders alone ({args.samples} samples per pass, samples/s per repeat; {os.cpu_count()} CPUs reported, "
              f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}):")
        rates = {name: [] for name in feeds}
        for rep in range(args.repeats + 1):
            for name, mk in feeds.items():
                random.seed(0)
                torch.manual_seed(0)
                t = wall(lambda: [None for _ in mk()])
                if rep:
                    rates[name].append(args.samples / t)
        for name, r in rates.items():
            print(f"  {name:44s} " + "  ".join(f"{v:8.1f}" for v in r) + f"   median {sorted(r)[len(r) // 2]:8.1f}")


if __name__ == "__main__":
    main()
