#!/usr/bin/env python3
"""The input side of training on a directory of synthetic 448x256 PNGs, crops of 256x256:

* samples/s of TripletLoader alone (decode threads, pinned staging, upload, vfi_triplet_batch_prepare) for 1, 2, 4 and 8
  decoding threads;
* vfi_triplet_batch_prepare alone at B = 8: ms and GB/s of the bytes it moves (3 source bytes read, 12 or 24 written per
  pixel and frame);
* a whole phase-mode training step (architecture.PhaseNet at batch 8, m = 10, batch statistics, get_loss, Adam) fed by the
  loader at each thread count, fed by the reference's way -- a stock DataLoader(num_workers=0) over
  DBreader_Vimeo90k.__getitem__, float upload, `preprocess`, `torch.cat` -- and on a batch already on the device.

Every figure is a host clock around whole passes over the dataset that end in a device synchronise, after a warm-up pass;
--repeats passes are printed one by one, the configurations alternating, so the spread shows.  The frames are seeded noise
over a smooth picture: real Vimeo frames compress better and decode faster or slower; nobody has measured them."""
import argparse
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
import phasenet_walk_ref as W  # noqa: E402
from vfi_amd import ops  # noqa: E402
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet  # noqa: E402
from vfi_amd.train.datareader import DBreader_Vimeo90k, TripletLoader  # noqa: E402
from vfi_amd.train.loss import get_loss  # noqa: E402
from vfi_amd.train.utils import calc_pyr_height, preprocess  # noqa: E402

H, W_, CROP = 256, 448, (256, 256)


def write_dataset(root, count, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W_), indexing="ij")
    size = 0
    for n in range(count):
        d = os.path.join(root, "sequences", f"{n // 8 + 1:05d}", f"{n % 8 + 1:04d}")
        os.makedirs(d)
        for k in range(3):
            base = np.stack([127 + 90 * np.sin((xx + 3 * k) * (0.02 + 0.01 * c) + n) * np.cos(yy * 0.03 + c) for c in range(3)], -1)
            img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"im{k + 1}.png"))
            size += os.path.getsize(os.path.join(d, f"im{k + 1}.png"))
    return size / (3 * count)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


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


def kernel_alone(dev, b=8):
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (b, 3, H, W_, 3), generator=g, dtype=torch.uint8).to(dev)
    params = torch.stack([torch.zeros(b, dtype=torch.int32), torch.randint(0, W_ - CROP[1] + 1, (b,), generator=g, dtype=torch.int32),
                          torch.randint(0, 8, (b,), generator=g, dtype=torch.int32)], 1)
    rgb = torch.empty((3, b, 3) + CROP, device=dev)
    lab = torch.empty((3, 3 * b) + CROP, device=dev)
    pix = 3 * b * CROP[0] * CROP[1]
    for name, kw, bytes_ in (("lab alone (phase mode)", dict(rgb=None, lab=lab), pix * (3 + 12)),
                             ("rgb and lab", dict(rgb=rgb, lab=lab), pix * (3 + 24)),
                             ("rgb alone", dict(rgb=rgb, lab=None), pix * (3 + 12))):
        ms = timed(lambda: ops.triplet_batch_prepare(src, params, CROP, **kw), 50, 5)
        print(f"  vfi_triplet_batch_prepare B={b} {CROP[0]}x{CROP[1]}, {name:24s} {ms * 1e3:8.1f} us  {bytes_ / (ms * 1e-3) * 1e-9:7.0f} GB/s "
              f"of {bytes_ / 1e6:.1f} MB")
    ms = timed(lambda: torch.cat([preprocess(rgb[s], dev) for s in range(3)], 0), 50, 5)
    print(f"  for comparison, cat(preprocess x 3) of float rgb already on the device {ms * 1e3:8.1f} us")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 2, 4, 8])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        mean_size = write_dataset(root, args.samples)
        print(f"{args.samples} triplets of {W_}x{H} PNGs, {mean_size / 1e3:.0f} KB each, written in {time.perf_counter() - t0:.1f} s; "
              f"{os.cpu_count()} CPUs reported, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}")
        ds = DBreader_Vimeo90k(root, random_crop=CROP)
        from PIL import Image
        path = str(ds.triplet_list[0]) + "/im1.png"
        t0 = time.perf_counter()
        for _ in range(20):
            np.asarray(Image.open(path).convert("RGB"))
        print(f"PIL decode of one frame on this host: {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms")
        kernel_alone(dev, args.batch)

        def seed():
            random.seed(0)
            torch.manual_seed(0)
        loaders = {f"TripletLoader, {w} threads": (lambda w=w: TripletLoader(ds, args.batch, workers=w, device=dev, rgb=False))
                   for w in args.workers}

        def reference_batches():
            for triple in torch.utils.data.DataLoader(dataset=ds, batch_size=args.batch, shuffle=True, num_workers=0):
                lab1, lab2, target = (preprocess(triple[k], dev) for k in (0, 2, 1))      # trainer.py:115-117
                yield torch.cat((lab1, lab2, target), 0), target                          # :103

        def device_batches(loader):
            for batch in loader:
                yield batch.img_batch_phase, batch.lab_target
        feeds = {name: (lambda mk=mk: device_batches(mk())) for name, mk in loaders.items()}
        feeds["reference DataLoader(num_workers=0) + preprocess"] = reference_batches

        print("the loader alone (one pass over the dataset, samples/s per repeat):")
        rates = {name: [] for name in feeds}
        for rep in range(args.repeats + 1):
            for name, feed in feeds.items():
                seed()
                t = wall(lambda: [None for _ in feed()])
                if rep:
                    rates[name].append(args.samples / t)
        for name, r in rates.items():
            print(f"  {name:52s} " + "  ".join(f"{v:7.1f}" for v in r) + f"   ({1e3 * args.batch / max(r):.1f} ms per batch of {args.batch} at best)")

        height = calc_pyr_height(torch.empty(3, *CROP, device="meta"))
        net = ArchPhaseNet(height, dev).fine_tune(batch_stats=True)
        net.core.load_state_dict(W.net_state(0))
        opt = torch.optim.Adam(net.parameters(), lr=1e-5)

        def step(img_batch, target):
            prediction, vals_pred, vals_target = net(img_batch, m=args.m)
            loss = get_loss(vals_pred, vals_target, prediction, target, net.pyr)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
        seed()
        resident = next(iter(feeds[next(iter(feeds))]()))
        ms = timed(lambda: step(*resident), 10, 3)
        print(f"the step alone on a resident batch (B={args.batch}, {CROP[0]}x{CROP[1]}, height {height}, m={args.m}, batch statistics, Adam): {ms:.2f} ms")
        print("the step with its input (ms per step per repeat, one pass over the dataset each):")
        times = {name: [] for name in feeds}
        steps = -(-args.samples // args.batch)
        for rep in range(args.repeats + 1):
            for name, feed in feeds.items():
                seed()
                t = wall(lambda: [step(*b) for b in feed()])
                if rep:
                    times[name].append(1e3 * t / steps)
        for name, r in times.items():
            print(f"  {name:52s} " + "  ".join(f"{v:7.2f}" for v in r))


if __name__ == "__main__":
    main()
