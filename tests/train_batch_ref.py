"""References of the training input side (tests/test_triplet_batch_gpu.py, test_datareader_host.py, test_trainer_gpu.py).

* `prepare_ref`: numpy restatement of what `vfi_triplet_batch_prepare` does to the frames -- slice, `[:, ::-1]`, `[::-1]`, slot
  swap (reference src/train/datareader.py:45-69) -- on uint8, so the rgb comparison is bit for bit.
* `lab_restated`: oracle.color_cpu.rgb2lab_single's formulas for (N, 3, H, W), every step in the given dtype: float64 is the
  reference, float32 the `ref32` of tests/glue_ref.tol_of.
* `reference_draw`: datareader.py:45-69 line by line, as far as it consumes random numbers.
* `write_triplets`: a tiny Vimeo-shaped dataset of seeded PNGs.
"""
import os
import random

import numpy as np
import torch

from oracle import color_cpu

HFLIP, VFLIP, SWAP = 1, 2, 4


def prepare_ref(src, params, h, w):
    """src uint8 (B, 3, Hs, Ws, 3) numpy, params (B, 3) -> uint8 (3 slots, B, 3, h, w): [first, last, middle] frame."""
    b = src.shape[0]
    out = np.empty((3, b, 3, h, w), dtype=np.uint8)
    for n in range(b):
        i, j, flags = (int(v) for v in params[n])
        frames = []
        for f in range(3):
            a = src[n, f, i:i + h, j:j + w]
            if flags & HFLIP:
                a = a[:, ::-1]
            if flags & VFLIP:
                a = a[::-1]
            frames.append(a.transpose(2, 0, 1))
        first, middle, last = frames
        if flags & SWAP:
            first, last = last, first
        out[0, n], out[1, n], out[2, n] = first, last, middle
    return out


def to_float(u8):
    """torch's `uint8.float() / 255`"""
    return torch.from_numpy(np.ascontiguousarray(u8)).float() / 255


def lab_restated(rgb, dtype):
    """rgb (N, 3, H, W) float32 tensor -> scaled Lab (N, 3, H, W), every step in `dtype` (np.float32 | np.float64)."""
    f = dtype
    arr = rgb.permute(0, 2, 3, 1).numpy().astype(f)
    arr = np.where(arr > f(0.04045), np.power((arr + f(0.055)) / f(1.055), f(2.4)), arr / f(12.92))
    xyz = arr @ color_cpu.XYZ_FROM_RGB.T.astype(f) / color_cpu.WHITE_D65_2.astype(f)
    t = np.where(xyz > f(0.008856), np.cbrt(xyz), f(7.787) * xyz + f(16.0) / f(116.0))
    L = f(116.0) * t[..., 1] - f(16.0)
    a = f(500.0) * (t[..., 0] - t[..., 1])
    b = f(200.0) * (t[..., 1] - t[..., 2])
    lab = np.stack([L / f(100.0), (a + f(128.0)) / f(255.0), (b + f(128.0)) / f(255.0)], 1)
    assert lab.dtype == f
    return torch.from_numpy(lab)


def lab_slots(rgb_u8, dtype):
    """uint8 (3, B, 3, h, w) -> Lab (3, 3B, h, w) of rgb / 255, in `dtype`"""
    s, b, _, h, w = rgb_u8.shape
    return lab_restated(to_float(rgb_u8).reshape(s * b, 3, h, w), dtype).reshape(s, 3 * b, h, w)


def threshold_source():
    """uint8 (1, 3, 6, 8, 3): channels at the byte values around rgb2lab's thresholds -- 9..12 (0.04045 * 255 = 10.3, the sRGB
    knee), 0..3 (the darkest values of the linear branches) and 19..26 (a grey crosses the Lab knee, linear value 0.008856,
    between bytes 23 and 24: ((v/255 + 0.055) / 1.055) ** 2.4 = 0.008856 at v = 23.5) -- as greys, as single channels over
    black, and in mixed triples."""
    vals = [0, 1, 2, 3, 9, 10, 11, 12] + list(range(19, 27))
    src = np.zeros((1, 3, 6, 8, 3), dtype=np.uint8)
    for f in range(3):
        for k in range(8):
            v = vals[k + 8 * (f % 2)]
            src[0, f, 0, k] = v                                  # grey
            for c in range(3):
                src[0, f, 1 + c, k, c] = v                       # one channel over black
            src[0, f, 4, k] = (v, vals[(k + 3) % 16], vals[(k + 5) % 16])
            src[0, f, 5, k] = (vals[(k + 1) % 8], 255 - v, v)
    return src


def reference_draw(height, width, random_crop, augment_s, augment_t):
    """What datareader.py:45-69 draws, in its order (RandomCrop.get_params: `torch.randint` for i then j, nothing when the
    crop is the frame; cointoss = `random.random() < p`)."""
    i = j = 0
    if random_crop is not None:
        th, tw = random_crop
        if not (width == tw and height == th):
            i = torch.randint(0, height - th + 1, size=(1,)).item()
            j = torch.randint(0, width - tw + 1, size=(1,)).item()
    flags = 0
    if augment_s:
        if random.random() < 0.5:
            flags |= HFLIP
        if random.random() < 0.5:
            flags |= VFLIP
    if augment_t:
        if random.random() < 0.5:
            flags |= SWAP
    return i, j, flags


def write_triplets(root, count, height, width, seed=0, smooth=False, sizes=None):
    """<root>/sequences/0000<k>/000<n>/im{1,2,3}.png, two triplets per folder; -> root.  `smooth`: low-frequency frames
    with a small motion (something a network can be trained on for a step) instead of noise; sizes: {index: (h, w)}."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for n in range(count):
        h, w = (sizes or {}).get(n, (height, width))
        d = os.path.join(root, "sequences", f"{n // 2 + 1:05d}", f"{n % 2 + 1:04d}")
        os.makedirs(d)
        if smooth:
            yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            ph = rng.random(3) * 6
        for k in range(3):
            if smooth:
                img = np.stack([0.5 + 0.4 * np.sin((xx + 1.5 * k) * (0.21 + 0.05 * c) + ph[c]) * np.cos((yy - k) * (0.17 + 0.04 * c) + n)
                                for c in range(3)], -1)
                img = (img * 255).round().astype(np.uint8)
            else:
                img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"im{k + 1}.png"))
    return root
