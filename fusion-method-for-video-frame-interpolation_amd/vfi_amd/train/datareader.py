"""Vimeo-90k triplet reader -- mirror of reference src/train/datareader.py:17-74, and the batch loader that feeds the
trainers from it.

`DBreader_Vimeo90k` has two faces over one parameter draw:

* `__getitem__(index)` is the reference's contract -- three float (3, h, w) CPU tensors, cropped, flipped and swapped on the
  host with PIL -- so the class works under a stock `torch.utils.data.DataLoader` exactly as the reference's does;
* `raw(index)` gives the three decoded uint8 (H, W, 3) arrays and `draw(height, width)` the sample's (i, j, flags);
  `TripletLoader` sends the former to the device as they are and the latter to `ops.triplet_batch_prepare`, which does the
  crop, the flips, the swap, the / 255 and `preprocess` of a whole batch in one launch.

`draw` consumes `torch`'s and `random`'s global generators exactly as the reference's `__getitem__` does
(`RandomCrop.get_params`: `torch.randint` for i, then j, nothing when the crop is the frame; then `random.random() < 0.5` for
the horizontal flip, the vertical flip and the temporal swap, each only when its `augment_*` flag is on), so one seed gives
one sequence of parameters on either face.

Differences from the reference: the triplet list is sorted (`os.listdir` order depends on the file system); frames that are
not RGB are converted; `torchvision` is not used.  `resize` is applied with PIL at decode time (bilinear) on both faces; the
reference never sets it when training, and its parity with `transforms.Resize` is unpinned.
"""
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from .. import ops

HFLIP, VFLIP, SWAP = 1, 2, 4
MAX_WORKERS = 16


def cointoss(p):
    return random.random() < p


def draw_params(random_crop, augment_s, augment_t, height, width):
    """One sample's (crop row i, crop column j, flags) for frames of height x width, drawn as the reference's `__getitem__`
    draws them: the one parameter draw of every reader here (DBreader_Vimeo90k, clipreader.DBreader_Y4M)."""
    i = j = 0
    if random_crop is not None:
        th, tw = random_crop
        if height < th or width < tw:
            raise ValueError(f"Required crop size {(th, tw)} is larger than input image size {(height, width)}")
        if not (width == tw and height == th):
            i = torch.randint(0, height - th + 1, size=(1,)).item()
            j = torch.randint(0, width - tw + 1, size=(1,)).item()
    flags = 0
    if augment_s:
        if cointoss(0.5):
            flags |= HFLIP
        if cointoss(0.5):
            flags |= VFLIP
    if augment_t:
        if cointoss(0.5):
            flags |= SWAP
    return i, j, flags


class DBreader_Vimeo90k(Dataset):
    def __init__(self, db_dir, random_crop=None, resize=None, augment_s=True, augment_t=True):
        db_dir = db_dir + "/sequences"
        self.random_crop = tuple(int(v) for v in random_crop) if random_crop is not None else None
        self.resize = resize
        self.augment_s = augment_s
        self.augment_t = augment_t
        isdir = lambda d, f: os.path.isdir(os.path.join(d, f))
        self.folder_list = sorted(db_dir + "/" + f for f in os.listdir(db_dir) if isdir(db_dir, f))
        self.triplet_list = []
        for folder in self.folder_list:
            self.triplet_list += sorted(folder + "/" + f for f in os.listdir(folder) if isdir(folder, f))
        self.triplet_list = np.array(self.triplet_list)
        self.file_len = len(self.triplet_list)

    def __len__(self):
        return self.file_len

    def _open(self, path):
        img = Image.open(path)
        if img.mode != "RGB":
            img = img.convert("RGB")
        if self.resize is not None:
            if isinstance(self.resize, int):            # the shorter side becomes `resize`
                w, h = img.size
                s = self.resize / min(w, h)
                size = (self.resize, max(1, int(h * s))) if w <= h else (max(1, int(w * s)), self.resize)
            else:
                size = (int(self.resize[1]), int(self.resize[0]))
            img = img.resize(size, Image.BILINEAR)
        return img

    def images(self, index):
        """The three PIL frames im1, im2, im3 of a triplet, decoded (and resized), not augmented."""
        d = str(self.triplet_list[index])
        return [self._open(d + f"/im{k}.png") for k in (1, 2, 3)]

    def raw(self, index):
        """The three frames as uint8 (H, W, 3) arrays, not augmented."""
        return [np.asarray(img) for img in self.images(index)]

    def crop_size(self, height, width):
        return self.random_crop if self.random_crop is not None else (height, width)

    def draw(self, height, width):
        """One sample's (crop row i, crop column j, flags) for frames of height x width; flags = HFLIP | VFLIP | SWAP."""
        return draw_params(self.random_crop, self.augment_s, self.augment_t, height, width)

    def __getitem__(self, index):
        frames = self.images(index)
        width, height = frames[1].size
        i, j, flags = self.draw(height, width)
        h, w = self.crop_size(height, width)
        if self.random_crop is not None:
            frames = [f.crop((j, i, j + w, i + h)) for f in frames]
        if flags & HFLIP:
            frames = [f.transpose(Image.FLIP_LEFT_RIGHT) for f in frames]
        if flags & VFLIP:
            frames = [f.transpose(Image.FLIP_TOP_BOTTOM) for f in frames]
        # ToTensor: HWC uint8 -> CHW float / 255
        frame0, frame1, frame2 = (torch.from_numpy(np.array(f)).permute(2, 0, 1).contiguous().float().div(255) for f in frames)
        if flags & SWAP:
            return frame2, frame1, frame0
        return frame0, frame1, frame2


class TripletBatch:
    """What TripletLoader yields.  lab (3, 3B, h, w): slots [first frame, last frame, target], each `preprocess` of its rgb;
    rgb (3, B, 3, h, w) in [0, 1]; params: the host int32 (B, 3) the batch was drawn with; paths: its triplet folders."""

    def __init__(self, lab, rgb, params, paths):
        self.lab, self.rgb, self.params, self.paths = lab, rgb, params, paths

    @property
    def img_batch_phase(self):
        """(9B, h, w): `torch.cat((lab_frame1, lab_frame2, target), 0)` of reference src/train/trainer.py:103, as a view."""
        return self.lab.view(-1, self.lab.shape[2], self.lab.shape[3])

    lab_frame1 = property(lambda self: self.lab[0])
    lab_frame2 = property(lambda self: self.lab[1])
    lab_target = property(lambda self: self.lab[2])
    rgb_frame1 = property(lambda self: self.rgb[0])
    rgb_frame2 = property(lambda self: self.rgb[1])
    rgb_target = property(lambda self: self.rgb[2])


class StagedLoader:
    """What the loaders of this package share: the batching of a dataset with `__len__` and `raw(index)`, `raw` running
    ahead -- this batch and the next -- on a ThreadPoolExecutor, two pinned uint8 staging buffers, each written again only
    after the event recorded behind its copy, and the non-blocking upload.  A subclass gives `_assemble(indices, futures)`,
    which turns the `raw` results of one batch into what the loader yields."""

    def __init__(self, dataset, batch_size, shuffle=True, workers=4, device="cuda", generator=None, rgb=True, lab=True):
        if batch_size < 1:
            raise ValueError(f"{type(self).__name__}: batch_size must be at least 1")
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), shuffle
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.device = torch.device(device)
        self.generator = generator
        self.want_rgb, self.want_lab = rgb, lab
        self._staging = [None, None]
        self._events = [None, None]
        self._turn = 0

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _stage(self, shape):
        """The next of the two staging buffers, free to be written, with room for `shape`."""
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()
            self._events[k] = None
        need = int(np.prod(shape))
        if self._staging[k] is None or self._staging[k].numel() < need:
            self._staging[k] = torch.empty(need, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        return k, self._staging[k][:need].view(shape)

    def _upload(self, k, stage):
        """Staging buffer k -> the device, non-blocking on the current stream, with the event that frees the buffer."""
        src = stage.to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            self._events[k] = torch.cuda.Event()
            self._events[k].record()
        return src

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        batches = [order[a:a + self.batch_size] for a in range(0, n, self.batch_size)]
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            submit = lambda idx: [pool.submit(self.dataset.raw, i) for i in idx]
            pending = [submit(b) for b in batches[:2]]
            try:
                for t, idx in enumerate(batches):
                    futures = pending.pop(0)
                    if t + 2 < len(batches):
                        pending.append(submit(batches[t + 2]))
                    yield self._assemble(idx, futures)
            finally:
                for futs in pending:
                    for f in futs:
                        f.cancel()


class TripletLoader(StagedLoader):
    """Batches of a DBreader_Vimeo90k on the device.  len = ceil(N / batch_size); the last batch is short, as a DataLoader
    without drop_last.

    Per batch, the consuming thread draws every sample's parameters in sample order (`dataset.draw`), so results never
    depend on thread timing or on `workers`.  Decoding runs ahead -- this batch and the next -- on a ThreadPoolExecutor (PIL
    releases the GIL; no worker processes: the parent has the GPU open, and a fork of it is not a clean process).  The
    frames are gathered in one of two pinned uint8 staging buffers, copied non-blocking on the current stream, and
    `ops.triplet_batch_prepare` does the rest in one launch.  A staging buffer is written again only after the event
    recorded behind its copy.  All samples of a batch must decode to one size.

    shuffle: a `torch.randperm` from `generator` (None: the global generator) at the start of every pass."""

    def _assemble(self, indices, futures):
        ds = self.dataset
        paths = [str(ds.triplet_list[i]) for i in indices]
        params = torch.empty((len(indices), 3), dtype=torch.int32)
        stage = k = shape = None
        for n, fut in enumerate(futures):
            frames = fut.result()
            if any(f.shape != frames[0].shape for f in frames) or frames[0].ndim != 3 or frames[0].shape[2] != 3:
                raise ValueError(f"TripletLoader: {paths[n]}: frames of shapes {[f.shape for f in frames]}")
            if stage is None:
                shape = frames[0].shape
                k, stage = self._stage((len(indices), 3) + shape)
                host = stage.numpy()
            elif frames[0].shape != shape:
                raise ValueError(f"TripletLoader: one batch holds {paths[0]} of {shape[0]}x{shape[1]} and {paths[n]} of "
                                 f"{frames[0].shape[0]}x{frames[0].shape[1]}: a batch has one source size")
            params[n, 0], params[n, 1], params[n, 2] = ds.draw(shape[0], shape[1])
            for f in range(3):
                host[n, f] = frames[f]
        src = self._upload(k, stage)
        rgb, lab = ops.triplet_batch_prepare(src, params, ds.crop_size(shape[0], shape[1]), rgb=self.want_rgb, lab=self.want_lab)
        return TripletBatch(lab, rgb, params, paths)
