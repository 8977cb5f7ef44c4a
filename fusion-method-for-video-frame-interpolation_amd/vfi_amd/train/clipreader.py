"""Training from clips: a triplet reader over YUV4MPEG2 files and the loader that feeds the trainers from it (DESIGN.md
section 32).  A user's own footage reaches training the way it reaches inference: as `.y4m`, with no PNG extraction step.

`DBreader_Y4M` indexes each clip once (`y4m.index_clip`) and lists every (clip, k) whose frames k, k + stride, k + 2 stride
lie inside the clip.  `raw(index)` gives the three frames' bytes as they lie in the file; `draw` is the parameter draw of
`DBreader_Vimeo90k` (`datareader.draw_params`), so one seed gives one parameter sequence on either reader.  There is no host
decoder: `ClipTripletLoader` uploads the bytes and `ops.yuv_triplet_batch_prepare` decodes only the crops, applies the flips
and the swap, and writes rgb and Lab of the whole batch in one launch.

`add_arguments` / `training_input` are what the three training command lines share: `--train_clips PATH` selects this reader,
without it each trainer builds the Vimeo reader it always built.
"""
import glob
import os

import numpy as np
import torch

from .. import ops
from ..fusion_net import y4m
from .datareader import DBreader_Vimeo90k, StagedLoader, TripletBatch, TripletLoader, draw_params


builtin_range = range       # (`range` is a parameter name of DBreader_Y4M, as of y4m.read_header)


class DBreader_Y4M:
    """source: a directory (its `*.y4m` files, sorted) or a list of files.  All clips must share their size and the four
    format integers (subsampling, siting, matrix, range).  Samples are ordered clip by clip, then by first frame k."""

    def __init__(self, source, random_crop=None, augment_s=True, augment_t=True, stride=1, matrix="bt709", range="limited"):
        if isinstance(source, (str, os.PathLike)):
            files = sorted(glob.glob(os.path.join(os.fspath(source), "*.y4m")))
            if not files:
                raise ValueError(f"DBreader_Y4M: no *.y4m files in {source}")
        else:
            files = [os.fspath(f) for f in source]
        stride = int(stride)
        if stride < 1:
            raise ValueError("DBreader_Y4M: stride must be at least 1")
        self.random_crop = tuple(int(v) for v in random_crop) if random_crop is not None else None
        self.augment_s, self.augment_t, self.stride = augment_s, augment_t, stride
        self.files, self.offsets, self.samples, self.paths = files, [], [], []
        self.fmt = None
        self._fds = []
        for c, path in enumerate(files):
            fmt, offsets = y4m.index_clip(path, matrix, range)
            if self.fmt is None:
                self.fmt = fmt
            elif (fmt.height, fmt.width) != (self.fmt.height, self.fmt.width) or fmt.yuv != self.fmt.yuv:
                raise ValueError(f"DBreader_Y4M: {files[0]} is {self.fmt.width}x{self.fmt.height} with format {self.fmt.yuv} and "
                                 f"{path} is {fmt.width}x{fmt.height} with format {fmt.yuv}: all clips must share both")
            self.offsets.append(offsets)
            for k in builtin_range(len(offsets) - 2 * stride):
                self.samples.append((c, k))
                self.paths.append(f"{path}#{k}")
        self.height, self.width = (self.fmt.height, self.fmt.width) if self.fmt is not None else (0, 0)
        self.frame_bytes = self.fmt.frame_bytes if self.fmt is not None else 0
        self._fds = [os.open(path, os.O_RDONLY) for path in files]      # one descriptor per clip; pread has no shared position

    def close(self):
        fds, self._fds = getattr(self, "_fds", []), []
        for fd in fds:
            os.close(fd)

    def __del__(self):
        self.close()

    def __len__(self):
        return len(self.samples)

    def raw(self, index):
        """The three frames of sample `index` as uint8 arrays of `frame_bytes`, as they lie in the file."""
        c, k = self.samples[index]
        frames = []
        for f in builtin_range(3):
            data = os.pread(self._fds[c], self.frame_bytes, self.offsets[c][k + f * self.stride])
            if len(data) != self.frame_bytes:
                raise ValueError(f"DBreader_Y4M: {self.files[c]}: frame {k + f * self.stride} ends after {len(data)} bytes")
            frames.append(np.frombuffer(data, dtype=np.uint8))
        return frames

    def crop_size(self, height, width):
        return self.random_crop if self.random_crop is not None else (height, width)

    def draw(self, height, width):
        """One sample's (crop row i, crop column j, flags): DBreader_Vimeo90k.draw's draw."""
        return draw_params(self.random_crop, self.augment_s, self.augment_t, height, width)

    def __getitem__(self, index):
        raise TypeError("DBreader_Y4M has no host-decoded samples (the package has no host YUV decoder): iterate a "
                        "ClipTripletLoader over it, which decodes on the device")


class ClipTripletLoader(StagedLoader):
    """Batches of a DBreader_Y4M on the device: TripletLoader's protocol (the same arguments, `__len__`, a short last batch,
    the TripletBatch it yields; `paths` are "file#k").  Per batch, the consuming thread draws the parameters in sample order;
    the reads run ahead on the thread pool; the frames' bytes are gathered in one of two pinned staging buffers of
    (B, 3, frame_bytes), uploaded in one non-blocking copy, and one `ops.yuv_triplet_batch_prepare` makes the batch."""

    def _assemble(self, indices, futures):
        ds = self.dataset
        paths = [ds.paths[i] for i in indices]
        params = torch.empty((len(indices), 3), dtype=torch.int32)
        k, stage = self._stage((len(indices), 3, ds.frame_bytes))
        host = stage.numpy()
        for n, fut in enumerate(futures):
            frames = fut.result()
            params[n, 0], params[n, 1], params[n, 2] = ds.draw(ds.height, ds.width)
            for f in builtin_range(3):
                host[n, f] = frames[f]
        src = self._upload(k, stage)
        rgb, lab = ops.yuv_triplet_batch_prepare(src, ds.fmt, params, ds.crop_size(ds.height, ds.width), (ds.height, ds.width),
                                                 rgb=self.want_rgb, lab=self.want_lab)
        return TripletBatch(lab, rgb, params, paths)


def add_arguments(parser):
    """The clip flags of a training command line."""
    parser.add_argument('--train_clips', type=str, default=None, metavar='PATH',
                        help='train from the *.y4m clips of this directory instead of the Vimeo triplets of --train')
    parser.add_argument('--clip_stride', type=int, default=1, help='frames between the members of a triplet')
    parser.add_argument('--matrix', type=str, choices=sorted(y4m.MATRICES), default='bt709')
    parser.add_argument('--range', type=str, choices=sorted(y4m.RANGES), default='limited',
                        help='an XCOLORRANGE token in a clip\'s header wins')


def reader_class(args):
    """The dataset class a training command line builds from its arguments."""
    return DBreader_Y4M if getattr(args, 'train_clips', None) else DBreader_Vimeo90k


def training_input(args, random_crop, device, **loader_kw):
    """-> (dataset, loader) of a training command line: DBreader_Y4M and ClipTripletLoader with --train_clips,
    DBreader_Vimeo90k and TripletLoader without.  loader_kw: rgb / lab."""
    if reader_class(args) is DBreader_Y4M:
        dataset = DBreader_Y4M(args.train_clips, random_crop=random_crop, stride=args.clip_stride, matrix=args.matrix, range=args.range)
        loader = ClipTripletLoader
    else:
        dataset = DBreader_Vimeo90k(args.train, random_crop=random_crop)
        loader = TripletLoader
    return dataset, loader(dataset, args.batch_size, shuffle=True, workers=args.workers, device=device, **loader_kw)
