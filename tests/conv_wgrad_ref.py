"""Case table, plan restatement and float64 references of the isolated weight-gradient tests
(test_conv_wgrad_host.py, test_conv_backward_gpu.py).  Plain Python, no GPU.

conv_wgrad_kernel<KS> (csrc/vfi_conv_grad.hip) gives one workgroup a run of `tiles_per_split` consecutive tiles; the
run may cross a tile-row end and an image boundary, and the last run may be short.  With the default workspace every
small layer gets one tile per workgroup, so each case lists the `max_splits` caps (ops.conv2d_backward_weight) that make
the runs longer, with the plan each cap must give.  The table states those numbers as literals: the host test holds
plan() to them, the GPU test holds the library's own split count to plan().
"""
import collections
import functools

import torch
import torch.nn.functional as F

from glue_ref import SENTINEL

WORKSPACE_FLOATS = 48 * 1024 * 1024     # ops.WORKSPACE_FLOATS (the GPU test asserts they agree)
WG_COLS, WG_TX = 128, 32                # kWgCols, kWgTX

Plan = collections.namedtuple("Plan", "tiles_x tiles_y tiles_total col_blocks co_blocks tiles_per_split splits last_tiles")


def _ceil_div(a, b):
    return -(-a // b)


def tile_rows(ks):
    return 1 if ks == 1 else 4          # WgradCfg<KS>::TY


def plan(n, cin, h, w, cout, ks, workspace_floats):
    """wgrad_plan of csrc/vfi_conv_grad.hip, plus the tile count of the last split."""
    tiles_x = _ceil_div(w, WG_TX)
    tiles_y = _ceil_div(h, tile_rows(ks))
    tiles_total = n * tiles_x * tiles_y
    col_blocks = _ceil_div(cin * ks * ks, WG_COLS)
    co_blocks = _ceil_div(cout, 32)
    per_split = cout * (cin * ks * ks + 1)
    s = min(_ceil_div(1024, col_blocks * co_blocks), 256, tiles_total, workspace_floats // per_split)
    s = max(s, 1)
    tiles_per_split = _ceil_div(tiles_total, s)
    splits = _ceil_div(tiles_total, tiles_per_split)
    return Plan(tiles_x, tiles_y, tiles_total, col_blocks, co_blocks, tiles_per_split, splits,
                tiles_total - (splits - 1) * tiles_per_split)


def workspace_for(case, max_splits):
    """The workspace size ops.conv2d_backward_weight hands on for this cap."""
    if max_splits is None:
        return WORKSPACE_FLOATS
    return min(WORKSPACE_FLOATS, max(int(max_splits), 1) * case.cout * (case.cin * case.ks * case.ks + 1))


def case_plan(case, max_splits):
    return plan(case.n, case.cin, case.h, case.w, case.cout, case.ks, workspace_for(case, max_splits))


def walk(p, ks, h, w):
    """The pixels each split's workgroup reads, in the kernel's order: for split s, tiles t_begin .. t_end - 1, tile t ->
    (n, y, x) over the tile's live rows and columns.  Yields (split, n, y, x)."""
    ty = tile_rows(ks)
    for split in range(p.splits):
        t_begin = split * p.tiles_per_split
        t_end = min(t_begin + p.tiles_per_split, p.tiles_total)
        for t in range(t_begin, t_end):
            txi, tyi, n = t % p.tiles_x, (t // p.tiles_x) % p.tiles_y, t // (p.tiles_x * p.tiles_y)
            for y in range(tyi * ty, min(tyi * ty + ty, h)):
                for x in range(txi * WG_TX, min(txi * WG_TX + WG_TX, w)):
                    yield split, n, y, x


class Case(collections.namedtuple("Case", "n cin cout h w ks pad caps sliced tags")):
    """caps: {max_splits: (tiles_per_split, splits, tiles of the last split)}; sliced: x and dy are channel slices of
    wider NaN-filled tensors."""

    @property
    def key(self):
        return (self.n, self.cin, self.cout, self.h, self.w, self.ks, self.pad, self.sliced)

    @property
    def id(self):
        return "%dx%d-%d_%dx%d_k%d_%s%s" % (self.n, self.cin, self.cout, self.h, self.w, self.ks, self.pad,
                                             "_sliced" if self.sliced else "")


def _case(n, cin, cout, h, w, ks, pad, caps, tags, sliced=False):
    return Case(n, cin, cout, h, w, ks, pad, caps, sliced, tags)


_ROW_A = (2, 3, 5, 9, 70, 3, "zeros", {None: (1, 18, 1), 5: (4, 5, 2), 4: (5, 4, 3), 2: (9, 2, 9), 1: (18, 1, 18)})
_ROW_B = (2, 6, 33, 7, 40, 5, "reflect", {None: (1, 8, 1), 3: (3, 3, 2), 1: (8, 1, 8)})

CASES = [
    _case(*_ROW_A, "3x3 tiles per image: runs cross tile-row ends and the image boundary (tile 9); ragged last split; one "
                   "workgroup walks everything"),
    _case(*_ROW_B, "KS 5; 2 column blocks x 2 cout blocks (Cout 33: a tail of 1); reflect halo; H 7 no multiple of TY"),
    _case(2, 130, 3, 5, 40, 1, "zeros", {None: (1, 20, 1), 4: (5, 4, 5), 1: (20, 1, 20)},
          "KS 1 (TY 1); 130 columns = 128 + 2; Cout 3"),
    _case(1, 29, 31, 6, 65, 3, "reflect", {None: (1, 6, 1), 2: (3, 2, 3), 1: (6, 1, 6)},
          "261 columns; an input channel straddles a 128-column block; W 65: three x-tiles, 1 live column in the last"),
    _case(1, 11, 32, 5, 33, 5, "zeros", {None: (1, 4, 1), 1: (4, 1, 4)}, "275 columns in 3 blocks; Cout exactly 32"),
    _case(1, 3, 40, 3, 100, 1, "reflect", {None: (1, 12, 1), 5: (3, 4, 3), 1: (12, 1, 12)},
          "KS 1, four x-tiles, 2 cout blocks"),
    _case(1, 1, 1, 3, 33, 5, "reflect", {None: (1, 2, 1), 1: (2, 1, 2)},
          "Cin = Cout = 1; H = pad + 1 (every row is a mirror source) at W > 32"),
    _case(1, 257, 1, 2, 31, 1, "zeros", {None: (1, 2, 1), 1: (2, 1, 2)}, "3 column blocks for KS 1; Cout 1"),
    _case(1, 4, 65, 8, 32, 3, "reflect", {None: (1, 2, 1), 1: (2, 1, 2)}, "3 cout blocks; W exactly 32"),
] + [
    # slab_reduce_kernel sums slab 0, then eight at a time, then the rest: 1+8, 1+8+1, 1+8+8, 1+8+8+1
    _case(1, 2, 4, h, 32, 3, "zeros", {None: (1, s, 1)}, "slab_reduce_kernel over %d slabs" % s)
    for h, s in ((33, 9), (37, 10), (65, 17), (69, 18))
] + [
    _case(1, 1, 1, 1, 1, ks, "zeros", {None: (1, 1, 1)}, "one pixel") for ks in (1, 3, 5)
] + [
    # batch strides that differ from C*H*W, NaN around the slices; n = 2 and runs of several tiles
    _case(*_ROW_A, "row 1 with x and dy as channel slices of wider tensors", sliced=True),
    _case(*_ROW_B, "row 2 with x and dy as channel slices of wider tensors", sliced=True),
]

CASE_CAPS = [(c, m) for c in CASES for m in c.caps]
CASE_CAP_IDS = ["%s-cap%s" % (c.id, m) for c, m in CASE_CAPS]

X_SLICE = (3, 2)        # channels of NaN before / after x in its wide tensor
DY_SLICE = (1, 4)       # ... and around dy


# ---- data and float64 references -----------------------------------------------------------------------------------
def _pad_conv(x, w, pad):
    k = w.shape[-1]
    p = (k - 1) // 2
    if p and pad == "reflect":
        return F.conv2d(F.pad(x, (p,) * 4, mode="reflect"), w)
    return F.conv2d(x, w, padding=p)


def weight_grad64(x, dy, ks, pad):
    """float64 dW (Cout, Cin, KS, KS) of the stride-1 layer by autograd (the layer is linear in W: any W serves)."""
    wd = torch.zeros((dy.shape[1], x.shape[1], ks, ks), dtype=torch.float64, requires_grad=True)
    (_pad_conv(x.double(), wd, pad) * dy.double()).sum().backward()
    return wd.grad.detach()


Data = collections.namedtuple("Data", "x dy dw db a sum_abs_dy k")


@functools.lru_cache(maxsize=None)
def data(key, kind):
    """kind 'int': x integers in [-3, 3], dy in [-2, 2] (every partial sum an integer far below 2**24: fp32 is exact in
    any order); 'randn': unit Gaussians.  -> fp32 x, dy and float64 dW, db, A = dW(|x|, |dy|), sum |dy| per channel, and
    K = n*h*w, the length of each dot product.  Computed once per case; do not modify."""
    n, cin, cout, h, w, ks, pad, _ = key
    g = torch.Generator().manual_seed(1000003 * ks + 7919 * h + 31 * w + 17 * cin + 5 * cout + n + (kind == "int"))
    if kind == "int":
        x = torch.randint(-3, 4, (n, cin, h, w), generator=g).float()
        dy = torch.randint(-2, 3, (n, cout, h, w), generator=g).float()
    else:
        x = torch.randn((n, cin, h, w), generator=g)
        dy = torch.randn((n, cout, h, w), generator=g)
    return Data(x, dy, weight_grad64(x, dy, ks, pad), dy.double().sum((0, 2, 3)),
                weight_grad64(x.abs(), dy.abs(), ks, pad), dy.double().abs().sum((0, 2, 3)), n * h * w)


def embed_in_nan(t, before, after):
    """(wide, slice): `t` (N, C, H, W) as channels [before, before + C) of a wider CPU tensor whose other channels hold
    the sentinel NaN of glue_ref."""
    n, c, h, w = t.shape
    wide = torch.full((n, before + c + after, h, w), SENTINEL, dtype=torch.int32).view(torch.float32)
    wide[:, before:before + c] = t
    return wide, wide[:, before:before + c]
