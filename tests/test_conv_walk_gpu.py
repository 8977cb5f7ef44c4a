"""The item walk of the three persistent Winograd 3x3 kernels (conv3x3_winograd_kernel, conv3x3_winograd4_kernel,
conv3x3_winograd4m_kernel) at small shapes.

A launch has min(items, resident) workgroups, so a small layer gives every workgroup ONE item and none of the code that
carries the request cursor across item boundaries runs: the ring of 8 bias slots, the per-item rebuild of descriptors and
per-lane offsets, the switch between border and interior tiles, the M = 32 kernel's three cursors and its LOOP statement,
the empty requests past the end of the sequence, next_valid over padded items, the K-split item order.
vfi_debug_conv_override caps the launch grid (and nothing else), so the same small layer is walked by 1, 2, 3, 5, 8 or 13
workgroups: each output must equal the uncapped launch's bit for bit (an item's arithmetic does not depend on which
workgroup runs it), from NaN-poisoned LDS into a NaN-filled output, and the uncapped launch is compared with a float64
CPU convolution at the bounds of tests/test_conv_gpu.py."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from vfi_amd import _lib, ops

pytestmark = pytest.mark.gpu

KERNELS = ("f2x2", "f4x4_m16", "f4x4_m32")
CAPS = (1, 2, 3, 5, 8, 13)
ACTS = (None, "relu", "elu", "tanh", "sigmoid")
ACT_FN = {None: lambda t: t, "relu": F.relu, "elu": F.elu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}
NAN = float("nan")


@pytest.fixture
def select(monkeypatch):
    """select(kernel, cap): sends every 3x3 layer to `kernel` and caps its launch grid; (-1, 0) again afterwards."""
    lib = _lib.lib()

    def set_(kernel, cap=0):
        if kernel != "f2x2":
            monkeypatch.setenv("VFI_CONV_WINOGRAD4M", "1" if kernel == "f4x4_m32" else "0")
        assert lib.vfi_debug_conv_override(0 if kernel == "f2x2" else 2, cap) == 0
    try:
        yield set_
    finally:
        assert lib.vfi_debug_conv_override(-1, 0) == 0


# ---- a case: inputs, float64 reference (computed once per shape, shared by kernels and caps), device tensors ----------
class Case:
    """variant: plain | residual | slices (x, out, residual are channel slices of wider tensors) | pool_max | pool_avg |
    bwd_data (ops.conv2d_backward_data on a zero-padded layer n, cin -> cout: the null-bias path)."""

    def __init__(self, n, cin, cout, h, w, pad, act, variant="plain", splits=1):
        self.key = (n, cin, cout, h, w, pad, act, variant)
        self.n, self.cin, self.cout, self.h, self.w, self.pad, self.act, self.variant, self.splits = n, cin, cout, h, w, pad, act, variant, splits
        # the convolution the kernel runs: bwd_data convolves dy (cout channels) into dx (cin channels)
        self.k_in, self.k_out = (cout, cin) if variant == "bwd_data" else (cin, cout)

    def __repr__(self):
        return "Case%r" % (self.key,)


def _conv64(x, w, b, pad):
    if pad == "reflect":
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    return F.conv2d(x, w, b, padding=1)


@functools.lru_cache(maxsize=None)
def _prepared(key, device):
    """Inputs scaled as in tests/test_conv_gpu.py; -> dict of device tensors and float64 references."""
    n, cin, cout, h, w, pad, act, variant = key
    g = torch.Generator().manual_seed(cin * 1000 + cout * 37 + h * 7 + w + n)
    x = torch.randn((n, cin, h, w), generator=g)
    wgt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    res = torch.randn((n, cout, h, w), generator=g)
    p = {}
    if variant == "bwd_data":
        dy = res                                   # the output gradient
        xd = x.double().requires_grad_(True)
        (_conv64(xd, wgt.double(), None, "zeros") * dy.double()).sum().backward()
        p["ref"] = xd.grad.detach()
        p["dy"] = dy.to(device)
        p["pct"] = ops.packed_transposed(wgt.to(device))
        return p
    ref = ACT_FN[act](_conv64(x.double(), wgt.double(), b.double(), pad))
    if variant in ("residual", "slices"):
        ref = ref + res.double()
        p["res"] = res.to(device)
    if variant.startswith("pool"):
        p["ref_pool"] = (F.max_pool2d if variant == "pool_max" else F.avg_pool2d)(ref, 2)
    p["ref"] = ref
    p["pc"] = ops.PackedConv(wgt, b, device=device)
    p["x"] = x.to(device)
    if variant == "slices":
        p["wide_x"] = torch.randn((n, cin + 9, h, w), generator=g).to(device)
        p["wide_x"][:, 4:4 + cin] = p["x"]
        p["wide_res"] = torch.randn((n, cout + 5, h, w), generator=g).to(device)
        p["wide_res"][:, 2:2 + cout] = p["res"]
    return p


def _run(case, device):
    """One launch of the case into NaN-filled outputs -> tuple of output tensors."""
    p = _prepared(case.key, device)
    n, cin, cout, h, w = case.n, case.cin, case.cout, case.h, case.w
    if case.variant == "bwd_data":
        out = torch.full((n, cin, h, w), NAN, device=device)
        ops.conv2d_backward_data(p["dy"], p["pct"], "zeros", out=out)
        return (out,)
    if case.variant.startswith("pool"):
        y = torch.full((n, cout, h, w), NAN, device=device)
        q = torch.full((n, cout, h // 2, w // 2), NAN, device=device)
        ws = ops._workspace(device)
        pc = p["pc"]
        _lib.call("vfi_conv2d_pool2", p["x"].data_ptr(), p["x"].stride(0), pc.packed.data_ptr(), pc.bias.data_ptr(), y.data_ptr(), y.stride(0),
                  q.data_ptr(), q.stride(0), int(case.variant == "pool_max"), n, cin, h, w, cout, 3, ops.PAD[case.pad], ops.ACT[case.act],
                  ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        return (y, q)
    if case.variant == "slices":
        wide = torch.full((n, cout + 7, h, w), NAN, device=device)
        wide[:, :3] = 7.0
        wide[:, 3 + cout:] = 7.0
        wx, wr = p["wide_x"].clone(), p["wide_res"].clone()
        ops.conv2d(wx[:, 4:4 + cin], p["pc"], case.pad, case.act, residual=wr[:, 2:2 + cout], out=wide[:, 3:3 + cout])
        # what lies outside the slices is untouched
        assert (wide[:, :3] == 7.0).all() and (wide[:, 3 + cout:] == 7.0).all(), case
        assert torch.equal(wx, p["wide_x"]) and torch.equal(wr, p["wide_res"]), case
        return (wide[:, 3:3 + cout],)
    out = torch.full((n, cout, h, w), NAN, device=device)
    ops.conv2d(p["x"], p["pc"], case.pad, case.act, residual=p.get("res"), out=out)
    return (out,)


def _check_against_float64(kernel, case, outs, device):
    p = _prepared(case.key, device)
    if case.variant == "bwd_data":       # as test_conv_backward_entries_match_float64
        rel = float((outs[0].cpu().double() - p["ref"]).norm() / p["ref"].norm())
        assert rel <= 2e-5, (kernel, case, rel)
        return
    refs = (p["ref"], p["ref_pool"]) if case.variant.startswith("pool") else (p["ref"],)
    for out, ref in zip(outs, refs):
        assert out.shape == ref.shape, (kernel, case, out.shape)
        err = (out.cpu().double() - ref).abs()
        emax, erms = err.max().item(), err.pow(2).mean().sqrt().item()
        if kernel == "f2x2":             # test_winograd_conv_matches_torch_cpu
            assert emax <= 3e-5, (kernel, case, emax)
        else:                            # test_large_plain_conv_matches_torch_cpu
            assert emax <= 1e-4 and erms <= 5e-6, (kernel, case, emax, erms)


# ---- how many items each workgroup of a capped launch walks ------------------------------------------------------------
def _tile(kernel):
    return (8, 32) if kernel == "f2x2" else (16, 64)


def _item_count(kernel, case):
    th, tw = _tile(kernel)
    return math.ceil(case.h / th) * math.ceil(case.w / tw) * case.n * math.ceil(case.k_out / 32) * (case.splits if kernel == "f2x2" else 1)


def _items_per_workgroup(kernel, case, cap):
    """The launchers' item list (padded to whole XCD rounds) dealt to `cap` workgroups: valid items of each."""
    th, tw = _tile(kernel)
    tiles, cb = math.ceil(case.h / th) * math.ceil(case.w / tw), math.ceil(case.k_out / 32)
    run = 1
    while run < 8 and tiles * case.n >= 512 * run:
        run *= 2
    per_split = (tiles * case.n + 8 * run - 1) // (8 * run) * (8 * run) * cb
    counts = [0] * cap
    for L in range(per_split * (case.splits if kernel == "f2x2" else 1)):
        lr = L % per_split
        xcd, q = lr & 7, lr >> 3
        tq = q // cb
        tl = (tq // run * 8 + xcd) * run + tq % run
        counts[L % cap] += tl // tiles < case.n
    return counts


def _algo(case):
    return _lib.lib().vfi_conv2d_algo(case.n, case.k_in, case.h, case.w, case.k_out, 3, int(case.variant in ("residual", "slices")),
                                      int(case.variant.startswith("pool")), ops.ACT[case.act if case.variant != "bwd_data" else None])


def _walk(kernel, case, select, device):
    """Uncapped against float64; then every cap that leaves a workgroup two or more items, bit for bit against uncapped.
    -> (uncapped outputs, number of capped launches)."""
    select(kernel, 0)
    assert _algo(case) == (1 if kernel == "f2x2" else 2), (kernel, case)
    base = _run(case, device)
    torch.cuda.synchronize()
    _check_against_float64(kernel, case, base, device)
    items, capped = _item_count(kernel, case), 0
    for cap in CAPS:
        if items <= cap:                 # one item per workgroup at most: nothing is walked
            continue
        counts = _items_per_workgroup(kernel, case, cap)
        assert sum(counts) == items and max(counts) >= 2, (kernel, case, cap, counts)
        select(kernel, cap)
        _lib.call("vfi_debug_poison_lds", _lib.stream_ptr())
        got = _run(case, device)
        torch.cuda.synchronize()
        for a, b in zip(base, got):
            assert torch.equal(a, b), (kernel, case, cap, int((a != b).sum()), float((a - b).abs().nan_to_num(nan=1e30).max()))
        capped += 1
    select(kernel, 0)
    return base, capped


# ---- the cases ----------------------------------------------------------------------------------------------------------
# Chunk counts 1, 2, 3, 4, 4, 5, 6, 7, 9, 16, 17 (every Cin % 4, both body parities at an item's end) on N = 2, Cout = 40 (two
# channel blocks, the second a tail: neighbouring items use different biases), 37 x 200: for F(4x4) top / interior / bottom
# tile rows and left / interior / right tile columns (48 items), for F(2x2) five tile rows x seven tile columns (140 items).
# With cap 1 and Cin = 3 one workgroup walks all of them as one-chunk items: the 8 bias slots wrap several times while the
# request cursor is four items ahead.
CHUNK_CINS = (3, 6, 9, 13, 16, 18, 24, 28, 35, 64, 66)
CHUNK_CASES = [Case(2, cin, 40, 37, 200, ("zeros", "reflect")[i % 2], ACTS[i % 5]) for i, cin in enumerate(CHUNK_CINS)]

GEOMETRY = [
    # h, w, pad
    (2, 2, "reflect"),       # smallest reflect-padded image
    (5, 40, "zeros"),        # one partial tile
    (16, 64, "reflect"),     # exactly one F(4x4) tile
    (17, 65, "zeros"),       # one-row and one-column tiles
    (33, 63, "reflect"),     # three F(4x4) tile rows, ragged last column
    (48, 192, "zeros"),      # exact tiles (and M = 16 against M = 32)
    (34, 131, "reflect"),    # odd width: element-wise stores
    (40, 198, "zeros"),      # W % 4 == 2
]
GEOMETRY_CASES = [Case(n, 18, 32, h, w, pad, ACTS[(i + n) % 5]) for i, (h, w, pad) in enumerate(GEOMETRY) for n in (1, 3)]

VARIANT_CASES = [
    Case(2, 28, 25, 37, 200, "reflect", "elu", "residual"),
    Case(2, 28, 25, 37, 200, "zeros", "relu", "residual"),        # M = 32 has an instantiation of its own for ReLU + residual
    Case(2, 28, 25, 37, 199, "zeros", "relu", "pool_max"),        # odd sizes: the pooled plane floors
    Case(2, 28, 25, 37, 199, "reflect", "relu", "pool_avg"),
    Case(2, 28, 25, 48, 192, "zeros", "relu", "pool_avg"),        # even sizes, whole tiles: M = 32's straight-line epilogue pools too
    Case(2, 28, 25, 37, 200, "reflect", "elu", "slices"),
    Case(2, 28, 25, 37, 200, "zeros", None, "bwd_data"),
]

# F(2x2) K split.  launch_winograd's rule on a device of >= 96 CUs (2 resident workgroups each; every candidate fits one round):
#   (1, 256 -> 96, 12 x 40): 4 tiles x 3 channel blocks, padded to 24 items of 64 chunks; S <= 8 keeps >= 8 chunks per item;
#       cost(S) = 70.4 / S + 4 + (S + 1) * 0.074 us -> 70.4, 39.4, 22.0, 13.5 for S = 1, 2, 4, 8: 8 splits, 96 valid items.
#   (2, 512 -> 64, 9 x 15): 2 tiles x 2 samples x 2 channel blocks, padded to 16 items of 128 chunks; S <= 16;
#       cost(S) = 140.8 / S + 4 + (S + 1) * 0.028 us -> ..., 21.9, 13.3 for S = 8, 16: 16 splits, 64 valid items; the plane of
#       135 pixels is odd, so the reduce kernel works element by element.
# The capped walk therefore crosses split boundaries (consecutive items of a workgroup lie in different K ranges).
SPLITK_CASES = [Case(1, 256, 96, 12, 40, "zeros", "relu", splits=8), Case(2, 512, 64, 9, 15, "reflect", "elu", splits=16)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_chunk_counts_across_item_boundaries(kernel, select, device):
    for case in CHUNK_CASES:
        _, capped = _walk(kernel, case, select, device)
        assert capped == len(CAPS), (kernel, case, capped)


@pytest.mark.parametrize("kernel", KERNELS)
def test_tile_geometries_across_item_boundaries(kernel, select, device):
    capped = 0
    for case in GEOMETRY_CASES:
        capped += _walk(kernel, case, select, device)[1]
    assert capped >= 3 * len(GEOMETRY), (kernel, capped)       # (a single-item layer has no capped launch: N = 3 always has two)


@pytest.mark.parametrize("kernel", KERNELS)
def test_residual_pool_slices_and_null_bias_across_item_boundaries(kernel, select, device):
    for case in VARIANT_CASES:
        _, capped = _walk(kernel, case, select, device)
        assert capped == len(CAPS), (kernel, case, capped)


def test_f2x2_k_split_items_across_split_boundaries(select, device):
    for case in SPLITK_CASES:
        _, capped = _walk("f2x2", case, select, device)
        assert capped == len(CAPS), (case, capped)


def test_m16_and_m32_agree_bit_for_bit_on_whole_tile_rows(select, device):
    """Where W % 64 == 0 conv3x3_winograd4m_kernel documents the bits of conv3x3_winograd4_kernel -- also when one of them
    walks all items in a single workgroup."""
    cases = [c for c in GEOMETRY_CASES + VARIANT_CASES if c.w % 64 == 0 and c.variant != "bwd_data"]
    assert len(cases) >= 5
    for case in cases:
        select("f4x4_m16", 0)
        m16 = _run(case, device)
        select("f4x4_m32", 0)
        m32 = _run(case, device)
        select("f4x4_m32", 1)
        _lib.call("vfi_debug_poison_lds", _lib.stream_ptr())
        m32_one = _run(case, device)
        torch.cuda.synchronize()
        for a, b, c in zip(m16, m32, m32_one):
            assert torch.equal(a, b) and torch.equal(a, c), (case, float((a - b).abs().nan_to_num(nan=1e30).max()))


def test_override_rejects_other_values_and_is_restored(device):
    lib = _lib.lib()
    assert lib.vfi_debug_conv_override(3, 0) == -1 and lib.vfi_debug_conv_override(-2, 0) == -1 and lib.vfi_debug_conv_override(0, -1) == -1
    # a rejected call changes nothing: the small layer is still the cost model's F(2x2) layer, and mode 2 moves it
    assert lib.vfi_conv2d_algo(1, 18, 48, 192, 32, 3, 0, 0, 0) == 1
    try:
        assert lib.vfi_debug_conv_override(2, 0) == 0
        assert lib.vfi_conv2d_algo(1, 18, 48, 192, 32, 3, 0, 0, 0) == 2
    finally:
        assert lib.vfi_debug_conv_override(-1, 0) == 0
    assert lib.vfi_conv2d_algo(1, 18, 48, 192, 32, 3, 0, 0, 0) == 1
