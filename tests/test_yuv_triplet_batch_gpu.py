"""`vfi_yuv_triplet_batch_prepare` / `ops.yuv_triplet_batch_prepare`: the Y'CbCr frames of a batch's
triplets -> the rgb and Lab tensors of a training step, in one launch that decodes only the crops.

Expected values are yuv_ref.py's restatements of the WHOLE frame (`yuv_to_rgb`, `rgb2lab`, in float64 and float32), then
numpy slicing in the order crop, hflip, vflip, slot; nothing of the library is used for them.  rgb and Lab must lie within
glue_ref.tol_of(float32 restatement, float64 restatement) of the float64 restatement, both sliced: the rule of
tests/test_yuv_gpu.py.  A second assertion compares with `ops.yuv_to_rgb` of each whole frame, sliced by torch: the two
kernels share the per-pixel code and the block ownership, so the bits are equal.

Frames are random bytes, so a crop interior to the frame tells chroma clamped at the crop's edge from chroma clamped at the
frame's.  Sources and crops are the smallest that reach every path: 2x2 (every neighbour index clamps; 1x1 crops at each
origin), 6x10 and 18x66 (crops of 5x7 at even, odd and mixed origins and in the far corner: partial blocks on every side),
8x130 (8x128 at j = 0: whole float4 rows; at j = 2: blocks split by the crop's edge; 6x127 at (1, 3): odd everything), and
3x5, 7x67 in 4:4:4.  Every case runs all eight flag values, B = 3 with three different parameter rows, the source on 16 bytes
at a stride of the frame's bytes and one byte in at a stride of one byte more, and the outputs dense on 16 bytes and with
padded strides one float into their storage."""
import numpy as np
import pytest
import torch

import yuv_ref as YR
from glue_ref import assert_close, assert_untouched, canary_buffer, fview
from vfi_amd import ops
from vfi_amd._lib import VfiLibraryError

pytestmark = pytest.mark.gpu

GUARD = 0xAB
ONE_PER_CLASS = [(YR.S420, YR.CENTRE, YR.BT709, YR.LIMITED), (YR.S420, YR.LEFT, YR.BT601, YR.FULL), (YR.S444, YR.CENTRE, YR.BT601, YR.LIMITED)]

# (Hs, Ws, h, w, i, j)
CROPS_420 = [(2, 2, 1, 1, 0, 0), (2, 2, 1, 1, 0, 1), (2, 2, 1, 1, 1, 0), (2, 2, 1, 1, 1, 1), (2, 2, 2, 2, 0, 0)]
for _hs, _ws in ((6, 10), (18, 66)):
    CROPS_420 += [(_hs, _ws, 5, 7, 0, 0), (_hs, _ws, 5, 7, 1, 1), (_hs, _ws, 5, 7, 1, 2), (_hs, _ws, 5, 7, _hs - 5, _ws - 7)]
CROPS_420 += [(8, 130, 8, 128, 0, 0), (8, 130, 8, 128, 0, 2), (8, 130, 6, 127, 1, 3)]
CROPS_444 = [(3, 5, 2, 3, 1, 1), (7, 67, 4, 61, 3, 5)]
CASES = [(f, c) for f in YR.FORMATS_420 for c in CROPS_420] + [(f, c) for f in YR.FORMATS_444 for c in CROPS_444]
CASE_IDS = [f"{YR.fmt_id(f)}-{c[0]}x{c[1]}-{c[2]}x{c[3]}at{c[4]},{c[5]}" for f, c in CASES]

_sources = {}


def source(fmt, hs, ws, b, device):
    """Seeded frames (b, 3, frame bytes) and everything computed once from them: the whole-frame restatements in float64
    and float32, (b, 3 frames, 3, hs, ws) each, and `ops.yuv_to_rgb` of each whole frame on the device."""
    key = (fmt, hs, ws, b)
    if key not in _sources:
        n = YR.frame_bytes(hs, ws, fmt)
        frames = np.random.default_rng(1000 * hs + ws + b).integers(0, 256, (b, 3, n), dtype=np.uint8)
        ref = {}
        for name, dtype in (("64", np.float64), ("32", np.float32)):
            rgb = np.stack([np.stack([YR.yuv_to_rgb(frames[s, f], hs, ws, fmt, dtype) for f in range(3)]) for s in range(b)])
            ref["rgb" + name] = rgb
            ref["lab" + name] = np.stack([np.stack([YR.rgb2lab(rgb[s, f], dtype) for f in range(3)]) for s in range(b)])
        dev = [[ops.yuv_to_rgb(torch.from_numpy(frames[s, f]).to(device), hs, ws, fmt, rgb=True, lab=(True, None))[:2]
                for f in range(3)] for s in range(b)]
        ref["rgb_dev"] = torch.stack([torch.stack([dev[s][f][0] for f in range(3)]) for s in range(b)])
        ref["lab_dev"] = torch.stack([torch.stack([dev[s][f][1] for f in range(3)]) for s in range(b)])
        _sources[key] = (frames, ref)
    return _sources[key]


def sliced(whole, params, h, w):
    """whole (B, 3 frames, 3, Hs, Ws), numpy or torch -> (3 slots, B, 3, h, w): crop, hflip, vflip, then the slot choice"""
    is_t = isinstance(whole, torch.Tensor)
    out = []
    for n, (i, j, flags) in enumerate(np.asarray(params).tolist()):
        frames = []
        for f in range(3):
            a = whole[n, f][:, i:i + h, j:j + w]
            if flags & 1:
                a = a.flip(2) if is_t else a[:, :, ::-1]
            if flags & 2:
                a = a.flip(1) if is_t else a[:, ::-1]
            frames.append(a)
        first, middle, last = frames
        if flags & 4:
            first, last = last, first
        out.append([first, last, middle])
    stack = torch.stack if is_t else np.stack
    return stack([stack([out[n][s] for n in range(len(out))]) for s in range(3)])


def place_source(frames, byte_off, extra, device):
    """(storage, src): src (B, 3, frame bytes + extra) `16 + byte_off` bytes into a storage of GUARD bytes"""
    b, _, n = frames.shape
    fs = n + extra
    store = torch.full((b * 3 * fs + 64,), GUARD, dtype=torch.uint8, device=device)
    src = store[16 + byte_off:16 + byte_off + b * 3 * fs].view(b, 3, fs)
    src[:, :, :n] = torch.from_numpy(frames).to(device)
    return store, src


def outputs(b, h, w, padded, device):
    """(flat rgb, rgb, flat lab, lab): (3, b, 3, h, w) views into canary buffers, dense on 16 bytes, or one float in with 3
    floats between samples and 5 more between slots"""
    block = 3 * h * w
    off, sb = (1, block + 3) if padded else (0, block)
    ss = b * sb + (5 if padded else 0)
    strides = (ss, sb, h * w, w, 1)
    flats = [canary_buffer(3 * ss + off + 7, device) for _ in range(2)]
    return flats[0], fview(flats[0], (3, b, 3, h, w), off, strides), flats[1], fview(flats[1], (3, b, 3, h, w), off, strides)


def rows_for(hs, ws, h, w, i, j, flags, b):
    """b different parameter rows: the flags rotate, the crop of the later samples moves where the frame has room"""
    return np.array([[min(i + n, hs - h), max(j - n, 0), (flags + 3 * n) % 8] for n in range(b)], dtype=np.int32)


def check(fmt, hs, ws, h, w, params, device, variants=((0, 0, False), (1, 1, True)), what=""):
    b = len(params)
    frames, ref = source(fmt, hs, ws, b, device)
    want = {k: sliced(ref[k], params, h, w) for k in ref}
    got = None
    for byte_off, extra, padded in variants:
        store, src = place_source(frames, byte_off, extra, device)
        before = store.clone()
        flat_r, rgb, flat_l, lab = outputs(b, h, w, padded, device)
        out = ops.yuv_triplet_batch_prepare(src, fmt, torch.from_numpy(params), (h, w), (hs, ws), rgb=rgb, lab=lab)
        tag = f"{what} params {params.tolist()} src+{byte_off} stride+{extra} padded={padded}"
        assert out[0] is rgb and out[1] is lab
        assert torch.equal(store, before), f"{tag}: the source or its guard bytes were written"
        assert_untouched(flat_r, rgb, what="rgb " + tag)
        assert_untouched(flat_l, lab, what="lab " + tag)
        assert_close(rgb, want["rgb32"], want["rgb64"], "rgb " + tag)
        assert_close(lab, want["lab32"], want["lab64"], "lab " + tag)
        # the whole-frame decoder's bits: same per-pixel code, same block ownership
        assert torch.equal(rgb, want["rgb_dev"]), f"{tag}: rgb differs from ops.yuv_to_rgb of the whole frame"
        assert torch.equal(lab, want["lab_dev"]), f"{tag}: lab differs from ops.yuv_to_rgb of the whole frame"
        again = outputs(b, h, w, padded, device)
        ops.yuv_triplet_batch_prepare(src, fmt, torch.from_numpy(params), (h, w), (hs, ws), rgb=again[1], lab=again[3])
        assert torch.equal(again[1], rgb) and torch.equal(again[3], lab), f"{tag}: a repeated call gives other bits"
        if got is not None:
            assert torch.equal(rgb, got[0]) and torch.equal(lab, got[1]), f"{tag}: differs from the other alignment"
        got = (rgb.clone(), lab.clone())
    return got


@pytest.mark.parametrize("fmt,crop", CASES, ids=CASE_IDS)
def test_crop_flips_and_slots_of_the_whole_frame_decode(fmt, crop, device):
    hs, ws, h, w, i, j = crop
    for flags in range(8):
        check(fmt, hs, ws, h, w, rows_for(hs, ws, h, w, i, j, flags, 3), device, what=f"flags {flags}")


@pytest.mark.parametrize("fmt", ONE_PER_CLASS, ids=YR.fmt_id)
def test_a_batch_beyond_one_launch_of_64_samples(fmt, device):
    b, hs, ws, h, w = 65, 6, 10, 5, 7
    rng = np.random.default_rng(5)
    params = np.stack([rng.integers(0, hs - h + 1, b), rng.integers(0, ws - w + 1, b), rng.integers(0, 8, b)], 1).astype(np.int32)
    assert len({tuple(r) for r in params.tolist()}) > 8 and params[64].tolist() != params[0].tolist()
    check(fmt, hs, ws, h, w, params, device, what="B=65")


@pytest.mark.parametrize("fmt", YR.FORMATS_420 + YR.FORMATS_444, ids=YR.fmt_id)
def test_out_of_gamut_corners_land_on_the_clamp_exactly(fmt, device):
    corners = [(0, 255, 255), (255, 0, 0), (0, 0, 0), (255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 0, 255),
               (16, 16, 240), (235, 240, 16), (128, 255, 0), (128, 0, 255)]
    hs, ws = 4, 2 * len(corners)                                  # 2 x 2 luma blocks of one colour each, two rows of blocks
    y = np.zeros((hs, ws), dtype=np.uint8)
    c = np.zeros((2, hs // 2, ws // 2), dtype=np.uint8)
    for n, (yy, cb, cr) in enumerate(corners):
        y[:, 2 * n:2 * n + 2] = yy
        c[0, :, n], c[1, :, n] = cb, cr
    if fmt[0] == YR.S444:
        c = c.repeat(2, axis=1).repeat(2, axis=2)
    frame = np.concatenate([y.ravel(), c.ravel()])
    raw = YR.yuv_to_rgb(frame, hs, ws, fmt, np.float64, clamp=False)
    assert (raw < -0.01).any() and (raw > 1.01).any()
    h, w, i, j = 3, ws - 3, 1, 1
    frames = np.broadcast_to(frame, (1, 3, len(frame))).copy()
    for flags, (byte_off, extra) in zip((0, 3, 5, 6), ((0, 0), (1, 1), (0, 0), (1, 1))):
        params = np.array([[i, j, flags]], dtype=np.int32)
        want = sliced(np.broadcast_to(raw, (1, 3) + raw.shape), params, h, w)
        _, src = place_source(frames, byte_off, extra, device)
        rgb = ops.yuv_triplet_batch_prepare(src, fmt, torch.from_numpy(params), (h, w), (hs, ws), lab=None)[0].cpu().numpy()
        assert (want < -1e-3).any() and (want > 1 + 1e-3).any()
        assert (rgb[want < -1e-3] == 0.0).all() and (rgb[want > 1 + 1e-3] == 1.0).all()
        assert rgb.min() >= 0.0 and rgb.max() <= 1.0


@pytest.mark.parametrize("fmt", ONE_PER_CLASS, ids=YR.fmt_id)
def test_rgb_only_and_lab_only_calls(fmt, device):
    hs, ws, h, w, b = (6, 10, 5, 7, 2) if fmt[0] == YR.S420 else (7, 67, 4, 61, 2)
    frames, _ = source(fmt, hs, ws, b, device)
    params = torch.tensor([[1, 1, 5], [0, 2, 2]], dtype=torch.int32)
    _, src = place_source(frames, 1, 1, device)
    full_r, full_l = ops.yuv_triplet_batch_prepare(src, fmt, params, (h, w), (hs, ws))
    assert full_r.shape == (3, b, 3, h, w) and full_l.shape == (3, 3 * b, h, w)
    for padded in (False, True):
        flat_r, rgb, flat_l, lab = outputs(b, h, w, padded, device)
        only_r, none_l = ops.yuv_triplet_batch_prepare(src, fmt, params, (h, w), (hs, ws), rgb=rgb, lab=None)
        assert only_r is rgb and none_l is None and torch.equal(rgb, full_r)
        assert_untouched(flat_r, rgb, what="rgb alone")
        none_r, only_l = ops.yuv_triplet_batch_prepare(src, fmt, params, (h, w), (hs, ws), rgb=False, lab=lab)
        assert none_r is None and only_l is lab and torch.equal(lab, full_l.view(3, b, 3, h, w))
        assert_untouched(flat_l, lab, what="lab alone")
    # a Y4MFormat-like object and a dense (3, 3B, h, w) Lab destination
    fmt_obj = type("F", (), {"yuv": fmt})()
    lab4 = torch.full((3, 3 * b, h, w), float("nan"), device=device)
    assert ops.yuv_triplet_batch_prepare(src, fmt_obj, params, (h, w), (hs, ws), rgb=None, lab=lab4)[1] is lab4
    assert torch.equal(lab4, full_l)


def test_refusals_leave_the_outputs_alone(device):
    b, hs, ws, h, w = 2, 6, 10, 5, 7
    f420, f444 = (0, 0, 0, 0), (1, 0, 0, 0)
    src = torch.zeros((b, 3, YR.frame_bytes(hs, ws, f420)), dtype=torch.uint8, device=device)
    ok = [[0, 0, 0], [1, 3, 7]]

    def refused(src, fmt, params, size=(h, w), source_size=(hs, ws), **kw):
        rgb = torch.full((3, b, 3, size[0], size[1]), float("nan"), device=device)
        lab = torch.full((3, 3 * b, size[0], size[1]), float("nan"), device=device)
        with pytest.raises(VfiLibraryError):
            ops.yuv_triplet_batch_prepare(src, fmt, torch.tensor(params, dtype=torch.int32), size, source_size,
                                          rgb=kw.get("rgb", rgb), lab=kw.get("lab", lab))
        torch.cuda.synchronize()
        assert bool(torch.isnan(rgb).all()) and bool(torch.isnan(lab).all())
    refused(src, f420, [[0, 0, 0], [2, 3, 0]])                       # i + h > Hs (second sample: the first alone would pass)
    refused(src, f420, [[0, 4, 0], [0, 0, 0]])                       # j + w > Ws
    refused(src, f420, [[0, 0, 8], [0, 0, 0]])                       # flags = 8
    refused(src, f420, [[-1, 0, 0], [0, 0, 0]])
    refused(src, f420, ok, size=(7, 7))                              # crop taller than the source
    refused(src, f420, ok, size=(0, 7))
    for bad in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2), (0, 0, 0, -1), (0, 0, 0)):
        refused(src, bad, ok)
    refused(src, f444, ok)                                           # 4:2:0-sized frames for a 4:4:4 format
    refused(src[:, :, :-1], f420, ok)                                # frames a byte short
    refused(torch.zeros((b, 3, 5 * 10 * 3 // 2 + 64), dtype=torch.uint8, device=device), f420, ok, size=(3, 7), source_size=(5, 10))     # odd Hs
    refused(torch.zeros((b, 3, 6 * 9 * 3 // 2 + 64), dtype=torch.uint8, device=device), f420, ok, size=(5, 5), source_size=(6, 9))      # odd Ws
    refused(src.float(), f420, ok)
    refused(src.cpu(), f420, ok)
    refused(src[0], f420, ok)                                        # (3, n): no batch dimension
    refused(src, f420, ok[:1])                                       # one parameter row for two samples
    refused(src, f420, ok, rgb=None, lab=None)                       # nothing wanted
    refused(src, f420, ok, rgb=torch.zeros((3, b, 3, h, w + 1), device=device))
    refused(src, f420, ok, lab=torch.zeros((3, 3 * b, h, w), device=device, dtype=torch.float64))
    rgb, lab = ops.yuv_triplet_batch_prepare(src, f420, torch.tensor(ok, dtype=torch.int32), (h, w), (hs, ws))     # the accepted call still runs
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(lab).all())
