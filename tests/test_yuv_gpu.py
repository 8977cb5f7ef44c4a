"""`vfi_yuv_to_rgb` / `vfi_rgb_to_yuv` through `ops.yuv_to_rgb` / `ops.rgb_to_yuv` against the numpy
restatements of yuv_ref.py, for all eight 4:2:0 formats and 4:4:4 in both ranges and matrices.

Shapes are the smallest that reach every path: 2x2 and 2x4 (every neighbour index clamps), 6x10, 16x24, 18x66 (W no multiple
of 4), 8x130 (a vector body plus a tail), 64x96 (several workgroups), and 1x1, 3x5, 7x67 for 4:4:4.  Every shape runs with
the frame one byte into its storage and the float planes one float into theirs (the byte / scalar paths), and with both on
16 bytes (the dword / float4 paths).

Decode: rgb and Lab within glue_ref.tol_of(float32 restatement, float64 restatement) of the float64 restatement, the rule of
the glue kernels and of tests/test_triplet_batch_gpu.py for Lab.
Encode: every byte equals floor(v64 + 0.5) of the float64 restatement, except where v64 lies within tol_of(pre-round float32,
pre-round float64) of a tie: there it may differ by 1, and such bytes may be at most 1 % of a case.  The inputs are seeded;
the seeds were fixed on the CPU, from the restatements alone, such that no case's inputs exceed that share (full-range
inputs that clamp to pure colours sit on exact ties: cb = +-1/2 gives 128 +- 127.5)."""
import numpy as np
import pytest
import torch

import yuv_ref as YR
from glue_ref import assert_close, assert_untouched, canary_buffer, fview
from vfi_amd import ops
from vfi_amd._lib import VfiLibraryError

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (2, 4), (6, 10), (16, 24), (18, 66), (8, 130), (64, 96)]
SHAPES_444 = SHAPES + [(1, 1), (3, 5), (7, 67)]
CASES = [(f, s) for f in YR.FORMATS_420 for s in SHAPES] + [(f, s) for f in YR.FORMATS_444 for s in SHAPES_444]
CASE_IDS = [f"{YR.fmt_id(f)}-{s[0]}x{s[1]}" for f, s in CASES]
ONE_PER_CLASS = [(YR.S420, YR.CENTRE, YR.BT709, YR.LIMITED), (YR.S420, YR.LEFT, YR.BT601, YR.FULL), (YR.S444, YR.CENTRE, YR.BT601, YR.LIMITED)]
GUARD = 0xAB
MAX_TIE_SHARE = 0.01


def frame_in_guards(data, byte_offset, device):
    """(storage, frame): the frame's bytes `16 + byte_offset` bytes into a storage of GUARD bytes (torch allocates on 256)"""
    n = len(data)
    store = torch.full((n + 64,), GUARD, dtype=torch.uint8, device=device)
    frame = store[16 + byte_offset:16 + byte_offset + n]
    frame.copy_(torch.as_tensor(data))
    return store, frame


def assert_guards(store, frame, what):
    c = store.clone()
    c[frame.storage_offset():frame.storage_offset() + frame.numel()] = GUARD
    assert bool((c == GUARD).all()), f"{what}: bytes outside the frame were modified"


def planes_in_guards(h, w, float_offset, device):
    flat = canary_buffer(3 * h * w + float_offset + 7, device)
    return flat, fview(flat, (3, h, w), float_offset)


def check_decode(frame_np, h, w, fmt, device, offsets, what):
    r64, r32 = YR.yuv_to_rgb(frame_np, h, w, fmt, np.float64), YR.yuv_to_rgb(frame_np, h, w, fmt, np.float32)
    l64, l32 = YR.rgb2lab(r64, np.float64), YR.rgb2lab(r32, np.float32)
    got = None
    for byte_off, float_off in offsets:
        store, frame = frame_in_guards(frame_np, byte_off, device)
        (fr, rgb), (fa, lab_a), (fb, lab_b) = (planes_in_guards(h, w, float_off, device) for _ in range(3))
        out = ops.yuv_to_rgb(frame, h, w, fmt, rgb=rgb, lab=(lab_a, lab_b))
        assert out[0] is rgb and out[1] is lab_a and out[2] is lab_b
        tag = f"{what} frame+{byte_off} planes+{float_off}"
        assert_guards(store, frame, tag)
        assert torch.equal(frame.cpu(), torch.as_tensor(frame_np)), f"{tag}: the frame was written"
        for flat, view in ((fr, rgb), (fa, lab_a), (fb, lab_b)):
            assert_untouched(flat, view, what=tag)
        assert_close(rgb, r32, r64, f"rgb {tag}")
        assert_close(lab_a, l32, l64, f"lab {tag}")
        assert torch.equal(lab_a, lab_b), f"{tag}: lab_a and lab_b differ"
        if got is not None:                                   # the byte / scalar paths and the vector paths: the same bits
            assert torch.equal(rgb, got[0]) and torch.equal(lab_a, got[1]), f"{tag}: differs from the other alignment"
        got = (rgb.clone(), lab_a.clone())
    return got


@pytest.mark.parametrize("fmt,shape", CASES, ids=CASE_IDS)
def test_decode_random_frames(fmt, shape, device):
    h, w = shape
    frame = np.random.default_rng(100 * h + w).integers(0, 256, YR.frame_bytes(h, w, fmt), dtype=np.uint8)
    check_decode(frame, h, w, fmt, device, [(1, 1), (0, 4)], "decode")


@pytest.mark.parametrize("fmt", YR.FORMATS_420 + YR.FORMATS_444, ids=YR.fmt_id)
def test_decode_all_256_values_in_each_plane_and_the_grey_ramp(fmt, device):
    h = w = 32 if fmt[0] == YR.S420 else 16                       # chroma planes of 256 samples
    y, cb, cr = (np.resize(np.roll(np.arange(256, dtype=np.uint8), s), n) for s, n in ((0, h * w), (85, 256), (171, 256)))
    frame = np.concatenate([y, cb, cr])
    for plane in YR.split(frame, h, w, fmt):
        assert len(np.unique(plane)) == 256
    check_decode(frame, h, w, fmt, device, [(1, 1), (0, 4)], "all values")
    # every grey byte: crosses both knees of the Lab formulas (the sRGB knee at 0.04045, the cube-root knee at 0.008856)
    grey = np.concatenate([y, np.full(512, 128, dtype=np.uint8)])
    check_decode(grey, h, w, fmt, device, [(0, 4)], "grey ramp")


@pytest.mark.parametrize("fmt", [f for f in YR.FORMATS_420 + YR.FORMATS_444], ids=YR.fmt_id)
def test_decode_out_of_gamut_corners_land_on_the_clamp_exactly(fmt, device):
    corners = [(0, 255, 255), (255, 0, 0), (0, 0, 0), (255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 255, 0), (255, 0, 255),
               (16, 16, 240), (235, 240, 16), (128, 255, 0), (128, 0, 255)]
    h, w = 4, 2 * len(corners)                                    # 2 x 2 luma blocks of one colour each, two rows of blocks
    y = np.zeros((h, w), dtype=np.uint8)
    c = np.zeros((2, h // 2, w // 2), dtype=np.uint8)
    for i, (yy, cb, cr) in enumerate(corners):
        y[:, 2 * i:2 * i + 2] = yy
        c[0, :, i], c[1, :, i] = cb, cr
    if fmt[0] == YR.S444:
        c = c.repeat(2, axis=1).repeat(2, axis=2)
    frame = np.concatenate([y.ravel(), c.ravel()])
    raw = YR.yuv_to_rgb(frame, h, w, fmt, np.float64, clamp=False)
    assert (raw < -0.01).any() and (raw > 1.01).any()
    for byte_off, float_off in ((1, 1), (0, 4)):
        _, fr = frame_in_guards(frame, byte_off, device)
        rgb = ops.yuv_to_rgb(fr, h, w, fmt, rgb=planes_in_guards(h, w, float_off, device)[1])[0].cpu().numpy()
        assert (rgb[raw < -1e-3] == 0.0).all() and (rgb[raw > 1 + 1e-3] == 1.0).all()
        assert rgb.min() >= 0.0 and rgb.max() <= 1.0


@pytest.mark.parametrize("fmt", ONE_PER_CLASS, ids=YR.fmt_id)
def test_decode_every_null_combination_but_all_null(fmt, device):
    h, w = 6, 10
    frame_np = np.random.default_rng(5).integers(0, 256, YR.frame_bytes(h, w, fmt), dtype=np.uint8)
    _, frame = frame_in_guards(frame_np, 1, device)
    full = ops.yuv_to_rgb(frame, h, w, fmt, rgb=True, lab=(True, True))
    assert all(t is not None and t.shape == (3, h, w) for t in full)
    for mask in range(1, 8):
        bufs = [planes_in_guards(h, w, 1, device) if mask >> i & 1 else None for i in range(3)]
        views = [b[1] if b else None for b in bufs]
        out = ops.yuv_to_rgb(frame, h, w, fmt, rgb=views[0], lab=(views[1], views[2]))
        for i in range(3):
            if bufs[i] is None:
                assert out[i] is None
            else:
                assert torch.equal(out[i], full[i]), (mask, i)
                assert_untouched(bufs[i][0], bufs[i][1], what=f"mask {mask} output {i}")
    with pytest.raises(VfiLibraryError, match="NULL"):
        ops.yuv_to_rgb(frame, h, w, fmt)                              # nothing wanted


def check_encode(x_np, fmt, device, what):
    h, w = x_np.shape[1:]
    want, near, tol = YR.expected_bytes(x_np, fmt)
    share = float(near.mean())
    print(f"{what}: {int(near.sum())} of {near.size} bytes within {tol:.2e} of a tie")
    assert share <= MAX_TIE_SHARE, f"{what}: {share:.2%} of the bytes are near ties: the case would excuse too much"
    got = None
    for byte_off, float_off in ((1, 1), (0, 4)):
        flat = canary_buffer(3 * h * w + float_off + 7, device)
        x = fview(flat, (3, h, w), float_off)
        x.copy_(torch.from_numpy(x_np))
        store, out = frame_in_guards(np.full(len(want), GUARD, dtype=np.uint8), byte_off, device)
        assert ops.rgb_to_yuv(x, fmt, out=out) is out
        tag = f"{what} frame+{byte_off} planes+{float_off}"
        assert_guards(store, out, tag)
        assert torch.equal(x.cpu(), torch.from_numpy(x_np)) or np.isnan(x_np).any()
        b = out.cpu().numpy()
        diff = np.abs(b.astype(np.int64) - want.astype(np.int64))
        assert (diff[~near] == 0).all(), f"{tag}: {int((diff[~near] != 0).sum())} bytes away from a tie differ, first at {np.nonzero(diff * ~near)[0][:5]}"
        assert (diff <= 1).all(), f"{tag}: a near-tie byte differs by {diff.max()}"
        lo, hi = YR.limits(h, w, fmt)
        assert (b >= lo).all() and (b <= hi).all(), f"{tag}: a byte outside the range's limits"
        again = torch.full_like(out, GUARD)
        ops.rgb_to_yuv(x, fmt, out=again)
        assert torch.equal(again, out), f"{tag}: a repeated call gives other bits"
        if got is not None:
            assert torch.equal(out, got), f"{tag}: differs from the other alignment"
        got = out.clone()
    return got.cpu().numpy()


@pytest.mark.parametrize("fmt,shape", CASES, ids=CASE_IDS)
def test_encode_random_frames(fmt, shape, device):
    h, w = shape
    check_encode(YR.encode_input(h, w, 300000 + 1000 * h + w), fmt, device, "encode")


@pytest.mark.parametrize("fmt", YR.FORMATS_420 + YR.FORMATS_444, ids=YR.fmt_id)
def test_encode_nan_gives_the_lower_limit(fmt, device):
    h, w = 6, 18
    x = YR.encode_input(h, w, 300000 + 1000 * h + w)
    x[:, 3, 7] = np.nan                                               # a whole pixel
    x[0, 0, 0] = np.nan                                               # one channel: everything it reaches
    x[2, 5, 17] = np.nan
    got = check_encode(x, fmt, device, "nan")
    lo, _ = YR.limits(h, w, fmt)
    yb, cbb, crb = YR.split(got, h, w, fmt)
    ylo, clo = lo[0], lo[-1]
    assert yb[3, 7] == ylo and yb[0, 0] == ylo and yb[5, 17] == ylo
    d = 2 if fmt[0] == YR.S420 else 1
    for plane in (cbb, crb):
        assert plane[3 // d, 7 // d] == clo and plane[0, 0] == clo and plane[5 // d, 17 // d] == clo


def test_decode_of_encode_round_trip_stays_within_one_code(device):
    """both kernels together, 4:4:4 full range: rgb -> bytes -> rgb returns within one code (plus the matrix's gain on it)"""
    fmt = (YR.S444, YR.CENTRE, YR.BT709, YR.FULL)
    x = torch.from_numpy(YR.encode_input(16, 24, 1)).to(device).clamp_(0, 1)
    back = ops.yuv_to_rgb(ops.rgb_to_yuv(x, fmt), 16, 24, fmt, rgb=True)[0]
    assert float((back - x).abs().max()) <= 2.5 / 255                 # |dR| <= |dy| + 2 (1 - Kr) |dcr| <= (0.5 + 0.79) / 255


def test_refusals_leave_the_outputs_alone(device):
    h, w = 6, 10
    f420, f444 = (0, 0, 0, 0), (1, 0, 0, 0)
    frame = torch.zeros(YR.frame_bytes(h, w, f420), dtype=torch.uint8, device=device)

    def dec_refused(frame, hh, ww, fmt, **kw):
        rgb = torch.full((3, hh, ww), float("nan"), device=device)
        la, lb = torch.full_like(rgb, float("nan")), torch.full_like(rgb, float("nan"))
        with pytest.raises(VfiLibraryError):
            ops.yuv_to_rgb(frame, hh, ww, fmt, rgb=kw.get("rgb", rgb), lab=(la, lb))
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (rgb, la, lb))
    dec_refused(torch.zeros(5 * 7 + 2 * 2 * 3, dtype=torch.uint8, device=device), 5, 7, f420)      # odd sizes in 4:2:0
    dec_refused(torch.zeros(6 * 7 + 2 * 3 * 3, dtype=torch.uint8, device=device), 6, 7, f420)
    for bad in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2), (0, 0, 0, -1)):
        dec_refused(frame, h, w, bad)
    dec_refused(frame, h, w, (0, 0, 0))                                # three integers
    dec_refused(frame[:-1], h, w, f420)                                # a byte short
    dec_refused(frame.float(), h, w, f420)
    dec_refused(frame.cpu(), h, w, f420)
    dec_refused(frame, h, w, f420, rgb=torch.zeros((3, h, w + 1), device=device))
    dec_refused(frame, h, w, f420, rgb=torch.zeros((3, h, w), device=device, dtype=torch.float64))
    dec_refused(frame, 0, w, f420)

    def enc_refused(x, fmt, n):
        out = torch.full((n,), GUARD, dtype=torch.uint8, device=device)
        with pytest.raises(VfiLibraryError):
            ops.rgb_to_yuv(x, fmt, out=out)
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
    x = torch.rand((3, h, w), device=device)
    n = YR.frame_bytes(h, w, f420)
    enc_refused(torch.rand((3, 5, 10), device=device), f420, 50 + 2 * 2 * 5)
    enc_refused(torch.rand((3, 6, 9), device=device), f420, 54 + 2 * 3 * 4)
    for bad in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
        enc_refused(x, bad, n)
    enc_refused(x, f420, n - 1)
    enc_refused(x, f444, n)                                            # a 4:2:0-sized buffer for a 4:4:4 frame
    enc_refused(x.double(), f420, n)
    enc_refused(x.cpu(), f420, n)
    enc_refused(x[:2], f420, n)
    # the accepted calls still run
    assert ops.rgb_to_yuv(x, f420).numel() == n and ops.rgb_to_yuv(torch.rand((3, 5, 7), device=device), f444).numel() == 105
    assert bool(torch.isfinite(ops.yuv_to_rgb(frame, h, w, f420, rgb=True)[0]).all())
