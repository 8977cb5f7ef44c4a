"""`vfi_triplet_batch_prepare` / `ops.triplet_batch_prepare`: decoded uint8 triplets -> the rgb and
Lab tensors of a training step, in one launch.

rgb is held bit for bit: `torch.equal` with `uint8.float() / 255` of the numpy restatement of the geometry
(train_batch_ref.prepare_ref).  Lab is held to `ops.rgb2lab`'s own rule (tests/test_image_ops_gpu.py): against the float64
restatement of oracle.color_cpu.rgb2lab_single, within glue_ref.tol_of(float32 restatement, float64 restatement)."""
import numpy as np
import pytest
import torch

import train_batch_ref as TR
from glue_ref import assert_close, assert_untouched, canary_buffer, fview
from oracle import color_cpu
from vfi_amd import ops
from vfi_amd._lib import VfiLibraryError
from vfi_amd.train.utils import preprocess

pytestmark = pytest.mark.gpu

HS, WS = 9, 13                                     # odd width: rows of 39 bytes
# (h, w, i, j)
CROPS = {"5x7-origin": (5, 7, 0, 0), "5x7-far-corner": (5, 7, 4, 6), "5x7-inside": (5, 7, 2, 3), "whole-frame": (9, 13, 0, 0),
         "1x1": (1, 1, 3, 5), "5x8-vector-width-unaligned-start": (5, 8, 1, 1)}


def _source(b, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (b, 3, HS, WS, 3), dtype=np.uint8)


def _run(src, params, h, w, device, **kw):
    return ops.triplet_batch_prepare(torch.from_numpy(src).to(device), torch.as_tensor(params, dtype=torch.int32).reshape(-1, 3),
                                     (h, w), **kw)


def test_rgb_is_uint8_over_255_bit_for_bit_for_all_256_values(device):
    src = np.zeros((1, 3, 16, 16, 3), dtype=np.uint8)
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for f in range(3):
        for c in range(3):
            src[0, f, :, :, c] = np.roll(v.reshape(-1), 85 * c + 7 * f).reshape(16, 16)      # every value in every channel position
    for f in range(3):
        for c in range(3):
            assert len(np.unique(src[0, f, :, :, c])) == 256
    rgb, lab = _run(src, [[0, 0, 0]], 16, 16, device)
    want = torch.from_numpy(src).float() / 255                                  # (1, 3 frames, 16, 16, 3)
    want = want[0].permute(0, 3, 1, 2)[[0, 2, 1]].unsqueeze(1)                  # slots [first, last, middle], (3, 1, 3, 16, 16)
    assert rgb.shape == (3, 1, 3, 16, 16) and rgb.dtype == torch.float32
    assert torch.equal(rgb.cpu(), want)
    assert lab.shape == (3, 3, 16, 16)


def _check_lab(lab, want_u8, what):
    ref64, ref32 = TR.lab_slots(want_u8, np.float64), TR.lab_slots(want_u8, np.float32)
    return assert_close(lab, ref32, ref64, what)


@pytest.mark.parametrize("crop", list(CROPS))
@pytest.mark.parametrize("b", [1, 3])
def test_geometry_and_lab(crop, b, device):
    h, w, i, j = CROPS[crop]
    src = _source(b, seed=h * w + b)
    srcd = torch.from_numpy(src).to(device)
    for flags in range(8):
        # different parameters per sample: flags rotate, the crop of samples 1, 2 moves where the frame has room
        params = np.array([[min(i + n, HS - h), max(j - n, 0), (flags + 3 * n) % 8] for n in range(b)], dtype=np.int32)
        rgb, lab = ops.triplet_batch_prepare(srcd, torch.from_numpy(params), (h, w))
        want_u8 = TR.prepare_ref(src, params, h, w)
        assert rgb.shape == (3, b, 3, h, w) and lab.shape == (3, 3 * b, h, w)
        assert torch.equal(rgb.cpu(), TR.to_float(want_u8)), (crop, b, flags)
        _check_lab(lab, want_u8, f"lab {crop} B={b} flags={flags}")
        # lab viewed as (9B, h, w) is the reference's torch.cat of preprocess of the three slots (trainer.py:103, :115-117)
        cat = torch.cat([preprocess(rgb[s], device) for s in range(3)], 0)
        ref64, ref32 = TR.lab_slots(want_u8, np.float64).reshape(9 * b, h, w), TR.lab_slots(want_u8, np.float32).reshape(9 * b, h, w)
        assert_close(lab.view(9 * b, h, w), ref32, ref64, "lab.view(9B,h,w)")
        assert_close(cat, ref32, ref64, "cat(preprocess(rgb slots))")


def test_lab_restatement_is_the_oracles():
    u8 = TR.prepare_ref(TR.threshold_source(), [[0, 0, 0]], 6, 8)
    rgb = TR.to_float(u8).reshape(3, 3, 6, 8)
    ref64 = TR.lab_restated(rgb, np.float64)
    for n in range(3):
        assert torch.equal(ref64[n].float(), color_cpu.rgb2lab_single(rgb[n]))


@pytest.mark.parametrize("flags", [0, 3, 5])
def test_lab_at_both_thresholds(flags, device):
    src = TR.threshold_source()
    for (h, w, i, j) in ((6, 8, 0, 0), (5, 7, 1, 1)):
        params = np.array([[i, j, flags]], dtype=np.int32)
        rgb, lab = _run(src, params, h, w, device)
        want_u8 = TR.prepare_ref(src, params, h, w)
        assert torch.equal(rgb.cpu(), TR.to_float(want_u8))
        _check_lab(lab, want_u8, f"lab thresholds {h}x{w} flags={flags}")


@pytest.mark.parametrize("h,w,offset,pad", [(5, 8, 0, 0), (5, 8, 3, 0), (5, 8, 4, 8), (5, 8, 2, 5), (5, 7, 1, 3)])
def test_slices_and_null_outputs(h, w, offset, pad, device):
    """Both outputs inside canary buffers: at an offset of `offset` floats (3, 2, 1: not a multiple of 4, so no float4
    stores) and with `pad` floats between samples and slots (a batch stride wider than the sample)."""
    b = 2
    src = _source(b, seed=offset + pad)
    params = np.array([[1, 2, 5], [3, 0, 2]], dtype=np.int32)
    want_u8 = TR.prepare_ref(src, params, h, w)
    block = 3 * h * w
    sb = block + pad                                         # sample stride
    ss = b * sb + pad                                        # slot stride
    strides = (ss, sb, h * w, w, 1)

    def outputs():
        flat_r, flat_l = canary_buffer(3 * ss + offset + 5, device), canary_buffer(3 * ss + offset + 5, device)
        return flat_r, fview(flat_r, (3, b, 3, h, w), offset, strides), flat_l, fview(flat_l, (3, b, 3, h, w), offset, strides)
    flat_r, rgb, flat_l, lab = outputs()
    got_r, got_l = _run(src, params, h, w, device, rgb=rgb, lab=lab)
    assert got_r is rgb and got_l is lab
    assert_untouched(flat_r, rgb, what="rgb slice")
    assert_untouched(flat_l, lab, what="lab slice")
    assert torch.equal(rgb.cpu(), TR.to_float(want_u8))
    _check_lab(lab.reshape(3, 3 * b, h, w), want_u8, f"lab slice offset {offset} pad {pad}")
    # one output NULL: the other keeps its bits, and nothing else is written
    flat_r2, rgb2, flat_l2, lab2 = outputs()
    only_r, none_l = _run(src, params, h, w, device, rgb=rgb2, lab=None)
    assert none_l is None and torch.equal(rgb2, rgb)
    assert_untouched(flat_r2, rgb2, what="rgb alone")
    none_r, only_l = _run(src, params, h, w, device, rgb=None, lab=lab2)
    assert none_r is None and torch.equal(lab2, lab)
    assert_untouched(flat_l2, lab2, what="lab alone")
    # and the dense new tensors hold the same bits as the slices
    dense_r, dense_l = _run(src, params, h, w, device)
    assert torch.equal(dense_r, rgb) and torch.equal(dense_l.view(3, b, 3, h, w), lab)


def test_refusals_leave_the_outputs_alone(device):
    b, h, w = 2, 5, 7
    src = torch.from_numpy(_source(b)).to(device)
    ok = [[0, 0, 0], [4, 6, 7]]

    def refused(src, params, size=(h, w), **kw):
        rgb = torch.full((3, b, 3, size[0], size[1]), float("nan"), device=device)
        lab = torch.full((3, 3 * b, size[0], size[1]), float("nan"), device=device)
        with pytest.raises(VfiLibraryError):
            ops.triplet_batch_prepare(src, torch.tensor(params, dtype=torch.int32), size, rgb=rgb, lab=lab, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(rgb).all()) and bool(torch.isnan(lab).all())
    refused(src, [[0, 0, 0], [5, 6, 0]])                     # i + h > Hs (second sample: the first alone would pass)
    refused(src, [[0, 7, 0], [0, 0, 0]])                     # j + w > Ws
    refused(src, [[0, 0, 8], [0, 0, 0]])                     # flags = 8
    refused(src, [[-1, 0, 0], [0, 0, 0]])
    refused(src, ok, size=(10, 7))                           # crop taller than the source
    refused(src.float(), ok)                                 # a float src
    refused(src.cpu(), ok)                                   # a CPU tensor
    rgb, lab = ops.triplet_batch_prepare(src, torch.tensor(ok, dtype=torch.int32), (h, w))     # the accepted call still runs
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(lab).all())


def test_a_batch_beyond_one_launch_of_64_samples(device):
    b, h, w = 70, 4, 8
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (b, 3, 6, 11, 3), dtype=np.uint8)
    params = np.stack([rng.integers(0, 3, b), rng.integers(0, 4, b), rng.integers(0, 8, b)], 1).astype(np.int32)
    rgb, lab = _run(src, params, h, w, device)
    want_u8 = TR.prepare_ref(src, params, h, w)
    assert torch.equal(rgb.cpu(), TR.to_float(want_u8))
    _check_lab(lab, want_u8, "lab B=70")
