"""GPU parity of the image-space stages (Lab, Gaussian, median, glue) against scipy (which the reference
calls directly) and the oracle's Lab restatement."""
import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter, median_filter

from oracle import color_cpu
from vfi_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h,w", [(96, 128), (37, 61), (20, 200)])
def test_gaussian_matches_scipy(h, w, device):
    rng = np.random.default_rng(h)
    x = rng.random((2, h, w), dtype=np.float32)
    ref = np.stack([gaussian_filter(a, 5) for a in x])
    got = ops.gaussian_filter(torch.from_numpy(x).to(device), 5).cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=2e-6)


@pytest.mark.parametrize("h,w,size", [(96, 128, 50), (64, 72, 50), (30, 41, 50), (40, 40, 7), (33, 65, 4)])
def test_median_matches_scipy_exactly(h, w, size, device):
    rng = np.random.default_rng(w)
    x = (rng.standard_normal((1, h, w)) * 3).astype(np.float32)
    x[0, :5, :7] = 0.25                       # ties
    x[0, 10:14, :] = -0.0
    ref = np.stack([median_filter(a, size=size) for a in x])
    got = ops.median_filter(torch.from_numpy(x).to(device), size).cpu().numpy()
    assert np.array_equal(got, ref)          # a selection: bit exact


def test_median_smooth_map_1080p_window(device):
    # the real input is a smooth low-frequency map; check a crop of a 1080p launch against scipy
    h, w = 1080, 1920
    yy, xx = np.meshgrid(np.linspace(0, 6, h), np.linspace(0, 9, w), indexing="ij")
    x = (np.sin(yy) * np.cos(xx) + 0.1 * np.sin(7 * xx)).astype(np.float32)[None]
    got = ops.median_filter(torch.from_numpy(x).to(device), 50).cpu().numpy()
    ref = median_filter(x[0, :160, :200], size=50)
    assert np.array_equal(got[0, :100, :100], ref[:100, :100])   # interior of the crop unaffected by its border


def test_lab_matches_oracle_and_round_trips(device):
    rng = np.random.default_rng(0)
    rgb = rng.random((3, 48, 64), dtype=np.float32)
    rgb[:, 0, 0] = 0.0; rgb[:, 0, 1] = 1.0; rgb[:, 0, 2] = 0.04045; rgb[:, 0, 3] = 0.003
    t = torch.from_numpy(rgb)
    lab = ops.rgb2lab(t.to(device))
    np.testing.assert_allclose(lab.cpu().numpy(), color_cpu.rgb2lab_single(t).numpy(), atol=2e-6)
    back = ops.lab2rgb(lab)
    np.testing.assert_allclose(back.cpu().numpy(), rgb, atol=2e-5)
    # out-of-gamut Lab (as PhaseNet produces) clips like the oracle
    wild = torch.from_numpy((rng.random((3, 32, 32), dtype=np.float32) * 1.4 - 0.2))
    np.testing.assert_allclose(ops.lab2rgb(wild.to(device)).cpu().numpy(), color_cpu.lab2rgb_single(wild).numpy(), atol=3e-5)


def test_glue_ops(device):
    rng = np.random.default_rng(1)
    a = torch.from_numpy(rng.standard_normal((1, 3, 20, 30)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal((1, 3, 20, 30)).astype(np.float32))
    got = ops.channel_mean_diff(a.to(device), b.to(device), 100.0, True).cpu()
    ref = ((a.mean(1) - b.mean(1)).abs() * 100).clamp(0, 1)
    assert (got - ref).abs().max().item() <= 1e-4
    got = ops.channel_mean_diff(a.to(device), None, 30.0, False).cpu()
    assert (got - a.mean(1) * 30).abs().max().item() <= 1e-5
    got = ops.absdiff(a.to(device), b.to(device), 5.0, True).cpu()
    assert (got - ((a - b).abs() * 5).clamp(0, 1)).abs().max().item() <= 1e-6


@pytest.mark.parametrize("hi,wi,ho,wo,ac,relu", [(9, 15, 12, 20, False, False), (12, 20, 17, 29, False, False),
                                                 (10, 12, 20, 24, True, False), (8, 12, 16, 24, False, True),
                                                 (6, 11, 8, 15, False, False),
                                                 # >= 16 x 64 outputs, up-scaling: the LDS-staged tile kernel (float4 rows /
                                                 # ragged rows, several tiles in both directions, relu + residual)
                                                 (40, 70, 80, 140, True, False), (33, 45, 47, 66, False, False),
                                                 (20, 40, 40, 80, False, True), (100, 300, 200, 600, True, True),
                                                 (54, 96, 77, 135, False, False), (16, 64, 16, 64, True, False),
                                                 # down-scaling (scalar and float4 kernels) and rows up / columns down
                                                 (20, 30, 9, 13, False, False), (20, 30, 9, 13, True, False),
                                                 (16, 64, 8, 32, False, False), (16, 64, 8, 32, True, False),
                                                 (12, 40, 24, 20, False, False), (12, 40, 24, 20, True, True),
                                                 # output extents of 1 with align_corners (source step 0)
                                                 (5, 7, 1, 1, True, False), (5, 7, 1, 12, True, False),
                                                 # a single pixel / a single row into the tile kernel
                                                 (1, 1, 16, 64, False, False), (1, 1, 16, 64, True, False),
                                                 (1, 9, 16, 64, False, False),
                                                 # tile boundaries: a third 256-column tile of 3 columns, a second one of 2
                                                 # and of 1, a third 16-row tile of one row
                                                 (20, 150, 33, 515, False, False), (16, 130, 16, 258, True, False),
                                                 (17, 129, 32, 257, False, False), (16, 64, 16, 64, True, True)])
def test_resize_bilinear_matches_torch(hi, wi, ho, wo, ac, relu, device):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(hi * wo)
    x = torch.randn((2, 5, hi, wi), generator=g)
    res = torch.randn((2, 5, ho, wo), generator=g)
    ref = F.interpolate(F.relu(x) if relu else x, size=(ho, wo), mode="bilinear", align_corners=ac) + res
    got = ops.resize_bilinear(x.to(device), (ho, wo), align_corners=ac, relu_input=relu, residual=res.to(device))
    assert (got.cpu() - ref).abs().max().item() <= 2e-6
    # into a channel slice of a wider tensor (PhaseNet block input)
    wide = torch.zeros((2, 9, ho, wo), device=device)
    ops.resize_bilinear(x.to(device), (ho, wo), align_corners=ac, relu_input=relu, out=wide[:, 2:7])
    ref2 = F.interpolate(F.relu(x) if relu else x, size=(ho, wo), mode="bilinear", align_corners=ac)
    assert (wide[:, 2:7].cpu() - ref2).abs().max().item() <= 2e-6 and wide[:, :2].abs().max().item() == 0


# ---- edge shapes of the Gaussian, Lab and difference kernels (tolerances and canaries: tests/glue_ref.py) -------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 40), (37, 1), (7, 9), (5, 64), (19, 21)])
def test_gaussian_on_images_smaller_than_the_radius(h, w, device):
    # sigma 5 -> radius 20: the reflection wraps more than once along every extent below 20; three images per call
    rng = np.random.default_rng(100 * h + w)
    x = rng.random((3, h, w), dtype=np.float32)
    ref = np.stack([gaussian_filter(a, 5) for a in x])
    got = ops.gaussian_filter(torch.from_numpy(x).to(device), 5).cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=2e-6)


@pytest.mark.parametrize("sigma,truncate", [(1.0, 4.0), (2.5, 2.0), (16.0, 4.0)])      # radius 4, 5 and 64 (the cap)
def test_gaussian_sigma_and_truncate(sigma, truncate, device):
    rng = np.random.default_rng(int(sigma * 10))
    x = rng.random((3, 40, 50), dtype=np.float32)
    ref = np.stack([gaussian_filter(a, sigma, truncate=truncate) for a in x])
    got = ops.gaussian_filter(torch.from_numpy(x).to(device), sigma, truncate).cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=2e-6)


def test_gaussian_into_a_slice_and_the_radius_cap(device):
    from glue_ref import assert_untouched, nan_wide
    from vfi_amd._lib import VfiLibraryError
    rng = np.random.default_rng(7)
    x = rng.random((3, 19, 21), dtype=np.float32)
    flat, wide = nan_wide((5, 19, 21), device)
    out = wide[1:4]
    assert ops.gaussian_filter(torch.from_numpy(x).to(device), 5, out=out) is out
    assert_untouched(flat, out, what="gaussian_filter out slice")
    np.testing.assert_allclose(out.cpu().numpy(), np.stack([gaussian_filter(a, 5) for a in x]), atol=2e-6)
    with pytest.raises(VfiLibraryError):
        ops.gaussian_filter(torch.from_numpy(x).to(device), 16.2, 4.0)          # radius 65


def _lab_restated(rgb, dtype):
    """oracle.color_cpu.rgb2lab_single's formulas for (N,3,H,W), every step in `dtype` (float32: the tolerance's ref32)."""
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


def _lab_edge_images():
    """(2,3,7,9) in [0,1): random, with greys and single channels at and around the two thresholds of rgb2lab."""
    rng = np.random.default_rng(11)
    rgb = rng.random((2, 3, 7, 9), dtype=np.float32)
    one = np.float32(1.0)
    t = np.float32(0.04045)
    around = [np.nextafter(t, -one), t, np.nextafter(t, one)]
    for k, v in enumerate(around):
        rgb[0, :, 0, k] = v                       # grey at the sRGB knee
        rgb[0, k, 0, 3 + k] = v                   # one channel at the knee
    # grey v with linear value (= Y, the matrix row sums to 1) at 0.008856: v = 1.055 Y^(1/2.4) - 0.055, +-3 float32 steps
    v0 = np.float32(1.055 * 0.008856 ** (1 / 2.4) - 0.055)
    v = v0
    for _ in range(3):
        v = np.nextafter(v, -one)
    for k in range(7):
        rgb[1, :, 1, k] = v
        v = np.nextafter(v, one)
    return torch.from_numpy(rgb)


def test_lab_batched_thresholds_and_out_slices(device):
    from glue_ref import assert_close, assert_untouched, nan_wide
    rgb = _lab_edge_images()
    ref64, ref32 = _lab_restated(rgb, np.float64), _lab_restated(rgb, np.float32)
    for i in range(2):      # the restatement is the oracle's
        assert torch.equal(ref64[i].float(), color_cpu.rgb2lab_single(rgb[i]))
    got = ops.rgb2lab(rgb.to(device))
    assert got.shape == (2, 3, 7, 9)
    assert_close(got, ref32, ref64, "rgb2lab batched (2,3,7,9)")
    # two frames into the halves of one (6,H,W) buffer, as the fused path fills lab12
    flat, wide = nan_wide((8, 7, 9), device)
    lab12 = wide[1:7]
    ops.rgb2lab(rgb[0].to(device), out=lab12[:3])
    assert_untouched(flat, lab12[:3], what="rgb2lab out=lab12[:3]")
    ops.rgb2lab(rgb[1].to(device), out=lab12[3:])
    assert_untouched(flat, lab12, what="rgb2lab out=lab12[3:]")
    assert_close(lab12.reshape(2, 3, 7, 9), ref32, ref64, "rgb2lab into lab12 slices")
    assert torch.equal(lab12.reshape(2, 3, 7, 9), got)


def _mean_diff_ref(a, b, scale, clamp, signed):
    v = a.mean(1)
    if b is not None:
        v = v - b.mean(1)
        if not signed:
            v = v.abs()
    v = v * scale
    return v, (v.clamp(0, 1) if clamp else v)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("mode", ["abs", "signed", "single"])
@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_channel_mean_diff_modes(c, mode, clamp, device):
    from glue_ref import assert_close
    g = torch.Generator().manual_seed(10 * c + len(mode))
    a = torch.randn((2, c, 7, 9), generator=g)
    b = None if mode == "single" else torch.randn((2, c, 7, 9), generator=g)
    if b is not None:
        b[0, :, 0, 0] = a[0, :, 0, 0]               # difference exactly 0
    scale, signed = 1.5, mode == "signed"
    got = ops.channel_mean_diff(a.to(device), None if b is None else b.to(device), scale, clamp, signed=signed).cpu()
    pre64, ref64 = _mean_diff_ref(a.double(), None if b is None else b.double(), scale, clamp, signed)
    _, ref32 = _mean_diff_ref(a, b, scale, clamp, signed)
    assert got.shape == (2, 7, 9)
    assert_close(got, ref32, ref64, f"channel_mean_diff C={c} {mode} clamp={clamp}")
    if clamp:
        lo, hi = pre64 < 0, pre64 > 1
        assert hi.any() and (lo.any() or mode == "abs")        # both ends occur (|.| has no negative side)
        assert (got[lo] == 0.0).all() and (got[hi] == 1.0).all()
        if b is not None:
            assert got[0, 0, 0].item() == 0.0
    elif mode != "abs":
        assert (got < 0).any()                      # signed values pass through


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("count", [1, 3, 1023])
def test_absdiff_counts_without_y_and_into_a_slice(count, with_y, clamp, device):
    from glue_ref import assert_close, assert_untouched, nan_wide
    g = torch.Generator().manual_seed(count + 2 * with_y)
    x = torch.randn((1, 1, count), generator=g)
    y = torch.randn((1, 1, count), generator=g) if with_y else None
    if count == 1:
        x[...] = -0.75 if clamp else 0.1            # scaled: 2.25 (clamps) / 0.3
    scale = 3.0
    pre64 = ((x.double() - y.double()) if with_y else x.double()).abs() * scale
    ref64 = pre64.clamp(0, 1) if clamp else pre64
    ref32 = ((x - y) if with_y else x).abs() * scale
    ref32 = ref32.clamp(0, 1) if clamp else ref32
    flat, wide = nan_wide((3, 1, count), device)
    for out in (None, wide[1:2]):
        got = ops.absdiff(x.to(device), None if y is None else y.to(device), scale, clamp, out=out)
        if out is not None:
            assert got is out
            assert_untouched(flat, out, what="absdiff out slice")
        assert_close(got, ref32, ref64, f"absdiff count={count} y={with_y} clamp={clamp}")
        if clamp:
            hi = pre64 > 1
            assert hi.any() or count == 3 or with_y
            assert (got.cpu()[hi] == 1.0).all()
