"""The default median path (median_walk_kernel) against the bisection kernel and scipy; VFI_MEDIAN_PATH is read at every
call, so both paths run in one process."""
import numpy as np
import pytest
import torch
from scipy.ndimage import median_filter

from vfi_amd import ops

pytestmark = pytest.mark.gpu


def run(x, size, path, monkeypatch, device):
    monkeypatch.setenv("VFI_MEDIAN_PATH", path)
    out = ops.median_filter(torch.from_numpy(np.ascontiguousarray(x)).to(device), size).cpu().numpy()
    torch.cuda.synchronize()
    return out


def smooth_map(h, w):
    yy, xx = np.meshgrid(np.linspace(0, 6, h), np.linspace(0, 9, w), indexing="ij")
    return (np.sin(yy) * np.cos(xx) + 0.1 * np.sin(7 * xx)).astype(np.float32)[None]


@pytest.mark.parametrize("h,w", [(1080, 1920), (720, 1280)])
def test_walk_equals_bisection_full_frame(h, w, monkeypatch, device):
    rng = np.random.default_rng(h)
    x = smooth_map(h, w) + (rng.standard_normal((1, h, w)) * 0.05).astype(np.float32)
    x[0, 100:140, 300:700] = 0.5                                  # a plateau of ties
    new = run(x, 50, "walk", monkeypatch, device)
    old = run(x, 50, "bisect", monkeypatch, device)
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))


def test_walk_matches_scipy_on_1080p_corners_and_interior(monkeypatch, device):
    h, w, c = 1080, 1920, 160
    x = smooth_map(h, w)
    got = run(x, 50, "walk", monkeypatch, device)[0]
    # a crop's border is reflected by scipy: compare only outputs whose window stays inside the crop, or touches the
    # image edge the crop shares with the frame
    for ys, xs in ((slice(0, c), slice(0, c)), (slice(0, c), slice(w - c, w)), (slice(h - c, h), slice(0, c)),
                   (slice(h - c, h), slice(w - c, w)), (slice(460, 460 + c), slice(880, 880 + c))):
        ref = median_filter(x[0, ys, xs], size=50)
        y_in = slice(0 if ys.start == 0 else 25, c - 25 if ys.stop != h else c)
        x_in = slice(0 if xs.start == 0 else 25, c - 25 if xs.stop != w else c)
        assert np.array_equal(got[ys, xs][y_in, x_in], ref[y_in, x_in]), (ys, xs)


@pytest.mark.parametrize("size", [2, 3, 4, 7, 16, 49, 50, 51, 64])
def test_walk_matches_scipy_sizes(size, monkeypatch, device):
    rng = np.random.default_rng(size)
    x = (rng.standard_normal((2, 150, 203)) * 3).astype(np.float32)
    x[0, :9, :13] = 0.25
    x[1, 20:24, :] = -0.0
    x[1, 30:33, :] = 0.0
    got = run(x, size, "walk", monkeypatch, device)
    ref = np.stack([median_filter(a, size=size) for a in x])
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("h,w", [(11, 17), (1, 40), (37, 1)])
def test_walk_image_smaller_than_window(h, w, monkeypatch, device):
    x = np.random.default_rng(h * w).standard_normal((1, h, w)).astype(np.float32)
    assert np.array_equal(run(x, 50, "walk", monkeypatch, device)[0], median_filter(x[0], size=50))


def test_walk_constant_and_heavy_ties(monkeypatch, device):
    x = np.full((1, 130, 140), 0.75, np.float32)
    assert np.array_equal(run(x, 50, "walk", monkeypatch, device), x)
    rng = np.random.default_rng(3)
    t = (rng.integers(-2, 3, (1, 130, 140)) * 0.5).astype(np.float32)
    t[rng.random(t.shape) < 0.3] = -0.0
    got = run(t, 50, "walk", monkeypatch, device)
    assert np.array_equal(got, median_filter(t[0], size=50)[None])
    assert np.array_equal(got.view(np.uint32), run(t, 50, "bisect", monkeypatch, device).view(np.uint32))


def test_median_paths_agree(monkeypatch, device):
    x = (np.random.default_rng(5).standard_normal((1, 200, 300)) * 2).astype(np.float32)
    outs = [run(x, 50, p, monkeypatch, device).view(np.uint32) for p in ("walk", "rank", "bisect")]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
