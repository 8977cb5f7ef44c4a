"""Scoring on device against plain torch-CPU statements of reference
src/evaluation/evaluate_image.py:22-28 and of piq's published psnr / ssim formulas."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scoring_ref as sr
from glue_ref import assert_close, assert_untouched, nan_wide
from vfi_amd import _lib
from vfi_amd._lib import VfiLibraryError
from vfi_amd.evaluation import evaluate_image as ei

pytestmark = pytest.mark.gpu


def _ssim_ref(x, y, ks=11, sigma=1.5, k1=0.01, k2=0.03):
    f = max(1, round(min(x.shape[-2:]) / 256))
    x, y = x.unsqueeze(0), y.unsqueeze(0)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    c = x.shape[1]
    co = torch.arange(ks, dtype=torch.float32) - ks // 2
    g = torch.exp(-co ** 2 / (2 * sigma ** 2)); g = g / g.sum()
    k = (g[:, None] * g[None, :]).expand(c, 1, ks, ks)
    conv = lambda t: F.conv2d(t, k, groups=c)
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    cs = (2 * sxy + k2 ** 2) / (sxx + syy + k2 ** 2)
    return float(((2 * mx * my + k1 ** 2) / (mx * mx + my * my + k1 ** 2) * cs).mean())


@pytest.mark.parametrize("dim", [96, 512])
def test_evaluate_image_matches_reference_expressions(dim, device):
    g = torch.Generator().manual_seed(dim)
    pred = torch.rand((3, dim + 8, dim + 8), generator=g)
    tgt = (pred + 0.05 * torch.randn((3, dim + 8, dim + 8), generator=g)).clamp(0, 1)
    got = ei.evaluate_image(types.SimpleNamespace(dim=dim), pred.to(device), tgt.to(device))
    c = lambda t: t[:, 4:4 + dim, 4:4 + dim]
    p, t = c(pred).double(), c(tgt).double()
    d = p - t
    assert abs(got[0] - _ssim_ref(c(pred), c(tgt))) <= 2e-5
    assert math.isnan(got[1])
    assert abs(got[2] - 10 * math.log10(1.0 / (float((d * d).mean()) + 1e-8))) <= 1e-6      # piq.psnr
    assert abs(got[3] - float(torch.sqrt((d * d).sum()))) <= 1e-6                              # ssd (evaluate_image.py:24)
    assert abs(got[4] - float(d.sum())) <= 1e-6 and abs(got[5] - float(d.mean())) <= 1e-9      # signed l1 / mse (:25-26)
    assert abs(got[6] - float(torch.var(d))) <= 1e-9                                           # :27


# ---- the five entry points alone, and ssim / psnr / evaluate_image on inputs with structure -----------------------------
# References, inputs, cases and bounds: tests/scoring_ref.py.  tests/test_scoring_host.py shows on the CPU that every SSIM
# and vfi_ssim_sum case below has a float32-vs-float64 gap of at most half its bound, and that a border off by one, a window
# shifted by one row or column, a pooling factor off by one and a transposed walk each move it by at least ten bounds.
SENT64 = 0x7FF80000DEADBEEF                  # a quiet double NaN with a payload
ONE_SWEEP = 1024 * 256                      # kRedBlocks blocks of 256 threads (csrc/vfi_image.hip)


def _dslice(device):
    """(buffer, out): `out` is doubles 2..3 of six sentinel doubles"""
    buf = torch.full((6,), SENT64, dtype=torch.int64, device=device)
    return buf, buf.view(torch.float64)[2:4]


def _dslice_intact(buf, written=True):
    keep = torch.cat([buf[:2], buf[4:]]) if written else buf
    return bool((keep == SENT64).all())


def _nan_ws(device):
    return torch.full((2048,), float("nan"), dtype=torch.float64, device=device)       # stale partials: never to be read


def _offset_copy(values, device):
    """`values` (1-D) one float past a 16-byte boundary, NaN canaries on both sides -> (flat, view)"""
    flat, wide = nan_wide((values.numel() + 8,), device, offset=1)
    view = wide[:values.numel()]
    view.copy_(values)
    assert view.data_ptr() % 16 == 4
    return flat, view


def _diff_sums(av, bv, device):
    fa, a = _offset_copy(av, device)
    fb, b = _offset_copy(bv, device)
    res = []
    for _ in range(2):
        buf, out = _dslice(device)
        _lib.call("vfi_diff_sums", a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), _nan_ws(device).data_ptr(),
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _dslice_intact(buf), "vfi_diff_sums wrote outside out[0..1]"
        res.append(out.cpu().clone())
    assert_untouched(fa, a, what="vfi_diff_sums a")
    assert_untouched(fb, b, what="vfi_diff_sums b")
    assert torch.equal(a.cpu(), av) and torch.equal(b.cpu(), bv)
    assert torch.equal(res[0].view(torch.int64), res[1].view(torch.int64)), "two calls, different bits"
    return float(res[0][0]), float(res[0][1])


@pytest.mark.parametrize("count", [1, 255, 256, 257, ONE_SWEEP - 1, ONE_SWEEP, ONE_SWEEP + 1, 3 * ONE_SWEEP + 1])
def test_diff_sums_counts(count, device):
    # integers: d in {1..8} by position, every partial sum exact, so a skipped or twice-added element shows in sum d
    i = torch.arange(count)
    d = 1 + (i * 5 + i // 256 + 3 * (i // ONE_SWEEP)) % 8
    b = ((i * 3) % 16).float()
    s1, s2 = _diff_sums(b + d.float(), b, device)
    assert s1 == int(d.sum()) and s2 == int((d * d).sum()), (s1, s2, int(d.sum()), int((d * d).sum()))
    # uniform data: only the order of the additions may differ from the exact sums
    g = torch.Generator().manual_seed(count)
    a, b = torch.rand(count, generator=g), torch.rand(count, generator=g)
    (r1, r2), (b1, b2) = sr.diff_sums_ref(a, b)
    s1, s2 = _diff_sums(a, b, device)
    print(f"count {count}: |s1 - ref| {abs(s1 - r1):.3e} (bound {b1:.3e})  |s2 - ref| {abs(s2 - r2):.3e} (bound {b2:.3e})")
    assert abs(s1 - r1) <= b1 and abs(s2 - r2) <= b2


@pytest.mark.parametrize("count", [1, 3, 1023, 4100, 16384 * 256 + 1])           # the last: one past blocks_1d's sweep
def test_mul_counts(count, device):
    g = torch.Generator().manual_seed(count)
    a, b = torch.randn(count, generator=g), torch.randn(count, generator=g)
    a[2::7] = 0.0                                                                # zeros (and -0 products)
    a[1::11] *= 1e-20                                                            # denormal products
    b[1::11] *= 1e-20
    want = a * b
    if count >= 1023:
        tiny = want[1::11].abs()
        assert bool(((tiny > 0) & (tiny < 2.0 ** -126)).any()) and bool((want < 0).any()) and bool((want == 0).any())
    fa, da = _offset_copy(a, device)
    fb, db = _offset_copy(b, device)
    flat, wide = nan_wide((count + 16,), device, offset=1)
    out = wide[8:8 + count]
    _lib.call("vfi_mul", da.data_ptr(), db.data_ptr(), out.data_ptr(), count, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert_untouched(flat, out, what="vfi_mul out")
    assert_untouched(fa, da, what="vfi_mul a")
    assert_untouched(fb, db, what="vfi_mul b")
    bad = int((out.cpu().view(torch.int32) != want.view(torch.int32)).sum())
    assert bad == 0, f"{bad} of {count} products differ from the float32 product"


def _avg_pool(x, f, device):
    p, h, w = x.shape
    fin, win = nan_wide((p + 2, h, w), device, offset=1)
    xin = win[1:p + 1]
    xin.copy_(x)
    flat, wide = nan_wide((p + 2, h // f, w // f), device, offset=1)
    out = wide[1:p + 1]
    _lib.call("vfi_avg_pool", xin.data_ptr(), out.data_ptr(), p, h, w, f, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert_untouched(flat, out, what="vfi_avg_pool out")
    assert_untouched(fin, xin, what="vfi_avg_pool x")
    assert torch.equal(xin.cpu(), x)
    return out.cpu()


@pytest.mark.parametrize("shape,f", [((1, 1, 1), 1), ((3, 7, 10), 3), ((2, 9, 8), 4), ((3, 5, 64), 5), ((1, 384, 385), 2),
                                     ((1, 2049, 2048), 1)])
def test_avg_pool_shapes(shape, f, device):
    g = torch.Generator().manual_seed(shape[1] * 7 + f)
    x = torch.rand(shape, generator=g)
    got = _avg_pool(x, f, device)
    assert_close(got, sr.avg_pool_ref(x, f, torch.float32), sr.avg_pool_ref(x, f, torch.float64), f"avg_pool {shape} f {f}")
    if f in (1, 2, 4):                                   # multiples of 2^-8: every sum and the scaling are exact
        x = torch.randint(0, 257, shape, generator=g).float() / 256
        assert torch.equal(_avg_pool(x, f, device).double(), sr.avg_pool_ref(x, f, torch.float64))


def _ssim_sum(case, device):
    """vfi_ssim_sum on the case's maps, everything outside the valid interior NaN -> (out[0], out[1])"""
    p, h, w = case["maps"][0].shape
    b = case["border"]
    dev = []
    for m in case["maps"]:
        _, wide = nan_wide((p + 2, h, w), device, offset=1)
        wide[1:p + 1, b:h - b, b:w - b] = m[:, b:h - b, b:w - b].to(device)
        dev.append(wide[1:p + 1])
    res = []
    for _ in range(2):
        buf, out = _dslice(device)
        _lib.call("vfi_ssim_sum", *(m.data_ptr() for m in dev), p, h, w, b, case["c1"], case["c2"], out.data_ptr(),
                  _nan_ws(device).data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _dslice_intact(buf), "vfi_ssim_sum wrote outside out[0..1]"
        res.append(out.cpu().clone())
    assert torch.equal(res[0].view(torch.int64), res[1].view(torch.int64)), "two calls, different bits"
    return float(res[0][0]), float(res[0][1])


@pytest.mark.parametrize("j", range(len(sr.C_PAIRS)))
@pytest.mark.parametrize("i", range(len(sr.SUM_CASES)), ids=[sr.case_id(c) for c in sr.SUM_CASES])
def test_ssim_sum_shapes(i, j, device):
    case = sr.sum_case(i, j)
    got, second = _ssim_sum(case, device)
    err = abs(got - case["ref64"])
    print(f"ssim_sum {sr.case_id(sr.SUM_CASES[i])} c {j}: sum {got:.9f} over {case['n_valid']} err {err:.3e} bound {case['bound']:.3e}")
    assert math.isfinite(got), "a read outside the valid interior"
    assert err <= case["bound"]
    assert second == 0.0


def test_ssim_sum_rejects_bad_sizes(device):
    m = torch.rand((2, 12, 12), device=device)
    buf, out = _dslice(device)
    ws = _nan_ws(device)
    for planes, h, w, border in [(2, 10, 12, 5), (2, 12, 10, 5), (0, 12, 12, 5), (2, 12, 12, 6), (2, 12, 12, -1)]:
        with pytest.raises(VfiLibraryError):
            _lib.call("vfi_ssim_sum", *([m.data_ptr()] * 5), planes, h, w, border, 1e-4, 9e-4, out.data_ptr(), ws.data_ptr(),
                      _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _dslice_intact(buf, written=False) and bool(torch.isnan(ws).all())


@pytest.mark.parametrize("i", range(len(sr.SSIM_CASES)), ids=[sr.case_id(c) for c in sr.SSIM_CASES])
def test_ssim_matches_float64(i, device):
    _, downsample, _ = sr.SSIM_CASES[i]
    case = sr.ssim_case(i)
    x, y = case["x"].to(device), case["y"].to(device)
    got = ei.ssim(x, y, downsample=downsample)
    err = abs(got - case["ref64"])
    print(f"ssim {sr.case_id(sr.SSIM_CASES[i])}: f {case['f']} got {got:.9f} ref64 {case['ref64']:.9f} err {err:.3e} bound {case['bound']:.3e}")
    assert math.isfinite(got) and err <= case["bound"]
    assert ei.ssim(x, y, downsample=downsample) == got
    assert torch.equal(x.cpu(), case["x"]) and torch.equal(y.cpu(), case["y"])


def test_psnr_cases(device):
    """piq.psnr's published formula: both images divided by data_range, then -10 log10(mse + 1e-8)"""
    x, y = sr.structured_pair((3, 37, 53), 21)
    assert ei.psnr(x.to(device), x.to(device)) == 10 * math.log10(1 / 1e-8)
    want = -10 * math.log10(float(((x.double() - y.double()) ** 2).mean()) + 1e-8)
    got = ei.psnr(x.to(device), y.to(device))
    assert abs(got - want) <= 1e-9 * want
    x8, y8 = (x * 255).round(), (y * 255).round()
    want = -10 * math.log10(float((((x8.double() - y8.double()) / 255) ** 2).mean()) + 1e-8)
    got = ei.psnr(x8.to(device), y8.to(device), data_range=255)
    print(f"psnr data_range 255: {got!r} vs {want!r}")
    assert abs(got - want) <= 1e-9 * want
    assert abs(ei.psnr(x8.to(device), x8.to(device), data_range=255) - 80.0) <= 1e-9 * 80.0


@pytest.mark.parametrize("shape,dim,crop", [((3, 100, 90), 128, (14, 19)), ((3, 70, 150), 64, (64, 64)), ((3, 45, 33), 33, (33, 33))])
def test_evaluate_image_crops(shape, dim, crop, device):
    pred, tgt = sr.structured_pair(shape, dim)
    got = ei.evaluate_image(types.SimpleNamespace(dim=dim), pred.to(device), tgt.to(device))
    sy, sx = shape[1] // 2 - dim // 2, shape[2] // 2 - dim // 2               # negative starts count from the end
    c = lambda t: t[:, sy:sy + dim, sx:sx + dim]
    assert tuple(c(pred).shape[1:]) == crop
    d = c(pred).double() - c(tgt).double()
    want = [sr.ssim_ref(c(pred), c(tgt), torch.float64)[0], float("nan"), 10 * math.log10(1.0 / (float((d * d).mean()) + 1e-8)),
            float(torch.sqrt((d * d).sum())), float(d.sum()), float(d.mean()), float(torch.var(d))]
    print(f"evaluate_image {shape} dim {dim}: " + " ".join(f"{g - w:.2e}" for g, w in zip(got, want)))
    assert math.isnan(got[1])
    for k, tol in ((0, 2e-5), (2, 1e-6), (3, 1e-6), (4, 1e-6), (5, 1e-9), (6, 1e-9)):
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])
