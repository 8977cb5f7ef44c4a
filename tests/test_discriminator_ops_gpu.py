"""The discriminator's entry points on the MI355X, through the C ABI: vfi_phase_split / vfi_phase_merge
bit for bit against indexing, the stride-2 convolution built on them against float64 `F.conv2d(stride=2, padding=1)`,
vfi_bn_leaky_* against the float64 closed forms, vfi_linear_* against float64 products.

Every output is a view into a buffer of NaN sentinels (glue_ref.canary_buffer) that must stay untouched around it; operands
start on a 16-byte boundary and one float past one, and their batch strides are padded.

Bounds.  Convolution, forward and data gradient: tests/test_conv_backward_gpu.py's DGRAD_BOUND for the kernel vfi_conv2d
selects, weights scaled by 1/sqrt(fan-in) of the convolution that runs; weight gradient: its dot-product bound, per element
(K+1) 2^-24 A with A the gradient of (|x|, |dy|) and K = N ceil(H/2) ceil(W/2) terms.  BatchNorm + LeakyReLU: the bounds of
tests/test_phasenet_bn_gpu.py (1e-5 max(1, max|expected|) elementwise, 1e-5 of the sum of the absolute terms for the two
reduced gradients).  Linear: forward and dx 1e-5 of the sum of the absolute terms per element (an fp32 tree loses at most
log2(n) 2^-24 of it); dw and dbias 4 ulp of the sum of their B absolute terms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adversarial_ref as AR
import phasenet_bn_ref as B
from glue_ref import assert_untouched, canary_buffer, fview
from test_conv_backward_gpu import DGRAD_BOUND
from vfi_amd import _lib, ops

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
GUARD = 8                       # sentinel floats before a view (a multiple of 4: the view's alignment is `off` alone)
SIZES = [(1, 1), (1, 6), (2, 2), (3, 5), (7, 8), (16, 9), (32, 32)]
LAYOUTS = [("aligned", 0, 4), ("one float in", 1, 4), ("odd stride", 0, 3)]     # (name, base offset, batch stride padding)


def _call(name, *args):
    h = _lib.lib()
    status = getattr(h, name)(*args)
    assert status == 0, (name, status, h.vfi_last_error())


def _held(shape, device, off=0, pad=4, values=None):
    """(flat, view): a view of `shape` into a sentinel buffer, `off` floats past a 16-byte boundary, batch stride padded by
    `pad` floats; filled with `values` when given."""
    shape = tuple(shape)
    per = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    bs = per + (pad if len(shape) > 1 else 0)
    flat = canary_buffer(GUARD + off + shape[0] * bs + GUARD, device)
    strides, s = [], 1
    for d in reversed(shape[1:]):
        strides.insert(0, s)
        s *= d
    view = fview(flat, shape, GUARD + off, [bs] + strides)
    if values is not None:
        view.copy_(values)
    assert view.data_ptr() % 16 == 4 * off
    return flat, view


def _d(t):
    return t.detach().double().cpu()


# ---- phase split / merge -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_phase_split_and_merge_are_indexing(h, w, device):
    for c in (1, 3, 64):
        g = torch.Generator().manual_seed(c * 1000 + h * 40 + w)
        x = torch.randn((2, c, h, w), generator=g)
        gs = torch.randn((2, 4 * c, (h + 1) // 2, (w + 1) // 2), generator=g)       # non-zero where the split's fill sits
        for name, off, pad in LAYOUTS:
            _, xd = _held(x.shape, device, off, pad, x)
            flat, out = _held(gs.shape, device, off, pad)
            _call("vfi_phase_split", xd.data_ptr(), xd.stride(0), out.data_ptr(), out.stride(0), 2, c, h, w, _lib.stream_ptr())
            assert_untouched(flat, out, what="vfi_phase_split")
            assert torch.equal(out.cpu(), AR.phase_split(x)), (c, name)
            _, gd = _held(gs.shape, device, off, pad, gs)
            flat2, back = _held(x.shape, device, off, pad)
            _call("vfi_phase_merge", gd.data_ptr(), gd.stride(0), back.data_ptr(), back.stride(0), 2, c, h, w, _lib.stream_ptr())
            assert_untouched(flat2, back, what="vfi_phase_merge")
            assert torch.equal(back.cpu(), AR.phase_merge(gs, (h, w))), (c, name)
            flat3, again = _held(x.shape, device, off, pad)
            _call("vfi_phase_merge", out.data_ptr(), out.stride(0), again.data_ptr(), again.stride(0), 2, c, h, w, _lib.stream_ptr())
            assert_untouched(flat3, again, what="vfi_phase_merge")
            assert torch.equal(again.cpu(), x), (c, name, "merge(split(x)) != x")
        assert torch.equal(ops.phase_merge(ops.phase_split(x.to(device)), (h, w)).cpu(), x)


# ---- the stride-2 convolution -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(3, 64), (6, 64), (64, 64), (128, 128)])
@pytest.mark.parametrize("h,w", SIZES)
def test_conv2d_stride2_against_float64(h, w, cin, cout, device):
    n = 2
    g = torch.Generator().manual_seed(cin * 7 + cout + h * 100 + w)
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    wt_d = torch.randn((cout, cin, 3, 3), generator=g) / (cout * 9) ** 0.5          # the data gradient's own filter
    bias = torch.randn((cout,), generator=g)
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    dy = torch.randn((n, cout, h2, w2), generator=g)
    algo_f = _lib.lib().vfi_conv2d_algo(n, 4 * cin, h2, w2, cout, 3, 0, 0, 0)
    algo_d = _lib.lib().vfi_conv2d_algo(n, cout, h2, w2, 4 * cin, 3, 0, 0, 0)
    assert algo_f in DGRAD_BOUND and algo_d in DGRAD_BOUND

    x64 = x.double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    want = F.conv2d(x64, w64, bias.double(), stride=2, padding=1)
    _, want_dw = torch.autograd.grad((want * dy.double()).sum(), [x64, w64])
    xd64 = x.double().requires_grad_(True)
    want_dx, = torch.autograd.grad((F.conv2d(xd64, wt_d.double(), stride=2, padding=1) * dy.double()).sum(), [xd64])
    wa = torch.zeros_like(w64, requires_grad=True)
    a_bound, = torch.autograd.grad((F.conv2d(x.double().abs(), wa, stride=2, padding=1) * dy.double().abs()).sum(), [wa])

    _, xd = _held(x.shape, device, 0, 4, x)
    flat, out = _held(want.shape, device, 0, 4)
    pc = ops.PackedConv(ops.stride2_weight(wt.to(device)), bias.to(device))
    assert ops.conv2d_stride2(xd, pc, out=out) is out
    assert_untouched(flat, out, what="conv2d_stride2")
    err = float((_d(out) - want.detach()).abs().max())
    assert bool(torch.isfinite(out).all()) and err <= DGRAD_BOUND[algo_f], (err, algo_f)

    _, dyd = _held(dy.shape, device, 0, 4, dy)
    flat, dx = _held(x.shape, device, 0, 4)
    pct = ops.packed_transposed(ops.stride2_weight(wt_d.to(device)))
    assert ops.conv2d_stride2_backward_data(dyd, pct, (h, w), out=dx) is dx
    assert_untouched(flat, dx, what="conv2d_stride2_backward_data")
    err_d = float((_d(dx) - want_dx).abs().max())
    assert bool(torch.isfinite(dx).all()) and err_d <= DGRAD_BOUND[algo_d], (err_d, algo_d)

    dw, db = ops.conv2d_stride2_backward_weight(xd, dyd)
    k = n * h2 * w2
    err_w = (_d(dw) - want_dw).abs()
    ratio = float((err_w / (EPS24 * a_bound).clamp_min(1e-300)).max())
    print(f"conv2d_stride2 {cin}->{cout} {h}x{w}: algo {algo_f}/{algo_d}, forward {err:.2e}, dX {err_d:.2e}, dW err/(2^-24 A) {ratio:.2f} (K+1 = {k + 1})")
    assert dw.shape == wt.shape and bool((err_w <= (k + 1) * EPS24 * a_bound).all()), ratio
    sum_abs = dy.double().abs().sum((0, 2, 3))
    assert bool(((_d(db) - dy.double().sum((0, 2, 3))).abs() <= (k + 1) * EPS24 * sum_abs).all())
    dw2, db2 = ops.conv2d_stride2_backward_weight(xd, dyd)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs differ"


# ---- BatchNorm + LeakyReLU ----------------------------------------------------------------------------------------------
HW_SHAPES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 1023: (31, 33), 4100: (41, 100)}
ENTRY_SHAPES = [(3, 1, 1), (1, 8, 3), (3, 64, 4), (2, 5, 1023), (3, 64, 4100)]      # tests/test_phasenet_bn_gpu.py's
BN_EPS = 1e-5


def _place(t, layout, device):
    """tests/test_phasenet_bn_gpu.py's three layouts: dense, a channel slice of a wider buffer, such a slice one float off
    16-byte alignment."""
    n, c, h, w = t.shape
    if layout == "dense":
        return t.to(device)
    wide = c + 7
    if layout == "misaligned":
        pad = (1 - 3 * h * w) % 4 or 4
        buf = torch.zeros(n * wide * h * w + pad, device=device)[pad:].view(n, wide, h, w)
    else:
        buf = torch.zeros((n, wide, h, w), device=device)
    v = buf[:, 3:3 + c]
    v.copy_(t)
    if layout == "misaligned":
        assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("slope", [0.2, 1.0])
@pytest.mark.parametrize("n,c,hw", ENTRY_SHAPES)
def test_bn_leaky_against_float64(n, c, hw, slope, device):
    g = torch.Generator().manual_seed(n * 100000 + c * 10 + hw)
    r = lambda *s: torch.randn(s, generator=g)
    h, w = HW_SHAPES[hw]
    y0, g0, gamma, beta = r(n, c, h, w) * 1.5 - 0.5, r(n, c, h, w), (r(c) * 0.3 + 1.0).to(device), (r(c) * 0.5).to(device)
    for layout in ("dense", "slices", "misaligned"):
        y, g_t = _place(y0, layout, device), _place(g0, layout, device)
        mean, var = ops.bn_stats(y)
        y64, g64, mu64, v64, ga64, be64 = _d(y), _d(g_t), _d(mean), _d(var), _d(gamma), _d(beta)
        z = B.bn_act_forward(y64, mu64, v64, ga64, be64, BN_EPS, None)
        want_t = torch.where(z > 0, z, z * slope)
        t = ops.bn_leaky_forward(y, mean, var, gamma, beta, BN_EPS, slope)
        err = float((_d(t) - want_t).abs().max())
        assert bool(torch.isfinite(t).all()) and err <= 1e-5 * max(1.0, float(want_t.abs().max())), (layout, err)
        assert torch.equal(t, ops.bn_leaky_forward(y, mean, var, gamma, beta, BN_EPS, slope)), "two runs differ"
        into = _place(torch.zeros(n, c, h, w), layout, device)
        assert ops.bn_leaky_forward(y, mean, var, gamma, beta, BN_EPS, slope, out=into) is into and torch.equal(into, t)
        if slope == 1.0:        # no activation: the bits of the existing entry
            assert torch.equal(t, ops.bn_act_forward(y, mean, var, gamma, beta, BN_EPS, None))
        # the adjoint, the derivative from the sign of the library's own output
        t64 = _d(t)
        g_z = torch.where(t64 > 0, g64, g64 * slope)
        want_gy, want_gg, want_gb = B.bn_act_backward(g_z, t64, y64, mu64, v64, ga64, BN_EPS, None)
        xh = (y64 - mu64.view(1, -1, 1, 1)) / torch.sqrt(v64 + BN_EPS).view(1, -1, 1, 1)
        g_y, g_gamma, g_beta = ops.bn_leaky_backward(g_t, t, y, mean, var, gamma, BN_EPS, slope)
        assert float(((_d(g_beta) - want_gb).abs() - 1e-5 * g_z.abs().sum((0, 2, 3))).max()) <= 0, layout
        assert float(((_d(g_gamma) - want_gg).abs() - 1e-5 * (g_z * xh).abs().sum((0, 2, 3))).max()) <= 0, layout
        err = float((_d(g_y) - want_gy).abs().max())
        assert bool(torch.isfinite(g_y).all()) and err <= 1e-5 * max(1.0, float(want_gy.abs().max())), (layout, err)
        again = ops.bn_leaky_backward(g_t, t, y, mean, var, gamma, BN_EPS, slope)
        assert all(torch.equal(a, b) for a, b in zip((g_y, g_gamma, g_beta), again)), "two runs differ"
        none, gg, gb = ops.bn_leaky_backward(g_t, t, y, mean, var, gamma, BN_EPS, slope, need_data=False)
        assert none is None and torch.equal(gg, g_gamma) and torch.equal(gb, g_beta)
        alias = _place(g0, layout, device)
        got, gg, gb = ops.bn_leaky_backward(alias, t, y, mean, var, gamma, BN_EPS, slope, out=alias)
        assert got is alias and torch.equal(alias, g_y) and torch.equal(gg, g_gamma) and torch.equal(gb, g_beta)
        if slope == 1.0:
            same = ops.bn_act_backward(g_t, None, y, mean, var, gamma, BN_EPS, None)
            assert all(torch.equal(a, b) for a, b in zip((g_y, g_gamma, g_beta), same))


# ---- linear layers ------------------------------------------------------------------------------------------------------
def _ulp32(s):
    return torch.from_numpy(np.spacing(s.numpy().astype(np.float32)).astype(np.float64))


def _linear_backward(x, w, y, slope, g, device, off, want):
    """vfi_linear_backward with the outputs named in `want` (the others NULL) -> {name: cpu tensor}; checks the canaries."""
    b, k = x.shape
    j = w.shape[0]
    held = {"dx": _held((b, k), device, off, 0) if "dx" in want else None,
            "dw": _held((j, k), device, off, 0) if "dw" in want else None,
            "dbias": _held((j,), device, off, 0) if "dbias" in want else None}
    ptr = lambda name: held[name][1].data_ptr() if held[name] is not None else None
    _call("vfi_linear_backward", x.data_ptr(), w.data_ptr(), y.data_ptr(), slope, g.data_ptr(), ptr("dx"), ptr("dw"), ptr("dbias"),
          b, k, j, _lib.stream_ptr())
    out = {}
    for name, hv in held.items():
        if hv is not None:
            assert_untouched(hv[0], hv[1], what="vfi_linear_backward " + name)
            out[name] = hv[1].cpu()
    return out


@pytest.mark.parametrize("k,j", [(1, 1), (3, 2), (255, 63), (256, 64), (257, 65), (4099, 3), (512, 1024), (131072, 8)])
def test_linear_against_float64(k, j, device):
    worst = dict(y=0.0, dx=0.0, dw=0.0)
    for b in (1, 2, 3, 4, 9):
        g_ = torch.Generator().manual_seed(k * 31 + j * 7 + b)
        x0, w0 = torch.randn((b, k), generator=g_), torch.randn((j, k), generator=g_) / k ** 0.5
        bias0, g0 = torch.randn((j,), generator=g_), torch.randn((b, j), generator=g_)
        x64, w64, b64, g64 = x0.double(), w0.double(), bias0.double(), g0.double()
        z64 = x64 @ w64.t() + b64
        z_abs = x64.abs() @ w64.abs().t() + b64.abs()
        for slope in (0.2, 1.0):
            for off in (0, 1):
                x, w, bias, g = (_held(t.shape, device, off, 0, t)[1] for t in (x0, w0, bias0, g0))
                flat, y = _held((b, j), device, off, 0)
                _call("vfi_linear_forward", x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), b, k, j, slope, _lib.stream_ptr())
                assert_untouched(flat, y, what="vfi_linear_forward")
                pos = _d(y) > 0                                 # the mask: the product's own output
                want = torch.where(pos, z64, z64 * slope)
                ratio = float(((_d(y) - want).abs() / z_abs).max())
                worst["y"] = max(worst["y"], ratio)
                assert bool(torch.isfinite(y).all()) and ratio <= 1e-5, (b, slope, off, ratio)
                flat2, y2 = _held((b, j), device, off, 0)
                _call("vfi_linear_forward", x.data_ptr(), w.data_ptr(), bias.data_ptr(), y2.data_ptr(), b, k, j, slope, _lib.stream_ptr())
                assert torch.equal(y, y2), "two runs differ"

                gm = torch.where(pos, g64, g64 * slope)
                full = _linear_backward(x, w, y, slope, g, device, off, ("dx", "dw", "dbias"))
                r_dx = float(((full["dx"].double() - gm @ w64).abs() / (gm.abs() @ w64.abs()).clamp_min(1e-300)).max())
                s_dw = gm.abs().t() @ x64.abs()
                r_dw = float(((full["dw"].double() - gm.t() @ x64).abs() / _ulp32(s_dw)).max())
                r_db = float(((full["dbias"].double() - gm.sum(0)).abs() / _ulp32(gm.abs().sum(0))).max())
                worst["dx"], worst["dw"] = max(worst["dx"], r_dx), max(worst["dw"], r_dw, r_db)
                assert r_dx <= 1e-5 and r_dw <= 4.0 and r_db <= 4.0, (b, slope, off, r_dx, r_dw, r_db)
                assert all(bool(torch.isfinite(v).all()) for v in full.values())
                again = _linear_backward(x, w, y, slope, g, device, off, ("dx", "dw", "dbias"))
                assert all(torch.equal(full[n_], again[n_]) for n_ in full), "two runs differ"
                for missing in ("dx", "dw", "dbias"):           # each output NULL in turn: the others keep their bits
                    some = _linear_backward(x, w, y, slope, g, device, off, tuple(n_ for n_ in full if n_ != missing))
                    assert missing not in some and all(torch.equal(full[n_], some[n_]) for n_ in some), missing
    print(f"linear K={k} J={j}: worst forward err / sum|terms| {worst['y']:.2e}, dx {worst['dx']:.2e}, dw, dbias {worst['dw']:.2f} ulp")


def test_linear_through_ops(device):
    g_ = torch.Generator().manual_seed(3)
    x, w, bias, g = (t.to(device) for t in (torch.randn((3, 70), generator=g_), torch.randn((5, 70), generator=g_),
                                            torch.randn((5,), generator=g_), torch.randn((3, 5), generator=g_)))
    y = ops.linear_forward(x, w, bias, 0.2)
    assert AR.rel(y, F.leaky_relu(F.linear(x.double(), w.double(), bias.double()), 0.2)) <= 1e-6
    dx, dw, db = ops.linear_backward(x, w, y, 0.2, g)
    gm = torch.where(y > 0, g, g * 0.2).double()
    assert AR.rel(dx, gm @ w.double()) <= 1e-6 and AR.rel(dw, gm.t() @ x.double()) <= 1e-6 and AR.rel(db, gm.sum(0)) <= 1e-6
    only = ops.linear_backward(x, w, y, 0.2, g, need_w=False, need_bias=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], dx)
    with pytest.raises(_lib.VfiLibraryError):
        ops.linear_forward(x, w[:, :60], bias, 0.2)
