"""vfi_conv2d_backward_weight and vfi_conv2d_backward_data in isolation (csrc/vfi_conv_grad.hip).

Weight gradient: every case of conv_wgrad_ref.CASES under every `max_splits` cap of its row, so that a workgroup of
conv_wgrad_kernel walks runs of several tiles (across tile-row ends, across the image boundary, with a ragged last run)
and slab_reduce_kernel sums 1 .. 18 slabs.  The split-K workspace is filled with NaN before every call: a reduce that
reads a slab this call did not write gives NaN.  Integer data must be bit-exact against float64 (fp32 MFMA and fp32 adds
are exact while every partial sum stays below 2**24, whatever the order); Gaussian data is held per element to the bound
of a K-term fp32 dot product summed in any order, |dW - dW64| <= (K+1) 2**-24 A with A = dW(|x|, |dy|), K = n*h*w.

Input gradient: reflect padding at minimal and lopsided sizes, zero padding on one-row / one-column images, dy and dx as
channel slices, against float64 autograd; dy is always read from a NaN-surrounded slice and dx written into a canary
buffer.  Bounds: those tests/test_conv_gpu.py holds for the kernel vfi_conv2d selects (see DGRAD_BOUND).

Argument errors raise VfiLibraryError before any kernel runs and leave the outputs' canaries alone."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_wgrad_ref as R
from glue_ref import assert_untouched, canary_buffer, fview
from vfi_amd import _lib, ops
from vfi_amd._lib import VfiLibraryError

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 2.0 ** -24
CASE_IDS = [c.id for c in R.CASES]


# ---- weight gradient -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_inputs(key, kind, device):
    """x, dy of a case on the device; a sliced case gets channel slices of wider tensors with NaN around them."""
    d = R.data(key, kind)
    if not key[-1]:
        return d.x.to(device), d.dy.to(device)
    cin, cout = key[1], key[2]
    xw = R.embed_in_nan(d.x, *R.X_SLICE)[0].to(device)
    dyw = R.embed_in_nan(d.dy, *R.DY_SLICE)[0].to(device)
    x, dy = xw[:, R.X_SLICE[0]:R.X_SLICE[0] + cin], dyw[:, R.DY_SLICE[0]:R.DY_SLICE[0] + cout]
    assert x.stride(0) != cin * x.shape[2] * x.shape[3] and dy.stride(0) != cout * x.shape[2] * x.shape[3]
    return x, dy


def _wgrad(case, cap, kind, bias, device):
    x, dy = _device_inputs(case.key, kind, device)
    ops._workspace(device).fill_(NAN)
    dw, db = ops.conv2d_backward_weight(x, dy, case.ks, case.pad, bias=bias, max_splits=cap)
    return dw.cpu(), None if db is None else db.cpu()


@pytest.mark.parametrize("case,cap", R.CASE_CAPS, ids=R.CASE_CAP_IDS)
def test_library_split_count_equals_plan(case, cap):
    assert ops.WORKSPACE_FLOATS == R.WORKSPACE_FLOATS
    p = R.case_plan(case, cap)
    got = _lib.lib().vfi_conv2d_backward_weight_splits(case.n, case.cin, case.h, case.w, case.cout, case.ks,
                                                       R.workspace_for(case, cap))
    assert got == p.splits == case.caps[cap][1], (got, p)


@pytest.mark.parametrize("case,cap", R.CASE_CAPS, ids=R.CASE_CAP_IDS)
def test_weight_gradient_is_exact_on_integer_data(case, cap, device):
    """x integers in [-3, 3], dy in [-2, 2]: any dropped, doubled or misplaced pixel or tap changes an integer."""
    d = R.data(case.key, "int")
    for bias in (True, False):
        dw, db = _wgrad(case, cap, "int", bias, device)
        assert dw.shape == d.dw.shape
        assert torch.equal(dw.double(), d.dw), (bias, int((dw.double() != d.dw).sum()), "elements differ")
        if bias:
            assert torch.equal(db.double(), d.db), (db, d.db)
        else:
            assert db is None


_worst_ratio = {}


@pytest.mark.parametrize("case,cap", R.CASE_CAPS, ids=R.CASE_CAP_IDS)
def test_weight_gradient_gaussian_within_dot_product_bound(case, cap, device):
    """Each element of dW within (K+1) 2**-24 A, each of db within (K+1) 2**-24 sum|dy| (derived, not measured; where A is
    0 -- a tap that only ever sees zero padding -- the element must be exactly 0)."""
    d = R.data(case.key, "randn")
    dw, db = _wgrad(case, cap, "randn", True, device)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    err_w, err_b = (dw.double() - d.dw).abs(), (db.double() - d.db).abs()
    ratio_w = (err_w / (EPS * d.a).clamp_min(1e-300)).max().item()
    ratio_b = (err_b / (EPS * d.sum_abs_dy).clamp_min(1e-300)).max().item()
    _worst_ratio[(case.id, cap)] = max(ratio_w, ratio_b)
    print("%s cap %s: K+1 = %d, worst err/(2^-24 A): dW %.3f, db %.3f; worst so far %.3f"
          % (case.id, cap, d.k + 1, ratio_w, ratio_b, max(_worst_ratio.values())))
    assert (err_w <= (d.k + 1) * EPS * d.a).all(), ratio_w
    assert (err_b <= (d.k + 1) * EPS * d.sum_abs_dy).all(), ratio_b


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_weight_gradient_bits_repeat(case, device):
    """Two calls give the same bits (Gaussian data, every cap); with integer data every cap gives the same bits."""
    ints = []
    for cap in case.caps:
        a = _wgrad(case, cap, "randn", True, device)
        b = _wgrad(case, cap, "randn", True, device)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), cap
        ints.append(_wgrad(case, cap, "int", True, device))
    for dw, db in ints[1:]:
        assert torch.equal(dw, ints[0][0]) and torch.equal(db, ints[0][1])


# ---- input gradient --------------------------------------------------------------------------------------------------
# max |dX - dX64| per selected kernel (vfi_conv2d_algo), as tests/test_conv_gpu.py holds them for O(1) outputs with
# weights scaled by 1/sqrt(fan-in): direct MFMA and streaming 1x1 kernels 2e-5 (test_conv_matches_torch_cpu), Winograd
# F(2x2) 3e-5 (test_winograd_conv_matches_torch_cpu), Winograd F(4x4) 1e-4 (test_large_plain_conv_matches_torch_cpu)
DGRAD_BOUND = {0: 2e-5, 3: 2e-5, 1: 3e-5, 2: 1e-4}

DGRAD_CASES = [  # (group, n, cin, cout, h, w, ks, pad, sliced out)
    # (a) reflect at minimal and lopsided sizes: H or W = pad + 1 (every index a mirror source) beside a long other axis
    ("a", 2, 5, 7, 3, 37, 5, "reflect", False), ("a", 2, 5, 7, 40, 3, 5, "reflect", False),
    ("a", 2, 5, 7, 4, 33, 5, "reflect", False), ("a", 2, 5, 7, 2, 33, 3, "reflect", False),
    ("a", 2, 5, 7, 33, 2, 3, "reflect", False),
    # (b) zero padding on one row / one column
    ("b", 2, 5, 7, 1, 35, 5, "zeros", False), ("b", 2, 5, 7, 35, 1, 5, "zeros", False),
    ("b", 2, 5, 7, 1, 35, 3, "zeros", False), ("b", 2, 5, 7, 35, 1, 3, "zeros", False),
] + [  # (c) dx a channel slice of a wider tensor (dy is a slice in every case)
    ("c", 2, 5, 7, 7, 37, ks, pad, True) for ks in (1, 3, 5) for pad in ("zeros", "reflect")
]
DGRAD_IDS = ["%s-%dx%d-%d_%dx%d_k%d_%s" % c[:8] for c in DGRAD_CASES]
DX_SLICE = (2, 3)       # channels of canary before / after dx in its wide tensor
GUARD = 37              # canary floats before and after a dense dx (odd: dx is only 4-byte aligned)


def _conv64(x, w, pad):
    k = w.shape[-1]
    p = (k - 1) // 2
    if p and pad == "reflect":
        return F.conv2d(F.pad(x, (p,) * 4, mode="reflect"), w)
    return F.conv2d(x, w, padding=p)


@functools.lru_cache(maxsize=None)
def _dgrad_data(n, cin, cout, h, w, ks, pad, kind):
    """fp32 dy, weight and the float64 dX by autograd.  Weights scaled by 1/sqrt(fan-in) of the convolution that runs
    (dY's cout channels in, KS*KS taps) unless the case asks for exact integers."""
    g = torch.Generator().manual_seed(97 * h + 13 * w + 1009 * ks + (pad == "reflect") + 2 * (kind != "randn"))
    if kind == "randn":
        dy = torch.randn((n, cout, h, w), generator=g)
        wt = torch.randn((cout, cin, ks, ks), generator=g) / (cout * ks * ks) ** 0.5
    else:
        dy = torch.randint(-3, 4, (n, cout, h, w), generator=g).float()
        wt = torch.randint(-2, 3, (cout, cin, ks, ks), generator=g).float()
        if kind == "int_scaled":
            wt = wt / (cout * ks * ks) ** 0.5
    xd = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    (_conv64(xd, wt.double(), pad) * dy.double()).sum().backward()
    return dy, wt, xd.grad.detach()


def _run_dgrad(n, cin, cout, h, w, ks, pad, sliced, kind, device):
    """-> (dX on the CPU, float64 reference, algo of the convolution that ran); asserts the canaries."""
    dy, wt, ref = _dgrad_data(n, cin, cout, h, w, ks, pad, kind)
    dyw = R.embed_in_nan(dy, *R.DY_SLICE)[0].to(device)
    dy_d = dyw[:, R.DY_SLICE[0]:R.DY_SLICE[0] + cout]
    hw = h * w
    if sliced:
        cw = DX_SLICE[0] + cin + DX_SLICE[1]
        flat = canary_buffer(n * cw * hw + 2 * GUARD, device)
        out = fview(flat, (n, cin, h, w), GUARD + DX_SLICE[0] * hw, (cw * hw, hw, w, 1))
    else:
        flat = canary_buffer(n * cin * hw + 2 * GUARD, device)
        out = fview(flat, (n, cin, h, w), GUARD)
    got = ops.conv2d_backward_data(dy_d, ops.packed_transposed(wt.to(device)), pad, out=out)
    torch.cuda.synchronize()
    assert got is out
    assert_untouched(flat, out, what="conv2d_backward_data")
    p = (ks - 1) // 2 if pad == "reflect" else 0
    algo = _lib.lib().vfi_conv2d_algo(n, cout, h + 2 * p, w + 2 * p, cin, ks, 0, 0, 0)
    assert algo in DGRAD_BOUND, algo
    return out.cpu(), ref, algo


_worst_dgrad = {}


def _note_dgrad(ks, err):
    _worst_dgrad[ks] = max(_worst_dgrad.get(ks, 0.0), err)
    return "worst so far for KS %d: %.3e" % (ks, _worst_dgrad[ks])


@pytest.mark.parametrize("group,n,cin,cout,h,w,ks,pad,sliced", DGRAD_CASES, ids=DGRAD_IDS)
def test_input_gradient_matches_float64(group, n, cin, cout, h, w, ks, pad, sliced, device):
    got, ref, algo = _run_dgrad(n, cin, cout, h, w, ks, pad, sliced, "randn", device)
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs().max().item()
    print("dgrad (%s) KS %d %s %dx%d: algo %d, max err %.3e, bound %.0e; %s"
          % (group, ks, pad, h, w, algo, err, DGRAD_BOUND[algo], _note_dgrad(ks, err)))
    assert err <= DGRAD_BOUND[algo], (err, algo)


@pytest.mark.parametrize("group,n,cin,cout,h,w,ks,pad,sliced", DGRAD_CASES, ids=DGRAD_IDS)
def test_input_gradient_on_integer_data(group, n, cin, cout, h, w, ks, pad, sliced, device):
    """dy integers in [-3, 3], weights in [-2, 2].  KS 1 and KS 5 run a direct kernel (embed, fp32 MFMA and the reflect fold
    are exact on such data): torch.equal.  KS 3 runs a Winograd kernel whose transform constants are not dyadic: there the
    integer weights are scaled by 1/sqrt(fan-in) and the selected kernel's bound of DGRAD_BOUND holds."""
    if ks != 3:
        got, ref, algo = _run_dgrad(n, cin, cout, h, w, ks, pad, sliced, "int", device)
        assert algo in (0, 3), "KS 1 and KS 5 have only direct kernels"
        print("dgrad (%s) KS %d %s %dx%d integers: algo %d, exact" % (group, ks, pad, h, w, algo))
        assert torch.equal(got.double(), ref), int((got.double() != ref).sum())
        return
    got, ref, algo = _run_dgrad(n, cin, cout, h, w, ks, pad, sliced, "int_scaled", device)
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs().max().item()
    print("dgrad (%s) KS 3 %s %dx%d integers / sqrt(fan-in): algo %d, max err %.3e, bound %.0e; %s"
          % (group, pad, h, w, algo, err, DGRAD_BOUND[algo], _note_dgrad(ks, err)))
    assert err <= DGRAD_BOUND[algo], (err, algo)


# ---- argument errors: VfiLibraryError, no kernel runs, outputs keep their canary ------------------------------------------
def _raises_and_keeps(flats, fn):
    with pytest.raises(VfiLibraryError):
        fn()
    torch.cuda.synchronize()
    for f in flats:
        assert_untouched(f, what="after a rejected call")


def test_backward_weight_argument_errors(device):
    n, cin, cout, h, w = 1, 3, 4, 6, 8
    x = torch.zeros((n, cin, h, w), device=device)
    dy = torch.zeros((n, cout, h, w), device=device)
    ws = ops._workspace(device)
    dwf, dbf = canary_buffer(cout * cin * 49, device), canary_buffer(cout, device)
    s = _lib.stream_ptr()

    def direct(ks=3, pad="zeros", hh=h, ww=w, ws_floats=ws.numel()):
        return lambda: _lib.call("vfi_conv2d_backward_weight", x.data_ptr(), cin * hh * ww, dy.data_ptr(), cout * hh * ww,
                                 dwf.data_ptr(), dbf.data_ptr(), n, cin, hh, ww, cout, ks, ops.PAD[pad], ws.data_ptr(),
                                 ws_floats, s)
    for ks in (7, 2):
        _raises_and_keeps((dwf, dbf), direct(ks=ks))
        with pytest.raises(VfiLibraryError):
            ops.conv2d_backward_weight(x, dy, ks)
        assert _lib.lib().vfi_conv2d_backward_weight_splits(n, cin, h, w, cout, ks, ws.numel()) == -1
        assert _lib.lib().vfi_conv2d_backward_weight_workspace_floats(cout, cin, ks) == -1
    # reflect with pad >= H, pad >= W (5x5: pad 2; 3x3: pad 1)
    for ks, hh, ww in ((5, 2, 8), (5, 6, 2), (3, 1, 8), (3, 6, 1)):
        _raises_and_keeps((dwf, dbf), direct(ks=ks, pad="reflect", hh=hh, ww=ww))
        with pytest.raises(VfiLibraryError):
            ops.conv2d_backward_weight(x[:, :, :hh, :ww].contiguous(), dy[:, :, :hh, :ww].contiguous(), ks, "reflect")
    # a workspace one float short of one slab
    per = _lib.lib().vfi_conv2d_backward_weight_workspace_floats(cout, cin, 3)
    assert per == cout * (cin * 9 + 1)
    _raises_and_keeps((dwf, dbf), direct(ws_floats=per - 1))
    # dy that does not match x; CPU tensors
    for bad in (torch.zeros((n, cout, h, w + 1), device=device), torch.zeros((n + 1, cout, h, w), device=device),
                torch.zeros((n, cout, h + 1, w), device=device)):
        with pytest.raises(VfiLibraryError):
            ops.conv2d_backward_weight(x, bad, 3)
    for a, b in ((x.cpu(), dy.cpu()), (x, dy.cpu()), (x.cpu(), dy)):
        with pytest.raises(VfiLibraryError):
            ops.conv2d_backward_weight(a, b, 3)
    # the accepted call next to the rejected ones does write
    direct(ws_floats=per)()
    torch.cuda.synchronize()
    assert (dwf[:cout * cin * 9].view(torch.float32) == 0).all() and (dbf.view(torch.float32) == 0).all()


def test_backward_data_argument_errors(device):
    n, cin, cout, h, w = 1, 3, 4, 6, 8
    dy = torch.zeros((n, cout, h, w), device=device)
    pct = {ks: ops.packed_transposed(torch.zeros((cout, cin, ks, ks), device=device)) for ks in (3, 5)}
    dxf = canary_buffer(n * cin * h * w, device)
    dx = fview(dxf, (n, cin, h, w))
    ws = torch.empty(1 << 20, dtype=torch.float32, device=device)
    s = _lib.stream_ptr()

    def direct(ks=3, pad="reflect", hh=h, ww=w, ws_floats=ws.numel()):
        return lambda: _lib.call("vfi_conv2d_backward_data", dy.data_ptr(), cout * hh * ww, pct[3 if ks != 5 else 5].packed.data_ptr(),
                                 dxf.data_ptr(), cin * hh * ww, n, cin, hh, ww, cout, ks, ops.PAD[pad], ws.data_ptr(),
                                 ws_floats, s)
    for ks in (7, 2):
        _raises_and_keeps((dxf,), direct(ks=ks))
        _raises_and_keeps((dxf,), direct(ks=ks, pad="zeros"))
        assert _lib.lib().vfi_conv2d_backward_data_workspace_floats(n, cin, h, w, cout, ks, 1) == -1
    for ks, hh, ww in ((5, 2, 8), (5, 6, 2), (3, 1, 8), (3, 6, 1)):
        _raises_and_keeps((dxf,), direct(ks=ks, hh=hh, ww=ww))
        small = fview(dxf, (n, cin, hh, ww))
        _raises_and_keeps((dxf,), lambda: ops.conv2d_backward_data(dy[:, :, :hh, :ww].contiguous(), pct[ks], "reflect", out=small))
    # a reflect workspace one float short
    need = _lib.lib().vfi_conv2d_backward_data_workspace_floats(n, cin, h, w, cout, 3, 1)
    assert need == n * (cin + cout) * (h + 2) * (w + 2) and need <= ws.numel()
    _raises_and_keeps((dxf,), direct(ws_floats=need - 1))
    _raises_and_keeps((dxf,), direct(ws_floats=0))
    # dy that does not match the weights or the output; CPU tensors
    for pad in ("zeros", "reflect"):
        _raises_and_keeps((dxf,), lambda: ops.conv2d_backward_data(torch.zeros((n, cout + 1, h, w), device=device), pct[3], pad, out=dx))
        _raises_and_keeps((dxf,), lambda: ops.conv2d_backward_data(torch.zeros((n, cout, h, w + 1), device=device), pct[3], pad, out=dx))
        _raises_and_keeps((dxf,), lambda: ops.conv2d_backward_data(dy.cpu(), pct[3], pad, out=dx))
        with pytest.raises(VfiLibraryError):
            ops.conv2d_backward_data(dy.cpu(), pct[3], pad)
        with pytest.raises(VfiLibraryError):
            ops.conv2d_backward_data(dy, pct[3], pad, out=torch.zeros((n, cin, h, w)))
    # the accepted call next to the rejected ones does write
    direct(ws_floats=need)()
    torch.cuda.synchronize()
    assert (dx == 0).all()
