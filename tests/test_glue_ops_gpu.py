"""The forward glue kernels of csrc/vfi_aux.hip, each against an independent CPU reference (torch float64 / float32) at the
smallest shapes at which every branch of the kernel and of its host dispatch exists.

Exact operations (pad, copy, one multiply, max, max + eps) are compared bit for bit with float32 torch; rounded ones within
glue_ref.tol_of (computed from the reference alone, printed by every assertion).  Slices an op writes sit in canary buffers,
slices an op reads are surrounded by NaN (glue_ref).

Which case reaches which kernel (the host conditions of vfi_pool2 / vfi_resize_bilinear decide):
  pool2_kernel (float2 loads)      test_pool2 (1,1,2,2), (2,5,6,10) dense / out_slice, (1,4,8,34)
  pool2_kernel_unaligned           test_pool2 (2,3,7,9) (odd W), (2,5,6,10) ptr_offset (pointer % 8 == 4) and odd_bstride
  resize_bilinear_kernel           test_resize_bilinear_slices (5,16)->(10,32) with the misaligned residual or output
  resize_bilinear_vec4_kernel      test_resize_bilinear_slices (5,16)->(10,32), no residual, aligned output
  resize_bilinear_tile_kernel<1>   test_resize_bilinear_slices (10,32)->(20,64), no residual, aligned output
  resize_bilinear_tile_kernel<0>   test_resize_bilinear_slices (10,33)->(20,66) (ragged rows: 16-byte store + scalar tail) and
                                   (10,32)->(20,64) with the misaligned residual (Wout % 4 == 0, every store the 16-byte one)
(the down-scaling, degenerate and tile-boundary shapes of the same kernels are in test_image_ops_gpu.py).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from glue_ref import assert_close, assert_untouched, canary_buffer, fview, nan_wide
from vfi_amd import _lib, ops
from vfi_amd._lib import VfiLibraryError

pytestmark = pytest.mark.gpu


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---- adacof_prepare ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgbx", [False, True])
@pytest.mark.parametrize("n,h,w", [(1, 17, 33), (2, 32, 64), (2, 40, 50)])
def test_adacof_prepare_matches_reflect_pad(n, h, w, rgbx, device):
    g = _gen(n, h, w)
    f0, f2 = torch.rand((n, 3, h, w), generator=g), torch.rand((n, 3, h, w), generator=g)
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    pad = lambda f: F.pad(f, (0, wp - w, 0, hp - h), mode="reflect")
    mean = torch.tensor([0.4631, 0.4352, 0.3990], dtype=torch.float32).view(1, 3, 1, 1)
    want6 = torch.cat((pad(f0) - mean, pad(f2) - mean), 1)
    p0, p2, x6 = ops.adacof_prepare(f0.to(device), f2.to(device), rgbx=rgbx)
    if rgbx:
        assert p0.shape == (n, hp, wp, 4) and p2.shape == (n, hp, wp, 4)
        p0, p2 = p0[..., :3].permute(0, 3, 1, 2), p2[..., :3].permute(0, 3, 1, 2)
    assert p0.shape == (n, 3, hp, wp)
    assert torch.equal(p0.cpu(), pad(f0)) and torch.equal(p2.cpu(), pad(f2))
    assert x6.shape == (n, 6, hp, wp) and torch.equal(x6.cpu(), want6)


def test_adacof_prepare_rejects_a_pad_as_large_as_the_frame(device):
    f = torch.rand((1, 3, 16, 40), device=device)       # pad 16 rows: not smaller than 16
    with pytest.raises(VfiLibraryError):
        ops.adacof_prepare(f, f.clone(), rgbx=False)


# ---- pool2 ------------------------------------------------------------------------------------------------------------
def _pool_input(shape, data, g):
    if data == "dyadic":        # multiples of 1/8: many ties for max, every float32 sum of avg exact
        x = torch.randint(-24, 25, shape, generator=g).float() / 8
    else:
        x = torch.randn(shape, generator=g)
    x[0, 0] = -x[0, 0].abs() - 0.5                # an all-negative plane
    if shape[2] >= 2 and shape[3] >= 4:
        x[-1, -1, :2, :2] = x[-1, -1, 0, 0]       # a window of four equal values
        x[-1, -1, :2, 2:4] = torch.tensor([[-1.0, -1.0], [-3.0, -1.0]])
    return x


POOL_CASES = [((1, 1, 2, 2), "dense"), ((2, 3, 7, 9), "dense"), ((2, 5, 6, 10), "dense"), ((2, 5, 6, 10), "ptr_offset"),
              ((2, 5, 6, 10), "odd_bstride"), ((2, 5, 6, 10), "out_slice"), ((1, 4, 8, 34), "dense")]


@pytest.mark.parametrize("data", ["randn", "dyadic"])
@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("shape,variant", POOL_CASES)
def test_pool2(shape, variant, is_max, data, device):
    n, c, h, w = shape
    x = _pool_input(shape, data, _gen(n, c, h, w, is_max))
    if variant == "ptr_offset":          # wide[:, 1:6] of a tensor that starts one float into its allocation
        _, wide = nan_wide((n, c + 2, h, w), device, offset=1)
        xd = wide[:, 1:1 + c]
        assert xd.data_ptr() % 8 == 4 and xd.stride(0) % 2 == 0 and w % 2 == 0
    elif variant == "odd_bstride":
        flat = canary_buffer(n * (c * h * w + 1), device)
        xd = fview(flat, shape, 0, (c * h * w + 1, h * w, w, 1))
        assert xd.data_ptr() % 8 == 0 and xd.stride(0) % 2 == 1
    else:
        xd = torch.empty(shape, device=device)
    xd.copy_(x)
    if variant == "out_slice":
        flat_o, wide_o = nan_wide((n, c + 3, h // 2, w // 2), device)
        out = wide_o[:, 2:2 + c]
        assert ops.pool2(xd, is_max, out=out) is out
        assert_untouched(flat_o, out, what="pool2 out slice")
    else:
        out = ops.pool2(xd, is_max)
    assert out.shape == (n, c, h // 2, w // 2)
    if is_max:
        assert torch.equal(out.cpu(), F.max_pool2d(x, 2))
    else:
        assert_close(out, F.avg_pool2d(x, 2), F.avg_pool2d(x.double(), 2), f"pool2 avg {shape} {variant} {data}")


def test_pool2_rejects_a_single_row(device):
    with pytest.raises(VfiLibraryError):
        ops.pool2(torch.zeros((1, 2, 1, 8), device=device), True)


# ---- resize_bilinear on slices ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res_kind,out_aligned", [("misaligned", False), ("misaligned", True), (None, True), (None, False)])
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("hi,wi,ho,wo", [(10, 33, 20, 66), (10, 32, 20, 64), (5, 16, 10, 32)])
def test_resize_bilinear_slices(hi, wi, ho, wo, ac, res_kind, out_aligned, device):
    n, c, relu = 2, 5, ac
    g = _gen(hi, wi, ho, wo, ac)
    x = torch.randn((n, c, hi, wi), generator=g)
    res = torch.randn((n, c, ho, wo), generator=g)
    _, wide_x = nan_wide((n, c + 2, hi, wi), device)
    xd = wide_x[:, 1:1 + c]
    xd.copy_(x)
    rd = None
    if res_kind is not None:         # 4-byte but not 16-byte aligned
        _, wide_r = nan_wide((n, c + 2, ho, wo), device, offset=1)
        rd = wide_r[:, 1:1 + c]
        rd.copy_(res)
        assert rd.data_ptr() % 16 == 4
    flat_o, wide_o = nan_wide((n, c + 2, ho, wo), device, offset=0 if out_aligned else 1)
    out = wide_o[:, 1:1 + c]
    assert out.data_ptr() % 16 == (0 if out_aligned else 4)
    ops.resize_bilinear(xd, (ho, wo), align_corners=ac, relu_input=relu, residual=rd, out=out)
    ref = F.interpolate(F.relu(x) if relu else x, size=(ho, wo), mode="bilinear", align_corners=ac)
    if rd is not None:
        ref = ref + res
    got = out.cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 2e-6
    assert_untouched(flat_o, out, what="resize_bilinear out slice")


def test_resize_bilinear_rejects_65536_planes(device):
    x = torch.zeros((1, 65536, 1, 1), device=device)
    with pytest.raises(VfiLibraryError):
        ops.resize_bilinear(x, (1, 1), align_corners=False)


# ---- upsample2x_tapsum --------------------------------------------------------------------------------------------------
def _tapsum_ref(taps, bias, act):
    u = F.interpolate(taps, scale_factor=2, mode="bilinear", align_corners=True)
    onehot = torch.zeros((1, 9, 3, 3), dtype=taps.dtype)
    for t in range(9):
        onehot[0, t, t // 3, t % 3] = 1
    z = F.conv2d(u, onehot, padding=1) + bias
    return torch.sigmoid(z) if act == 4 else (F.relu(z) if act == 1 else z)


@pytest.mark.parametrize("act", [0, 1, 4])
@pytest.mark.parametrize("n,hs,ws", [(1, 1, 1), (2, 1, 5), (2, 3, 1), (3, 7, 11)])
def test_upsample2x_tapsum(n, hs, ws, act, device):
    taps = torch.randn((n, 9, hs, ws), generator=_gen(n, hs, ws))
    bias = 0.37
    td, out = taps.to(device), torch.full((n, 1, 2 * hs, 2 * ws), float("nan"), device=device)
    _lib.call("vfi_upsample2x_tapsum", td.data_ptr(), out.data_ptr(), n, hs, ws, bias, act, _lib.stream_ptr())
    assert_close(out, _tapsum_ref(taps, bias, act), _tapsum_ref(taps.double(), bias, act), f"tapsum {(n, hs, ws)} act {act}")


def test_upsample2x_tapsum_rejects_an_unknown_act(device):
    taps, out = torch.zeros((1, 9, 2, 2), device=device), torch.zeros((1, 1, 4, 4), device=device)
    with pytest.raises(VfiLibraryError):
        _lib.call("vfi_upsample2x_tapsum", taps.data_ptr(), out.data_ptr(), 1, 2, 2, 0.0, 9, _lib.stream_ptr())


# ---- softmax_channels_ --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("n,c,h,w", [(1, 1, 1, 1), (2, 2, 1, 3), (2, 25, 3, 5), (3, 49, 31, 33)])
def test_softmax_channels_in_place(n, c, h, w, sliced, device):
    x = torch.randn((n, c, h, w), generator=_gen(n, c, h, w)) * 4
    x[0, 0, 0, 0] = 80.0
    x[-1, -1, -1, -1] = -80.0
    if c > 1:
        x[-1, 0, -1, -1] = 80.0             # +80 and -80 in one pixel
    if w > 1:
        x[0, :, 0, 1] = 1.25                # all logits equal
    if sliced:
        flat, wide = nan_wide((n, c + 5, h, w), device)
        xd = wide[:, 3:3 + c]
        xd.copy_(x)
    else:
        xd = x.to(device)
    assert ops.softmax_channels_(xd) is xd
    if sliced:
        assert_untouched(flat, xd, what="softmax slice")
    ref64 = torch.softmax(x.double(), 1)
    _, tol = assert_close(xd, torch.softmax(x, 1), ref64, f"softmax {(n, c, h, w)} sliced={sliced}")
    rows = (xd.cpu().double().sum(1) - 1).abs().max().item()
    print(f"softmax {(n, c, h, w)}: |row sum - 1| {rows:.3e} tol {tol:.3e}")
    assert rows <= tol, f"rows sum to 1 within {tol:.3e}: {rows:.3e}"


# ---- affine_slice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("count", [1, 3, 4, 1023, 4100])
def test_affine_slice(n, count, device):
    g = _gen(n, count)
    src = torch.randn((n, 1, 1, count), generator=g)
    div = torch.rand((n,), generator=g) + 0.5
    inv_pi = torch.tensor(1.0 / math.pi, dtype=torch.float32)
    dv = div.view(n, 1, 1, 1)

    def run(kind, with_div, mul):
        sd, flat, dd = src.to(device), None, None
        if kind == "src_slice":
            _, wide = nan_wide((n, 3, 1, count), device)
            sd = wide[:, 1:2]
            sd.copy_(src)
        if kind == "in_place":
            dd = sd
        elif kind == "dst_slice":
            flat, wide = nan_wide((n, 4, 1, count), device)
            dd = wide[:, 2:3]
        else:
            dd = torch.full((n, 1, 1, count), float("nan"), device=device)
        assert ops.affine_slice(sd, dd, div.to(device) if with_div else None, mul) is dd
        if flat is not None:
            assert_untouched(flat, dd, what=f"affine_slice {kind}")
        what = f"affine_slice n={n} count={count} {kind} div={with_div} mul={mul:.4f}"
        if not with_div:             # one multiplication (or a plain copy): exact
            want = src * (inv_pi if mul != 1.0 else torch.tensor(1.0))
            assert torch.equal(dd.cpu(), want), what
        else:
            assert_close(dd, src / dv * (inv_pi if mul != 1.0 else 1.0), src.double() / dv.double() * mul, what)

    for kind in ("dense", "dst_slice", "in_place", "src_slice"):
        for with_div in (False, True):
            for mul in (1.0, 1.0 / math.pi):
                run(kind, with_div, mul)


def test_affine_slice_rejects_a_shape_mismatch(device):
    with pytest.raises(VfiLibraryError):
        ops.affine_slice(torch.zeros((2, 1, 1, 8), device=device), torch.zeros((2, 1, 1, 9), device=device))


# ---- batch_max ----------------------------------------------------------------------------------------------------------
def _batch_max_want(x, eps):
    return x.reshape(x.shape[0], -1).max(1)[0] + torch.tensor(eps, dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_batch_max(n, count, device):
    g = _gen(n, count)
    base = torch.randn((n, 1, 1, count), generator=g)
    eps = 0.25
    inputs = {"negative": -base.abs() - 0.5}
    first, last = base.clone().clamp_(max=3.0), base.clone().clamp_(max=3.0)
    first[..., 0] = torch.arange(5, 5 + n).float().view(n, 1, 1)
    last[..., -1] = torch.arange(5, 5 + n).float().view(n, 1, 1)
    inputs["max_first"], inputs["max_last"] = first, last
    zeros = torch.zeros((n, 1, 1, count))
    zeros[..., ::2] = -0.0
    inputs["signed_zeros"] = zeros
    for kind, x in inputs.items():
        e = 1e-8 if kind == "signed_zeros" else eps
        got = ops.batch_max(x.to(device), e)
        assert torch.equal(got.cpu(), _batch_max_want(x, e)), (kind, got.cpu(), _batch_max_want(x, e))
    # a channel slice of a wider tensor whose other channels hold larger values (and the garbage the calls above left in
    # the workspace the allocator hands out again)
    wide = torch.full((n, 3, 1, count), 1e30, device=device)
    x = inputs["negative"]
    wide[:, 1:2].copy_(x)
    assert torch.equal(ops.batch_max(wide, 0.0).cpu(), torch.full((n,), 1e30))
    got = ops.batch_max(wide[:, 1:2], eps)
    assert torch.equal(got.cpu(), _batch_max_want(x, eps)), ("slice", got.cpu())


def test_batch_max_of_8_mb_per_sample_with_the_maximum_last(device):
    n, count = 2, 1024 * 256 * 8 + 1            # one element more than 1024 blocks x 256 threads x 8 cover in one sweep
    x = torch.rand((n, 1, 1, count), generator=_gen(n, count)) - 2.0
    x[0, ..., -1], x[1, ..., -1] = -0.5, 7.0
    got = ops.batch_max(x.to(device), 1e-8)
    assert torch.equal(got.cpu(), _batch_max_want(x, 1e-8)), got.cpu()


def test_batch_max_ignores_what_an_earlier_call_left_in_its_workspace(device):
    """ops.batch_max allocates its int32 workspace uninitialised: the encodings of a first call (large positive maxima)
    are what a second call of the same size most likely gets back from the allocator."""
    n, count = 3, 257
    big = torch.full((n, 1, 1, count), 3e38, device=device)
    assert torch.equal(ops.batch_max(big, 0.0).cpu(), torch.full((n,), 3e38))
    del big
    x = -torch.rand((n, 1, 1, count), generator=_gen(n, count, 1)) - 1.0
    assert torch.equal(ops.batch_max(x.to(device), 0.25).cpu(), _batch_max_want(x, 0.25))


# ---- phasenet_emit / phasenet_emit_low --------------------------------------------------------------------------------
def _emit_ref(pred, amp_in, mx):
    """phase_net.py:155-156,167-168 and reverse_normalize :83,89 of the reference, for two input frames."""
    n, _, h, w = pred.shape
    beta = (pred[:, 4:8] + 1) / 2
    amplitude = beta * amp_in[:, 4:8] + (1 - beta) * amp_in[:, :4]
    phase = pred[:, :4] * math.pi
    amplitude = amplitude * mx.view(n, 1, 1, 1)
    return phase.reshape(-1, 1, h, w), amplitude.reshape(-1, 1, h, w)


def _emit_low_ref(pred, low_in, mx):
    """phase_net.py:115-116,124 and :98."""
    alpha = (pred[:, 0] + 1) / 2
    low = alpha * low_in[:, 0] + (1 - alpha) * low_in[:, 1]
    return (low * mx.view(-1, 1, 1)).unsqueeze(1)


def _pred_like(shape, g):
    p = torch.rand(shape, generator=g) * 2 - 1
    flat = p.view(-1)
    flat[::5] = 1.0                     # beta / alpha exactly 1 ...
    flat[2::7] = -1.0                   # ... and exactly 0
    return p


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_phasenet_emit_matches_the_formulas(n, hw, device):
    g = _gen(n, hw)
    pred = _pred_like((n, 8, 1, hw), g)
    amp_in = torch.rand((n, 8, 1, hw), generator=g)
    mx = torch.rand((n,), generator=g) * 3 + 0.1
    _, wide_p = nan_wide((n, 72, 1, hw), device)
    pd = wide_p[:, 64:]
    pd.copy_(pred)
    _, wide_a = nan_wide((n, 81, 1, hw), device)          # the block input: 64 + 1 + 8 phases, then the amplitudes
    ad = wide_a[:, 73:]
    ad.copy_(amp_in)
    phase, amp = ops.phasenet_emit(pd, ad, mx.to(device))
    p32, a32 = _emit_ref(pred, amp_in, mx)
    p64, a64 = _emit_ref(pred.double(), amp_in.double(), mx.double())
    assert_close(phase, p32, p64, f"phasenet_emit phase n={n} hw={hw}")
    assert_close(amp, a32, a64, f"phasenet_emit amp n={n} hw={hw}")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_phasenet_emit_low_matches_the_formulas(n, hw, device):
    g = _gen(n, hw, 2)
    pred = _pred_like((n, 1, 1, hw), g)
    low_in = torch.randn((n, 2, 1, hw), generator=g)
    mx = torch.rand((n,), generator=g) * 3 + 0.1
    _, wide_p = nan_wide((n, 65, 1, hw), device)
    pd = wide_p[:, 64:]
    pd.copy_(pred)
    low = ops.phasenet_emit_low(pd, low_in.to(device), mx.to(device))
    assert_close(low, _emit_low_ref(pred, low_in, mx), _emit_low_ref(pred.double(), low_in.double(), mx.double()),
                 f"phasenet_emit_low n={n} hw={hw}")


# ---- tanh_residual_clamp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 1023, 4100])
def test_tanh_residual_clamp(count, device):
    g = _gen(count)
    x = (torch.rand((1, 1, 1, count), generator=g) * 2 - 1) * 20
    x.view(-1)[::3] /= 16                               # a third of the samples where tanh is not saturated
    base = torch.rand((1, 1, 1, count), generator=g) * 2 - 0.5
    if count == 1:
        x[...], base[...] = 20.0, 0.75                  # saturated tanh, upper clamp
    if count >= 3:
        x.view(-1)[:3] = torch.tensor([-20.0, 20.0, 0.25])
        base.view(-1)[:3] = torch.tensor([0.5, 1.5, 0.25])
    # keep every sum away from the clamp points, so that which side it falls on does not hang on one float32 rounding
    s = base.double() + torch.tanh(x.double())
    near = ((s - 1).abs() < 1e-5) | (s.abs() < 1e-5)
    base[near] += 0.01
    pre64 = base.double() + torch.tanh(x.double())
    ref64 = pre64.clamp(0, 1)
    ref32 = (base + torch.tanh(x)).clamp(0, 1)
    got = ops.tanh_residual_clamp(x.to(device), base.to(device)).cpu()
    assert_close(got, ref32, ref64, f"tanh_residual_clamp count={count}")
    lo, hi = pre64 < 0, pre64 > 1
    if count >= 3:
        assert lo.any() and hi.any() and (~lo & ~hi).any()
    assert (got[lo] == 0.0).all() and (got[hi] == 1.0).all()
