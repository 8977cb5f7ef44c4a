"""PhaseNet's band-level head (vfi_phasenet_predict, vfi_phasenet_predict_n) and its one-pass tail (vfi_phasenet_level_tail)
against a float64 restatement, element by element, each element within a bound derived for it (tests/phasenet_head_ref.py).

The sibling comparisons (test_phasenet_predict_equals_conv_then_emit, test_predict_n_equals_conv_then_emit_n,
test_level_tail_equals_predict_then_resize) hold these kernels against one another, and they share their arithmetic: an error
common to them passes.  Here every output is filled with a sentinel before the call; after it every element inside must lie
within its bound, everything outside must still be the sentinel (planes 72..87 of the target, the gap between batch strides, the
floats before and after each buffer), and the inputs must be unchanged.  Every level-tail case first asserts which launches
the library takes for it (vfi_phasenet_level_tail_path), so a case that is here for the one-pass kernel cannot pass through the
two-launch form unnoticed.

Measured worst error over bound per case and output kind: DESIGN.md, "The level head against float64"."""
import functools

import pytest
import torch

import phasenet_head_ref as H

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 8            # floats in front of and behind every buffer (32 bytes: keeps 16-byte alignment)
TWO_LAUNCHES, ONE_PASS, ONE_PASS_VEC = 0, 1, 2          # VFI_TAIL_PATH_*


def _carve(flat, off, shape, bstride):
    """(N,C,H,W) view of a flat buffer from float offset GUARD + off on, samples bstride floats apart."""
    n, c, h, w = shape
    assert flat.data_ptr() % 16 == 0 and GUARD + off + (n - 1) * bstride + c * h * w <= flat.numel() - GUARD
    return torch.as_strided(flat, shape, (bstride, h * w, w, 1), GUARD + off)


def _buffer(n, bstride, device, slack=4):
    return torch.full((2 * GUARD + n * bstride + slack,), SENTINEL, device=device)


def _outside_untouched(flat, view):
    """Every float of `flat` outside `view` (a view of it) still holds the sentinel."""
    inside = torch.zeros(flat.shape, dtype=torch.bool, device=flat.device)
    torch.as_strided(inside, view.shape, view.stride(), view.storage_offset()).fill_(True)
    return bool((flat[~inside] == SENTINEL).all())


def _within(what, got, ref_bound):
    """Every element within its bound; prints the worst error over bound first.  A NaN fails."""
    ref, bound = ref_bound
    err = (got.double() - ref).abs()
    ratio = err / bound
    print(f"RATIO {what}: worst error/bound {float(ratio.max()):.3f} (error {float(err.max()):.3e})")
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), float(ratio.nan_to_num(float("inf")).max()), bad.nonzero()[:4].tolist())


@functools.lru_cache(maxsize=1)
def _draw(n, h, w, p, num_img):
    """The inputs of a case, on the CPU: features randn, amplitudes rand, max in [0.5, 1.5], the map randn / 8, bias 0.1 randn."""
    g = torch.Generator().manual_seed((h * 4099 + w) * 16 + n + 1000003 * p)        # (no two cases share their draw)
    fp = torch.randn((n, 80, h, w), generator=g)
    x = torch.rand((n, 64 + p + 8 * num_img, h, w), generator=g)
    mx = torch.rand((n,), generator=g) + 0.5
    wt = torch.randn((p, 64, 1, 1), generator=g) / 8.0
    b = torch.randn((p,), generator=g) * 0.1
    return fp, x, mx, wt, b


# ---- vfi_phasenet_level_tail ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _tail_reference(n, h, w, ho, wo, with_bias, fallback, device):
    """The float64 reference of a case, computed once and shared by the cases that differ only in where the buffers lie."""
    fp, x, mx, wt, b = (t.to(device) for t in _draw(n, h, w, 8, 2))
    return H.tail64(fp[:, :64], wt.view(8, 64), b if with_bias else None, x[:, 80:], mx, ho, wo, fallback)


def _run_tail(device, n, h, w, ho, wo, path, feat_off=0, amp_off=0, next_off=0, next_pad=0, with_bias=True):
    from vfi_amd import _lib, ops
    vals_fp, vals_x, vals_mx, wt, b = _draw(n, h, w, 8, 2)
    hw, hwo = h * w, ho * wo
    fp_flat, x_flat = _buffer(n, 80 * hw, device), _buffer(n, 88 * hw, device)
    fp, x = _carve(fp_flat, feat_off, (n, 80, h, w), 80 * hw), _carve(x_flat, amp_off, (n, 88, h, w), 88 * hw)     # features = fp[:, :64]
    fp.copy_(vals_fp)
    x.copy_(vals_x)
    amp_in = x[:, 80:]
    mx = vals_mx.to(device)
    pc = ops.PackedConv(wt, b, device=device)
    nb = 88 * hwo + next_pad
    xn_flat = _buffer(n, nb, device)
    x_next = _carve(xn_flat, next_off, (n, 88, ho, wo), nb)[:, :72]
    p_flat, a_flat = _buffer(n, 4 * hw, device), _buffer(n, 4 * hw, device)
    p_out, a_out = _carve(p_flat, 0, (n, 4, h, w), 4 * hw), _carve(a_flat, 0, (n, 4, h, w), 4 * hw)
    fp_before, x_before, mx_before, packed_before = fp_flat.clone(), x_flat.clone(), mx.clone(), pc.packed.clone()
    args = (fp.data_ptr(), fp.stride(0), pc.packed.data_ptr(), pc.bias.data_ptr() if with_bias else None, amp_in.data_ptr(), x.stride(0),
            mx.data_ptr(), x_next.data_ptr(), x_next.stride(0), p_out.data_ptr(), a_out.data_ptr(), n, h, w, ho, wo)
    assert fp.data_ptr() % 16 == 4 * feat_off % 16 and amp_in.data_ptr() % 16 == 4 * (amp_off + 80 * hw) % 16
    assert x_next.data_ptr() % 16 == 4 * next_off % 16 and p_out.data_ptr() % 16 == 0 and a_out.data_ptr() % 16 == 0

    assert _lib.lib().vfi_phasenet_level_tail_path(*args) == path
    # every CU's LDS full of NaNs: a window element that is read without having been staged shows even where its weight is 0
    _lib.call("vfi_debug_poison_lds", _lib.stream_ptr())
    _lib.call("vfi_phasenet_level_tail", *args, _lib.stream_ptr())
    torch.cuda.synchronize()

    ref = _tail_reference(n, h, w, ho, wo, with_bias, path == TWO_LAUNCHES, device)
    case = f"tail {n}x{h}x{w}->{ho}x{wo} path {path} offsets {feat_off},{amp_off},{next_off}+{next_pad}{'' if with_bias else ' no bias'}"
    _within(case + " phase", p_out, ref["phase"])
    _within(case + " amp", a_out, ref["amp"])
    nxt, e_next = ref["next"]
    _within(case + " resized features", x_next[:, :64], (nxt[:, :64], e_next[:, :64]))
    _within(case + " resized prediction", x_next[:, 64:], (nxt[:, 64:], e_next[:, 64:]))
    assert _outside_untouched(xn_flat, x_next)               # planes 72..87, the gap between samples, the guards
    assert _outside_untouched(p_flat, p_out) and _outside_untouched(a_flat, a_out)
    assert torch.equal(fp_flat, fp_before) and torch.equal(x_flat, x_before)          # the inputs are only read
    assert torch.equal(mx, mx_before) and torch.equal(pc.packed, packed_before)


@pytest.mark.parametrize("n,h,w,ho,wo,path", [
    (2, 64, 64, 64, 64, ONE_PASS_VEC),            # scale exactly 1: one partial tile column, 17-row windows (the 17th at weight 0)
    (2, 62, 68, 64, 70, ONE_PASS),                # just above 1: 17-row windows whose last row carries weight (0.016 and 0.516)
    (1, 4, 1024, 5, 1449, ONE_PASS),              # windows of at most 5 rows (fewer than thread rows), 12 tile columns, odd width
    (1, 1024, 4, 1449, 6, ONE_PASS),              # windows of 4 columns, 91 tile rows, one quad stored whole and one by elements
    (3, 46, 90, 65, 127, ONE_PASS),               # width TX - 1; last tile row of one row
    (1, 64, 66, 128, 132, ONE_PASS_VEC),          # exactly x2; second tile column of 4 columns
    (1, 32, 128, 256, 1024, ONE_PASS_VEC),        # x8: 9-row windows
    (2, 50, 82, 71, 129, ONE_PASS),               # second tile column of one column
    (1, 48, 86, 48, 258, ONE_PASS),               # scale 1 down, x3 across, width = 2 mod 4
    (3, 135, 240, 191, 340, ONE_PASS_VEC),        # a level pair of the 1080p pyramid at batch 3
    (2, 70, 60, 64, 64, TWO_LAUNCHES),            # fewer rows than the source (8 HW <= 64 HWo allows it): the two launches
    (2, 65, 67, 92, 95, TWO_LAUNCHES),            # an odd plane: vfi_phasenet_predict does not stream
])
def test_level_tail_within_float64_bounds(n, h, w, ho, wo, path, device):
    _run_tail(device, n, h, w, ho, wo, path)


@pytest.mark.parametrize("kw,path", [
    (dict(next_off=1), ONE_PASS),                 # x_next one float past a 16-byte boundary: 16-byte stores at 4-byte alignment
    (dict(next_pad=1), ONE_PASS),                 # a batch stride of x_next that is no multiple of 4: the same from sample 1 on
    (dict(feat_off=2, amp_off=2), ONE_PASS_VEC),  # features and amplitudes 8 bytes past: the one-pass kernel still runs
    (dict(feat_off=1), TWO_LAUNCHES),             # features 4 bytes past: nothing streams
    (dict(with_bias=False), ONE_PASS_VEC),        # a map without bias: a null pointer
])
def test_level_tail_alignment_cases(kw, path, device):
    """64x66 -> 128x132 (Wout a multiple of 4) from buffers that start off a 16-byte boundary; batch 2, so that the batch strides
    count."""
    _run_tail(device, 2, 64, 66, 128, 132, path, **kw)


# ---- vfi_phasenet_predict, vfi_phasenet_predict_n ---------------------------------------------------------------------------------
# Which kernel runs is conv1x1_stream_vec's rule (csrc/vfi_conv.hip) on the features and the prediction planes, narrowed by the
# alignment of the amplitudes and outputs: H W >= 4096, and pointers, batch strides and 4 H W all multiples of 16 bytes -> four
# pixels per thread; of 8 bytes -> two pixels per thread; else the matrix-core 1x1 convolution followed by vfi_phasenet_emit[_n].
# All of them must meet the same bound.
@pytest.mark.parametrize("num_img", [2, 3])
@pytest.mark.parametrize("n,h,w,off", [
    (3, 64, 64, 0),             # four pixels per thread
    (1, 2, 2049, 0),            # 4 H W = 8 mod 16: two pixels per thread
    (3, 50, 82, 0),             # H W / 4 = 1025: one thread in the last block
    (1, 64, 64, 2),             # features and prediction 8 bytes past a 16-byte boundary: two pixels per thread by pointer
    (1, 1, 4097, 0),            # an odd plane: matrix cores
    (3, 65, 63, 0),             # 4095 pixels, planes at 4-byte alignment: matrix cores
])
def test_predict_within_float64_bounds(n, h, w, off, num_img, device):
    """num_img = 3: the 64 -> 12 map, 12 amplitude planes and the second blend (vfi_phasenet_predict_n)."""
    from vfi_amd import _lib, ops
    p = 12 if num_img == 3 else 8
    vals_fp, vals_x, vals_mx, wt, b = _draw(n, h, w, p, num_img)
    hw = h * w
    cx = vals_x.shape[1]
    fp_flat, x_flat = _buffer(n, 80 * hw, device), _buffer(n, cx * hw, device)
    fp, x = _carve(fp_flat, off, (n, 80, h, w), 80 * hw), _carve(x_flat, 0, (n, cx, h, w), cx * hw)
    fp[:, :64].copy_(vals_fp[:, :64])                       # planes 64..79 keep the sentinel: the prediction goes to 64..64+p
    x.copy_(vals_x)
    amp_in = x[:, 64 + p + 4 * num_img:]
    assert amp_in.shape[1] == 4 * num_img
    mx = vals_mx.to(device)
    pc = ops.PackedConv(wt, b, device=device)
    pred = fp[:, 64:64 + p]
    p_flat, a_flat = _buffer(n, 4 * hw, device), _buffer(n, 4 * hw, device)
    p_out, a_out = _carve(p_flat, 0, (n, 4, h, w), 4 * hw), _carve(a_flat, 0, (n, 4, h, w), 4 * hw)
    feat_before, x_before = fp[:, :64].clone(), x_flat.clone()
    args = (fp.data_ptr(), fp.stride(0), pc.packed.data_ptr(), pc.bias.data_ptr(), amp_in.data_ptr(), x.stride(0), mx.data_ptr(),
            pred.data_ptr(), fp.stride(0), p_out.data_ptr(), a_out.data_ptr(), n, 64, h, w)
    if num_img == 2:
        _lib.call("vfi_phasenet_predict", *args, _lib.stream_ptr())
    else:
        _lib.call("vfi_phasenet_predict_n", *args, num_img, _lib.stream_ptr())
    torch.cuda.synchronize()

    ref = H.head64(fp[:, :64], wt.view(p, 64).to(device), b.to(device), amp_in, mx, num_img)
    case = f"predict num_img {num_img} {n}x{h}x{w} offset {off}"
    _within(case + " pred", pred, ref["pred"])
    _within(case + " phase", p_out, ref["phase"])
    _within(case + " amp", a_out, ref["amp"])
    assert _outside_untouched(fp_flat, fp[:, :64 + p])       # planes 64+p..79, the guards
    assert _outside_untouched(p_flat, p_out) and _outside_untouched(a_flat, a_out)
    assert torch.equal(fp[:, :64], feat_before) and torch.equal(x_flat, x_before)


# ---- the one measured number ------------------------------------------------------------------------------------------------------
def test_device_tanh_stays_within_its_allowance(device):
    """The device's tanhf alone: a 1 -> 1 1x1 map of weight 1 without bias through the streaming kernel -- fmaf(1, x, 0) + 0 is
    exact -- over 2^16 inputs spanning [-4, 4] and the same scaled into [-0.05, 0.05], against float64 tanh.  The allowance A of
    the bounds is twice the worst value measured (phasenet_head_ref.TANH_MEASURED); above 5 ulp of 1 the error would be a
    finding about tanhf, not something for A to absorb."""
    from vfi_amd import ops
    pc = ops.PackedConv(torch.ones((1, 1, 1, 1)), None, device=device)
    wide = torch.linspace(-4.0, 4.0, 2 ** 16, dtype=torch.float64).float()
    worst = 0.0
    for v in (wide, (wide * 0.0125).float()):
        y = ops.conv2d(v.to(device).view(1, 1, 256, 256), pc, "zeros", "tanh")
        torch.cuda.synchronize()
        err = float((y.double().view(-1) - torch.tanh(v.double().to(device))).abs().max())
        print(f"RATIO tanhf over [{float(v.min()):.4f}, {float(v.max()):.4f}]: worst error {err:.4e}")
        worst = max(worst, err)
    assert worst <= H.TANH_FINDING
    assert worst <= H.TANH_ALLOWANCE
