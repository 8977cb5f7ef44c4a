"""Float64 restatement of PhaseNet's band-level head and of its one-pass tail, with a derived error bound per element.

The operations: the 64 -> 8 (three images: 64 -> 12) tanh map over the block's feature planes, the level's phase and amplitude
(vfi_phasenet_predict, vfi_phasenet_predict_n), and the bilinear resize, align_corners=False, of [feature 64 | prediction 8]
into the next level's block input (vfi_phasenet_level_tail, or vfi_resize_bilinear in its two-launch form).  The head formulas
are phasenet_walk_ref.head_forward and phasenet_fusion_grad_ref.head_forward, called on float64 tensors; the resize is
`resize64` below.  Everything works on any torch device (the tests run it in float64 on the GPU, through torch's own kernels).

Every function returns the float64 values and, next to them, a bound on |device value - float64 value| for EVERY element.  The
bounds are derived here, not measured; the one measured number is TANH_ALLOWANCE.  u = 2^-24 is float32's unit roundoff: one
rounding changes a value x by at most u |x|.

Prediction, e_pred = 66 u S + A, with S = sum_c |w_c x_c| + |b| per pixel and output (evaluated in float64).
    The device sums the 64 products and the bias in float32 -- one fused multiply-add per channel in the streaming kernels,
    multiply and add rounded separately and in another order in the matrix-core kernel.  Either way the computed sum is
    sum_c w_c x_c (1 + d_c) + b (1 + d_b) with |d| <= (1 + u)^65 - 1 (Higham, Accuracy and Stability of Numerical Algorithms,
    section 3.1: each term meets at most 64 additions and one multiplication, whatever the order), which is below 66 u.  tanh
    has slope <= 1, so the error of its argument passes through at most unchanged.  A bounds what the device's tanhf adds, its
    final rounding included.

Phase, e_phase = pi e_pred + 2 u pi |pred|.
    phase = fl(pred * fl(pi)).  The prediction's error is scaled by pi.  float32's pi is off by 0.47 u relative, the product is
    rounded once (u): 1.47 u |pred| pi, counted as 2 u; the rest covers that |pred| is the reference's, not the device's.

Amplitude, e_amp = ((e_pred / 2 + u) (|a0| + |a1|) + 4 u max(|a0|, |a1|)) mx + u |amp|.
    beta = fl(fl(pred + 1) / 2): the sum lies in [0, 2] and is rounded once, halving is exact: |error of beta| <= e_pred / 2 + u.
    1 - beta is rounded once more (u), the product (1 - beta) a0 once (u |a0|), the fused beta a1 + ... once (u max): the blend
    a is off by at most (e_pred / 2 + u)(|a0| + |a1|) + 3 u max(|a0|, |a1|), counted with 4 u.  amp = fl(a mx) scales that by mx
    and rounds once: u |amp|.  Three images: the second blend a' = fb a + (1 - fb) a2 with fb from prediction 8 + b is bounded
    the same way, (e_pred' / 2 + u)(|a| + |a2|) + 4 u max(|a|, |a2|), plus the first blend's own error, which enters with the
    weight fb <= 1.

Resized planes, e = 8 u M + E, with M the largest magnitude among the element's four taps and E the largest input bound among
them (0 for the feature planes, which the device reads exactly; e_pred for the prediction planes).
    The tap indices and the fractions lx, ly are float32 values which the reference takes over bit for bit (below), so the
    error is that of evaluating (1 - ly)((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11) in float32.  Each tap's path to the
    result meets at most six roundings without contraction (1 - lx, the product, the sum, 1 - ly, the product, the sum), five or
    fewer with it; all intermediate values are convex combinations of the taps up to these roundings, so each rounding is at
    most u M (1 + O(u)): 6 u M, counted as 8 u M.  The weights are non-negative and sum to one up to the roundings already
    counted, so input errors combine to at most their maximum.

Coordinates.  vfi::tail::src_coord is max(fmaf(scale, o + 0.5, -0.5), 0) with scale = fl(in / out): coord="fma" reproduces it
    exactly -- scale (24 bits) times o + 0.5 (at most 12 bits for o < 2048) is exact in float64, so scale (o + 0.5) - 0.5
    evaluated in float64 and rounded to float32 is rounded once, as fmaf rounds.  Index min(int(c), in - 1), fraction c - index
    in float32 (exact).  The one-pass kernel's resized planes therefore get no coordinate term.

Fallback resize (resize_bilinear_*_kernel in vfi_aux.hip), e += coordinate term.
    These kernels spell the coordinate sy * (yo + 0.5f) - 0.5f, which the compiler may contract into the fmaf above or round
    twice.  Rounded twice it is g = fl(fl(p) - 0.5) = fl(p) - 0.5 exactly (a multiple of ulp(p) of smaller magnitude), with
    p = scale (o + 0.5); contracted it is f = fl(p - 0.5).  |g - f| <= ulp(p) / 2 + ulp(f) / 2.  `taps` computes both in float32
    and `resize64_bound(coord_slack=True)` asserts |g - f| <= ulp(f), one float32 ulp of the coordinate, at every index of the
    shape at hand before using that figure.  Bilinear interpolation is continuous and piecewise linear in each coordinate with
    slope at most the largest difference of adjacent source pixels, also across an integer (where the floor of f and g may
    differ): the term is ulp(fy) dY + ulp(fx) dX, dY and dX the largest |difference| of vertically resp. horizontally adjacent
    source pixels in rows y0..y1 and columns x0-1..x1+1.

TANH_ALLOWANCE (A) is twice the worst |tanhf(x) - tanh(x)| measured on the device over 2^16 inputs spanning [-4, 4] and the same
scaled into [-0.05, 0.05] (tests/test_phasenet_head_f64_gpu.py: test_device_tanh_stays_within_its_allowance repeats the
measurement).  5 ulp of 1 (6e-7, OpenCL's full-profile tanh) is the limit beyond which it would be a finding, not an allowance.
"""
import math

import torch

import phasenet_fusion_grad_ref as FG
import phasenet_walk_ref as W

U = 2.0 ** -24
TANH_MEASURED = 7.345116e-08           # worst |tanhf - tanh| found on an MI355X: at x = -0.64972913 (0.62 ulp of 1); 1.9e-09 on [-0.05, 0.05]
TANH_ALLOWANCE = 2 * TANH_MEASURED
TANH_FINDING = 5 * 2.0 ** -23          # 5 ulp of 1


def head64(feat, w, b, amp_in, max_amp, num_img=2):
    """feat (N,64,H,W), w (P,64), b (P,) or None, amp_in (N,4*num_img,H,W), max_amp (N,): float32 tensors of one device.
    -> {"pred", "phase", "amp"} -> (float64 values, per-element bound); pred (N,P,H,W), phase and amp (N,4,H,W)."""
    f, w, a, mx = feat.double(), w.double(), amp_in.double(), max_amp.double()
    b = torch.zeros(w.shape[0], dtype=torch.float64, device=w.device) if b is None else b.double()
    if num_img == 2:
        pred, phase, amp = W.head_forward(f, w, b, a, mx)
    else:
        pred, phase, amp = FG.head_forward(f, w, b, a, mx, num_img)
    s = torch.einsum("jk,nkhw->njhw", w.abs(), f.abs()) + b.abs().view(1, -1, 1, 1)
    e_pred = 66 * U * s + TANH_ALLOWANCE
    e_phase = math.pi * e_pred[:, :4] + 2 * U * math.pi * pred[:, :4].abs()
    a0, a1 = a[:, :4].abs(), a[:, 4:8].abs()
    e_a = (e_pred[:, 4:8] / 2 + U) * (a0 + a1) + 4 * U * torch.maximum(a0, a1)
    if num_img == 3:
        beta = (pred[:, 4:8] + 1) / 2
        blend, a2 = (beta * a[:, 4:8] + (1 - beta) * a[:, :4]).abs(), a[:, 8:12].abs()
        e_a = e_a + (e_pred[:, 8:12] / 2 + U) * (blend + a2) + 4 * U * torch.maximum(blend, a2)
    e_amp = e_a * mx.view(-1, 1, 1, 1) + U * amp.abs()
    return {"pred": (pred, e_pred), "phase": (phase, e_phase), "amp": (amp, e_amp)}


def taps(n_in, n_out, device="cpu"):
    """Along one axis -> (i0, i1 int64, fraction float64, f, g float32): f the coordinate with one rounding (fmaf:
    vfi::tail::src_coord), g the one with two (product, then the subtraction); indices and fraction are f's."""
    o = torch.arange(n_out, dtype=torch.float64, device=device)
    scale = torch.tensor(float(n_in), dtype=torch.float32, device=device) / torch.tensor(float(n_out), dtype=torch.float32, device=device)
    assert n_out < 2 ** 27                                    # scale * (o + 0.5) exact in float64
    p = scale.double() * (o + 0.5)
    f = (p - 0.5).float().clamp_min(0.0)
    g = (p.float() - 0.5).clamp_min(0.0)                      # (float32 - 0.5 -> float32: rounded, as the device would)
    i0 = f.long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    frac = f - i0.float()
    assert bool((frac.double() == f.double() - i0.double()).all())        # the float32 subtraction is exact
    return i0, i1, frac.double(), f, g


def _gather(src, y, x):
    return src[..., y, :][..., x]


def resize64(src, ho, wo, coord="fma"):
    """torch's bilinear resize, align_corners=False, of (..., h, w) planes: the four-tap combination in float64, tap indices
    and fractions from float32 coordinates.  coord="fma": the coordinate of vfi::tail::src_coord, bit for bit."""
    assert coord == "fma"
    src = src.double()
    h, w = src.shape[-2:]
    y0, y1, ly, _, _ = taps(h, ho, src.device)
    x0, x1, lx, _, _ = taps(w, wo, src.device)
    ly = ly[:, None]
    top = (1.0 - lx) * _gather(src, y0, x0) + lx * _gather(src, y0, x1)
    bot = (1.0 - lx) * _gather(src, y1, x0) + lx * _gather(src, y1, x1)
    return (1.0 - ly) * top + ly * bot


def _tap_max(t, y0, y1, x0, x1):
    return torch.maximum(torch.maximum(_gather(t, y0, x0), _gather(t, y0, x1)), torch.maximum(_gather(t, y1, x0), _gather(t, y1, x1)))


def resize64_bound(src, ho, wo, err=None, coord_slack=False):
    """Bound of the resized planes of `src` (..., h, w): 8 u M + E (module docstring); err = the per-element bound of src (None:
    exact inputs).  coord_slack: add the coordinate term of the fallback kernels."""
    src = src.double()
    h, w = src.shape[-2:]
    y0, y1, _, fy, gy = taps(h, ho, src.device)
    x0, x1, _, fx, gx = taps(w, wo, src.device)
    bound = 8 * U * _tap_max(src.abs(), y0, y1, x0, x1)
    if err is not None:
        bound = bound + _tap_max(err, y0, y1, x0, x1)
    if coord_slack:
        ulp_y, ulp_x = _ulp32(fy), _ulp32(fx)
        assert bool(((gy - fy).abs().double() <= ulp_y).all()) and bool(((gx - fx).abs().double() <= ulp_x).all())
        # largest |difference| of vertically adjacent pixels, rows y0..y1 (one pair), columns x0-1..x1+1
        dv = torch.zeros_like(src)
        dv[..., :-1, :] = (src[..., 1:, :] - src[..., :-1, :]).abs()          # dv[y] = |src[y+1] - src[y]|; y0 == y1 at the last row: 0
        d_y = None
        for dx in (-1, 0, 1, 2):
            xs = (x0 + dx).clamp(0, w - 1)
            t = _gather(dv, y0, xs)
            d_y = t if d_y is None else torch.maximum(d_y, t)
        # ... of horizontally adjacent pixels, rows y0 and y1, pairs (x0-1,x0), (x0,x0+1), (x0+1,x0+2)
        dh = torch.zeros_like(src)
        dh[..., :, :-1] = (src[..., :, 1:] - src[..., :, :-1]).abs()
        d_x = None
        for dx in (-1, 0, 1):
            xs = (x0 + dx).clamp(0, w - 1)
            t = torch.maximum(_gather(dh, y0, xs), _gather(dh, y1, xs))
            d_x = t if d_x is None else torch.maximum(d_x, t)
        bound = bound + ulp_y[:, None] * d_y + ulp_x * d_x
    return bound


def _ulp32(c):
    """Spacing of float32 at c >= 0 (float32 tensor) -> float64; the smallest normal's spacing below it."""
    e = torch.frexp(c.clamp_min(2.0 ** -126))[1]              # c = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(c, dtype=torch.float64), e - 24)


def tail64(feat, w, b, amp_in, max_amp, ho, wo, fallback=False):
    """vfi_phasenet_level_tail -> {"phase", "amp", "next"} -> (float64 values, bound); next (N,72,ho,wo) = resize of
    [feat | pred].  fallback: the bound of the two-launch form (vfi_resize_bilinear's coordinate)."""
    head = head64(feat, w, b, amp_in, max_amp)
    pred, e_pred = head["pred"]
    f = feat.double()
    nxt = torch.cat((resize64(f, ho, wo), resize64(pred, ho, wo)), 1)
    e_next = torch.cat((resize64_bound(f, ho, wo, None, fallback), resize64_bound(pred, ho, wo, e_pred, fallback)), 1)
    return {"phase": head["phase"], "amp": head["amp"], "next": (nxt, e_next)}
