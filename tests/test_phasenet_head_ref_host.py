"""CPU checks of tests/phasenet_head_ref.py (the float64 restatement of PhaseNet's level head and its bounds) and of the path
query vfi_phasenet_level_tail_path, which makes no GPU call."""
import math

import pytest
import torch
import torch.nn.functional as F

import phasenet_head_ref as H


@pytest.mark.parametrize("n_in,n_out", [(64, 64), (4, 5), (1024, 1449), (46, 65), (66, 132), (32, 256), (86, 258), (70, 64), (65, 92), (1, 3)])
def test_taps_are_one_rounding_of_the_exact_coordinate(n_in, n_out):
    """`taps`' coordinate is fmaf's: the float32 nearest to scale (o + 0.5) - 0.5 evaluated exactly (in rationals)."""
    from fractions import Fraction
    scale = float(torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32))
    i0, i1, frac, f, g = H.taps(n_in, n_out)
    for o in range(n_out):
        exact = Fraction(scale) * Fraction(2 * o + 1, 2) - Fraction(1, 2)
        c = float(f[o])
        if exact <= 0:
            assert c == 0.0
            continue
        ulp = float(H._ulp32(f[o:o + 1]))
        assert abs(Fraction(c) - exact) <= Fraction(ulp) / 2, (o, c, float(exact))
        assert int(i0[o]) == min(int(c), n_in - 1) and int(i1[o]) == min(int(i0[o]) + 1, n_in - 1)
        assert float(frac[o]) == c - int(i0[o])


def test_resize64_is_torch_bilinear_up_to_the_float32_coordinate():
    """Exact scales (x1, x2: the float32 coordinate is the exact one) give torch's float64 result to float64 rounding; elsewhere
    the two differ by the coordinate's float32 rounding, within a few units of the fallback bound's coordinate term."""
    src = torch.randn((2, 3, 17, 23), generator=torch.Generator().manual_seed(1))
    for ho, wo in ((17, 23), (34, 46), (17, 46)):
        ref = F.interpolate(src.double(), size=(ho, wo), mode="bilinear", align_corners=False)
        assert float((H.resize64(src, ho, wo) - ref).abs().max()) <= 1e-14
    ref = F.interpolate(src.double(), size=(24, 33), mode="bilinear", align_corners=False)
    assert float((H.resize64(src, 24, 33) - ref).abs().max()) <= 1e-5


@pytest.mark.parametrize("num_img", [2, 3])
def test_a_float32_evaluation_lies_within_the_bounds(num_img):
    """torch's float32 evaluation of the same formulas on the CPU (another summation order, another tanhf) stays inside every
    bound, with room: the bounds are worst-case ones."""
    g = torch.Generator().manual_seed(num_img)
    p = 12 if num_img == 3 else 8
    n, h, w, ho, wo = 2, 9, 13, 13, 19
    f, wt, b = torch.randn((n, 64, h, w), generator=g), torch.randn((p, 64), generator=g) / 8, torch.randn((p,), generator=g) * 0.1
    a, mx = torch.rand((n, 4 * num_img, h, w), generator=g), torch.rand((n,), generator=g) + 0.5
    ref = H.head64(f, wt, b, a, mx, num_img)
    pred = torch.tanh(torch.einsum("jk,nkhw->njhw", wt, f) + b.view(1, -1, 1, 1))
    beta = (pred[:, 4:8] + 1) / 2
    amp = beta * a[:, 4:8] + (1 - beta) * a[:, :4]
    if num_img == 3:
        fb = (pred[:, 8:12] + 1) / 2
        amp = fb * amp + (1 - fb) * a[:, 8:12]
    got = {"pred": pred, "phase": pred[:, :4] * torch.tensor(math.pi, dtype=torch.float32), "amp": amp * mx.view(-1, 1, 1, 1)}
    for k, v in got.items():
        r, bound = ref[k]
        assert bool(((v.double() - r).abs() <= 0.5 * bound).all()), k
    if num_img == 2:
        for fallback in (False, True):
            nxt, e = H.tail64(f, wt, b, a, mx, ho, wo, fallback)["next"]
            assert nxt.shape == (n, 72, ho, wo) and bool((e > 0).all())
            assert bool((e[:, 64:] >= H.TANH_ALLOWANCE).all())                 # the prediction planes carry the prediction's bound


def test_a_wrong_weight_or_tap_leaves_the_bounds():
    """What the bounds are for: one of 64 weights off by 2^-12 relative, or a resize tap one column off, is outside them."""
    g = torch.Generator().manual_seed(5)
    n, h, w, ho, wo = 1, 16, 20, 23, 29
    f, wt, b = torch.randn((n, 64, h, w), generator=g), torch.randn((8, 64), generator=g) / 8, torch.randn((8,), generator=g) * 0.1
    a, mx = torch.rand((n, 8, h, w), generator=g), torch.rand((n,), generator=g) + 0.5
    ref = H.tail64(f, wt, b, a, mx, ho, wo)
    w2 = wt.clone()
    w2[:, 5] *= 1 + 2.0 ** -12
    bad = H.head64(f, w2, b, a, mx)
    for k in ("phase", "amp"):
        assert bool(((bad[k][0] - ref[k][0]).abs() > ref[k][1]).any()), k
    nxt, e = ref["next"]
    shifted = torch.cat((nxt[..., 1:], nxt[..., -1:]), -1)
    assert bool(((shifted - nxt).abs() > e).any())


def test_level_tail_path_query_validates_like_the_entry_point():
    """No GPU call: the rule on sizes and alignment, and null pointers and shapes the entry point refuses come back as its
    status, not as a path."""
    from vfi_amd import _lib
    q = _lib.lib().vfi_phasenet_level_tail_path
    p, s80, s88 = 4096, 80 * 4096, 88 * 4096
    assert q(p, s80, p, None, p, s88, p, p, s88, p, p, 1, 64, 64, 64, 64) == 2
    assert q(p, s80, p, None, p, s88, p, p + 4, s88, p, p, 1, 64, 64, 64, 64) == 1            # x_next 4 bytes past
    assert q(p, s80, p, None, p, s88, p, p, s88 + 1, p, p, 2, 64, 64, 64, 64) == 1            # its batch stride odd
    assert q(p, s80, p, None, p, s88, p, p, s88, p, p, 1, 64, 64, 64, 65) == 1                # odd target width
    assert q(p + 8, s80, p, None, p + 8, s88, p, p, s88, p, p, 1, 64, 64, 64, 64) == 2        # inputs 8 bytes past
    assert q(p + 4, s80, p, None, p, s88, p, p, s88, p, p, 1, 64, 64, 64, 64) == 0            # features 4 bytes past
    assert q(p, s80, p, None, p, s88, p, p, s88, p + 4, p, 1, 64, 64, 64, 64) == 0            # phase_out 4 bytes past
    assert q(p, 80 * 4095, p, None, p, 88 * 4095, p, p, s88, p, p, 1, 63, 65, 64, 65) == 0    # fewer than 4096 pixels
    assert q(p, 80 * 4225, p, None, p, 88 * 4225, p, p, s88, p, p, 1, 65, 65, 65, 65) == 0    # an odd plane
    assert q(p, s80, p, None, p, s88, p, p, s88, p, p, 1, 64, 64, 63, 128) == 0               # fewer rows than the source
    assert q(None, s80, p, None, p, s88, p, p, s88, p, p, 1, 64, 64, 64, 64) == -1
    assert q(p, s80, p, None, p, s88, p, p, 88, p, p, 1, 64, 64, 1, 1) < 0                    # target too small to carry pred
