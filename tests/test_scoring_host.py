"""The scoring references (tests/scoring_ref.py) against each other, and the proof that tests/test_scoring_gpu.py can fail:
for every SSIM and vfi_ssim_sum case, float32 and float64 evaluations of the reference agree to half the case's bound, and
every planted mistake that fits the case moves the float64 value by at least ten bounds.  No GPU."""
import math

import pytest
import torch

import scoring_ref as sr


@pytest.mark.parametrize("dim", [96, 512])
def test_ssim_ref_float32_is_the_formula_of_the_first_scoring_test(dim):
    from test_scoring_gpu import _ssim_ref
    g = torch.Generator().manual_seed(dim)
    pred = torch.rand((3, dim + 8, dim + 8), generator=g)
    tgt = (pred + 0.05 * torch.randn((3, dim + 8, dim + 8), generator=g)).clamp(0, 1)
    c = lambda t: t[:, 4:4 + dim, 4:4 + dim]
    assert sr.ssim_ref(c(pred), c(tgt), torch.float32)[0] == _ssim_ref(c(pred), c(tgt))


@pytest.mark.parametrize("i", range(len(sr.SSIM_CASES)), ids=[sr.case_id(c) for c in sr.SSIM_CASES])
def test_ssim_cases_have_margin_and_teeth(i):
    shape, downsample, _ = sr.SSIM_CASES[i]
    case = sr.ssim_case(i)
    bound, planted = case["bound"], case["planted"]
    gap = abs(case["ref32"] - case["ref64"])
    shifts = {k: abs(v - case["ref64"]) for k, v in planted.items() if k != "true"}
    print(f"{sr.case_id(sr.SSIM_CASES[i])}: f {case['f']} ssim {case['ref64']:.6f} bound {bound:.3e} |ref32 - ref64| {gap:.3e} "
          + " ".join(f"{k} {v:.3e}" for k, v in shifts.items()))
    # the full-size maps the planted windows are cut from hold the reference's own value in the true window
    assert abs(planted["true"] - case["ref64"]) <= 1e-12
    assert gap <= 0.5 * bound
    expect = {"border-1", "row+1", "col+1"}
    ph, pw = shape[1] // case["f"], shape[2] // case["f"]
    if min(ph, pw) > 12:
        expect.add("border+1")
    if ph != pw:
        expect.add("transposed")
    if case["f"] > 1:
        expect.add("pool f-1")
    if min(shape[1:]) // (case["f"] + 1) >= sr.KS:
        expect.add("pool f+1")
    assert set(shifts) == expect
    for k, v in shifts.items():
        assert v >= 10.0 * bound, (k, v, bound)


@pytest.mark.parametrize("j", range(len(sr.C_PAIRS)))
@pytest.mark.parametrize("i", range(len(sr.SUM_CASES)), ids=[sr.case_id(c) for c in sr.SUM_CASES])
def test_ssim_sum_cases_have_margin_and_teeth(i, j):
    shape, border, _ = sr.SUM_CASES[i]
    case = sr.sum_case(i, j)
    bound = case["bound"]
    gap = abs(case["ref32"] - case["ref64"])
    shifts = {k: abs(v - case["planted"]["true"]) for k, v in case["planted"].items() if k != "true"}
    print(f"{sr.case_id(sr.SUM_CASES[i])} c {j}: sum {case['ref64']:.6f} of {case['n_valid']} bound {bound:.3e} "
          f"|ref32 - ref64| {gap:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in shifts.items()))
    assert case["n_valid"] == shape[0] * (shape[1] - 2 * border) * (shape[2] - 2 * border)
    assert abs(case["planted"]["true"] - case["ref64"]) <= 1e-12 * case["n_valid"]
    assert gap <= 0.5 * bound
    expect = set() if border == 0 else {"border-1", "row+1", "col+1"}
    if min(shape[1:]) > 2 * (border + 1):
        expect.add("border+1")
    if shape[1] != shape[2] and border > 0:
        expect.add("transposed")
    assert set(shifts) == expect and shifts
    for k, v in shifts.items():
        assert v >= 10.0 * bound, (k, v, bound)


def test_structured_pair_varies_across_the_frame():
    x, y = sr.structured_pair((1, 384, 385), 6)
    assert x.dtype == y.dtype == torch.float32 and 0.0 <= float(min(x.min(), y.min())) and float(max(x.max(), y.max())) <= 1.0
    m = sr.ssim_ref(x, y, torch.float64, downsample=False)[1][0]
    h, w = m.shape
    quads = [float(q.mean()) for q in (m[:h // 2, :w // 2], m[:h // 2, w // 2:], m[h // 2:, :w // 2], m[h // 2:, w // 2:])]
    print("quadrant SSIM", quads)
    assert quads[0] > quads[2] > quads[3] and quads[0] > quads[1] > quads[3]       # falls along x and along y
    assert quads[0] - quads[3] > 0.3 and abs(quads[1] - quads[2]) > 0.05              # and not symmetrically


def test_pool_factor_rounding():
    assert [sr.pool_factor(n, 2000) for n in (383, 384, 640, 641, 896, 1080)] == [1, 2, 2, 3, 4, 4]
    assert sr.pool_factor(2000, 641) == 3


def test_crop_center_negative_starts():
    from vfi_amd.fusion_net.interpolate_twoframe import crop_center
    assert tuple(crop_center(torch.zeros(100, 90, 3), 128, 128).shape[:2]) == (14, 19)
    assert tuple(crop_center(torch.zeros(256, 448, 3), 512, 512).shape[:2]) == (128, 32)
    img = torch.arange(100 * 90, dtype=torch.float32).reshape(100, 90, 1)
    assert torch.equal(crop_center(img, 128, 128), img[86:, 71:])


def test_diff_sums_ref_is_exact_on_integers():
    i = torch.arange(1000)
    d = 1 + (i * 5) % 8
    b = ((i * 3) % 16).float()
    (s1, s2), (b1, b2) = sr.diff_sums_ref(b + d.float(), b)
    assert s1 == int(d.sum()) and s2 == int((d * d).sum())
    assert math.isclose(b1, 1002 * 2.0 ** -53 * s1) and math.isclose(b2, 1002 * 2.0 ** -53 * s2)
