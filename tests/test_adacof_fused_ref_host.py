"""The float64 statement of the fused AdaCoF operator (tests/adacof_fused_ref.py) against the two fp32 statements the project
already trusts: the fixtures the reference's own kernel text produced, and oracle/adacof_cpu.c.  CPU only."""
import glob
import os

import numpy as np
import pytest

import adacof_fused_ref as R
from conftest import GOLDEN
from oracle import adacof_cpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "adacof_sampling_*.npz")))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[16:-4] for p in FIXTURES])
def test_one_sided_sampler_reproduces_reference_fixture(path):
    # the fixtures sample an already-padded input (FunctionAdaCoF.forward), with exact-integer, negative, -0.0 and +-1000
    # offsets (tests/golden/make_golden.py: adacof_inputs).  Largest fp32-fixture-vs-float64 difference seen: 4.0e-7 (f5d1
    # 2.5e-7, f5d1_b2 2.3e-7, f11d2 4.0e-7, f3d1_c1 1.4e-7) -- a wrong corner or fraction would show as 1e-2 or more.
    g = np.load(path)
    out = R.sample_side(g["input"], g["weight"], g["offset_i"], g["offset_j"], int(g["dilation"]), padded=True)
    err = float(np.abs(out - g["output"]).max())
    print(f"{os.path.basename(path)}: fp32 fixture vs float64 {err:.2e}")
    assert out.shape == g["output"].shape and err <= R.IMAGE_ATOL


def test_fixture_set_is_present():
    assert len(FIXTURES) >= 4


def _oracle(case):
    d = R.inputs(case)
    pad = (case.f - 1) * case.dil // 2
    edge = lambda x: np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), mode="edge")
    o1 = adacof_cpu.adacof_forward(edge(d["f0"]), d["w1"], d["a1"], d["b1"], case.dil)
    o2 = adacof_cpu.adacof_forward(edge(d["f2"]), d["w2"], d["a2"], d["b2"], case.dil)
    frame, mask = adacof_cpu.blend_mask(o1, o2, d["occ"], d["w1"], d["a1"], d["b1"], d["w2"], d["a2"], d["b2"])
    return o1, o2, frame, mask


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_float64_reference_brackets_the_fp32_oracle(case):
    # What fp32 evaluation costs on its own -- the largest fp32-oracle-vs-float64 differences over the case table (the
    # oracle evaluates left to right without contraction; the mask error is that of mask = Var / 20):
    #                                          t1, t2, frame   mask (absolute)   mask (relative, where mask >= 1e-3)
    #   softmax / dominant weights, gaussian     3.7e-7          3.1e-7            3.3e-7
    #   boundary / edge fields                   4.0e-7          2.0e-7            2.1e-7
    #   far field                                4.2e-7          1.3e-8            4.0e-7
    #   rand weights (sum ~F*F/2, images ~S/2)   4.8e-6          6.0e-7            8.9e-7
    # tests/test_adacof_fused_gpu.py holds the kernels to the same bounds; one of them may be raised to at most twice the
    # figure of its row here, never further.
    ref = R.reference(case)
    img, excess, merr, finite = R.errors(case, _oracle(case), ref)
    big = ref["mask"] >= 1e-3
    rel = float((np.abs(_oracle(case)[3] - ref["mask"])[big] / ref["mask"][big]).max()) if big.any() else 0.0
    print(f"{R.case_id(case)}: fp32 oracle vs float64: images {img:.2e} mask {merr:.2e} (relative {rel:.2e}, excess {excess:.2e})")
    assert R.passes(img, excess, finite), (img, excess, merr)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.field in ("gauss1", "gauss02", "gauss01") and c.weights != "dominant"],
                         ids=R.case_id)
def test_small_offset_cases_leave_the_mask_unsaturated(case):
    # otherwise the mask comparison of these cases would check only the clamp
    m = R.reference(case)["mask"]
    inside = float(((m > 0.0) & (m < 1.0)).mean())
    assert inside >= 0.5, inside


def test_logits_reference_agrees_with_the_weights_reference():
    # lg = log W + shift: the float64 softmax of the fp32 logits is W up to the rounding of lg (|lg| <= ~200: 8e-6)
    case = R.CASES[1]
    a, b = R.reference(case), R.reference(case, logits=True)
    for k in a:
        assert np.abs(a[k] - b[k]).max() <= 1e-4
    assert np.abs(R.inputs(case)["lg1"]).max() > 20.0


def test_case_table_reaches_every_instantiation_twice():
    # the arithmetic of adacof_fused_ref's docstring, applied to the table: every (WIN?, FT) group of the rgbx kernels gets
    # (9,70), a second shape and the boundary field; every planar VEC gets two widths per FT
    groups = {}
    for c in R.CASES:
        e = (c.f - 1) * c.dil
        assert e % 2 == 0
        groups.setdefault(((13 + e) * (73 + e) <= 2048, c.f == 5), []).append(c)
    assert len(groups) == 4
    for cs in groups.values():
        assert (9, 70) in {(c.h, c.w) for c in cs} and len({(c.n, c.h, c.w) for c in cs}) >= 2
        assert any(c.field == "boundary" for c in cs) and any(c.weights == "rand" for c in cs)
    for ft5 in (True, False):
        widths = {c.w for c in R.CASES if (c.f == 5) == ft5}
        assert len([w for w in widths if w % 4 == 0]) >= 2              # VEC=4 (VFI_ADACOF_VARIANT=0)
        assert len([w for w in widths if w % 2 == 0]) >= 2              # VEC=2 (VFI_ADACOF_VARIANT=1; 0: W % 4 == 2)
        assert len([w for w in widths if w % 2 == 1]) >= 2              # VEC=1 under either switch
    assert {(c.f, c.dil) for c in R.CASES} == {(5, 1), (5, 2), (3, 2), (7, 1), (5, 3), (7, 2), (11, 2)}
