"""Every instantiation of `adacof_fused_kernel` (csrc/vfi_adacof.hip) against the float64 statement of the operator
(tests/adacof_fused_ref.py), at the smallest shapes and the offset fields at which each can go wrong.

adacof_fused_ref's docstring derives which (F, dilation) reaches which instantiation; nothing here asserts which kernel ran
(the library has no entry point to ask).  The default environment reaches the planar VEC=1 kernels and all eight rgbx ones;
the planar VEC=2 / VEC=4 kernels and the non-WIN rgbx kernels at every F sit behind VFI_ADACOF_VARIANT / VFI_ADACOF_MARGIN,
which the library reads once per process: test_variants_behind_the_environment_switches runs the same table in a child.

Bounds (adacof_fused_ref: IMAGE_ATOL, MASK_RTOL, MASK_ATOL, MASK_RTOL_FAR) are those of tests/test_adacof_gpu.py.  What fp32
evaluation alone costs against float64 on these very cases is recorded in tests/test_adacof_fused_ref_host.py
(images <= 4.2e-7, 4.8e-6 with weights that sum to ~F*F/2; mask <= 6e-7).  The kernels contract to fma, precompute the
bilinear weights and form the variance in one pass from pivoted moments; measured on an MI355X over the whole table they are
within 6.6e-7 on the images (4.9e-6 with the large weights) and 3.1e-6 on the mask (7.9e-6 with the large weights), so no
bound is raised.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

import adacof_fused_ref as R
from vfi_amd import _lib
from vfi_amd._lib import VfiLibraryError
from vfi_amd.adacof.cupy_module.adacof import adacof_fused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fused_matches_float64(case, device):
    # planar, rgbx and (unless the weights do not sum to 1) rgbx + logits: t1, t2, frame and mask of each
    seen = []
    for mode, img, excess, merr, finite in R.run_case(case, device):
        print(f"{R.case_id(case)} {mode}: images {img:.2e} mask {merr:.2e} (excess {excess:.2e})")
        seen.append(mode)
        assert finite, mode                                  # the rgbx frames carry NaN in their fourth lane
        assert img <= R.IMAGE_ATOL, (mode, img)
        assert excess <= 0.0, (mode, merr, excess)
    assert tuple(seen) == R.modes_of(case)


PRODUCTION = [c for c in R.CASES if (c.f, c.dil) == (5, 1) and (c.h, c.w) in ((9, 70), (10, 129))
              and c.field in ("gauss3", "boundary", "edge") and c.weights == "softmax"]
assert len(PRODUCTION) == 6


@pytest.mark.parametrize("case", PRODUCTION, ids=R.case_id)
def test_production_variant_properties(case, device):
    # rgbx + logits, F=5, dilation 1: the kernel the pipeline launches
    d = R.device_inputs(case, device)
    first = R.launch(case, d, "rgbx_logits")
    # determinism
    again = R.launch(case, d, "rgbx_logits")
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # the optional outputs may be omitted: same frame bits
    t1, t2, frame, mask = R.launch(case, d, "rgbx_logits", want_sides=False, want_mask=False)
    assert t1 is None and t2 is None and mask is None and torch.equal(frame, first[2])
    # a tap that read an LDS word the workgroup had not staged would now return NaN
    _lib.call("vfi_debug_poison_lds", _lib.stream_ptr())
    after = R.launch(case, d, "rgbx_logits")
    torch.cuda.synchronize()
    for a, b in zip(first, after):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def _args(device, f=5, h=8, w=16):
    z = lambda *s: torch.zeros(s, device=device)
    k = f * f
    return dict(f0=z(1, 3, h, w), f2=z(1, 3, h, w), w=z(1, k, h, w), occ=z(1, 1, h, w))


def test_misaligned_rgbx_frame_is_rejected(device):
    a = _args(device)
    buf = torch.zeros(8 * 16 * 4 + 4, device=device)
    off = buf[1:1 + 8 * 16 * 4].view(1, 8, 16, 4)             # a float4 buffer sliced one float in: contiguous, 4-byte aligned
    ok = buf[:8 * 16 * 4].view(1, 8, 16, 4)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    adacof_fused(ok, ok, a["w"], a["w"], a["w"], a["w"], a["w"], a["w"], a["occ"], 1, rgbx=True)
    with pytest.raises(VfiLibraryError, match="VFI_ERR_INVALID_ARG"):
        adacof_fused(off, ok, a["w"], a["w"], a["w"], a["w"], a["w"], a["w"], a["occ"], 1, rgbx=True)
    with pytest.raises(VfiLibraryError, match="VFI_ERR_INVALID_ARG"):
        adacof_fused(ok, off, a["w"], a["w"], a["w"], a["w"], a["w"], a["w"], a["occ"], 1, rgbx=True)


def test_odd_tap_reach_is_rejected(device):
    a = _args(device, f=4)                                      # (F-1)*dilation = 3: the replication pad would be 1.5
    with pytest.raises(VfiLibraryError, match="VFI_ERR_SHAPE"):
        adacof_fused(a["f0"], a["f2"], a["w"], a["w"], a["w"], a["w"], a["w"], a["w"], a["occ"], 1)
    x = torch.zeros((1, 8, 16, 4), device=device)
    with pytest.raises(VfiLibraryError, match="VFI_ERR_SHAPE"):
        adacof_fused(x, x, a["w"], a["w"], a["w"], a["w"], a["w"], a["w"], a["occ"], 1, rgbx=True)


def test_logits_need_rgbx_frames(device):
    a = _args(device)
    with pytest.raises(VfiLibraryError):
        adacof_fused(a["f0"], a["f2"], a["w"], a["w"], a["w"], a["w"], a["w"], a["w"], a["occ"], 1, weights_are_logits=True)


@pytest.mark.parametrize("c", [1, 4])
def test_other_channel_counts_are_unsupported(c, device):
    a = _args(device)
    fr, out = torch.zeros((1, c, 8, 16), device=device), torch.zeros((1, c, 8, 16), device=device)
    p = _lib.dptr
    with pytest.raises(VfiLibraryError, match="VFI_ERR_UNSUPPORTED"):
        _lib.call("vfi_adacof_fused", p(fr), p(fr), p(a["w"]), p(a["w"]), p(a["w"]), p(a["w"]), p(a["w"]), p(a["w"]),
                  p(a["occ"]), None, None, p(out), None, 1, c, 8, 16, 5, 1, _lib.stream_ptr())


@pytest.mark.parametrize("switch", ["VFI_ADACOF_VARIANT=0", "VFI_ADACOF_VARIANT=1", "VFI_ADACOF_MARGIN=0"])
def test_variants_behind_the_environment_switches(switch, device):
    # VARIANT=0: planar VEC=4 (W % 4 == 0) / VEC=2 (W % 4 == 2) / VEC=1 (odd W); VARIANT=1: VEC=2 for every even W;
    # MARGIN=0: the non-WIN rgbx kernels at every F.  The whole table once, in a fresh process (tools/check_adacof_fused.py);
    # a few seconds of work after the start-up of torch and the HIP runtime.
    name, value = switch.split("=")
    env = dict(os.environ, **{name: value})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_adacof_fused.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert not re.search(r"^FAIL", r.stdout, flags=re.M), r.stdout[-3000:]
    assert len(re.findall(r"^ok ", r.stdout, flags=re.M)) == sum(len(R.modes_of(c)) for c in R.CASES), r.stdout[-3000:]
    m = re.search(r"worst abs error ([0-9.e+-]+)", r.stdout)
    assert m and float(m.group(1)) <= R.IMAGE_ATOL, r.stdout[-3000:]
