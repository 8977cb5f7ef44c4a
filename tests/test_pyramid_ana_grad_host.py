"""CPU checks of the pyramid analysis' gradient (vfi_pyr_analyze_backward): the float64 restatement of the analysis
(tests/pyramid_ana_grad_ref.py) against the oracle, and the closed-form adjoint the kernels implement (polar prologue
included) against float64 autograd of that restatement -- which pins the math, the constants 1 / (h_k w_k) included,
independently of any kernel."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from oracle import layout_cpu, pyramid_cpu

import pyramid_ana_grad_ref as ref

SIZES = [(64, 96), (65, 77), (90, 120)]


def _case(h, w, n=2, seed=1):
    spec = pyramid_cpu.PyramidSpec(h, w, layout_cpu.calc_pyr_height(h, w))
    return spec, torch.rand((n, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _randn(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("h,w", SIZES)
def test_float64_restatement_matches_oracle(h, w):
    spec, x = _case(h, w)
    want = pyramid_cpu.build(spec, x.float())
    high, bands, low = ref.build64(spec, x.float())
    assert float((want[0].double() - high).abs().max()) <= 2e-6 * float(high.abs().max())
    assert float((want[-1].double() - low).abs().max()) <= 2e-6 * float(low.abs().max())
    for k in range(spec.nlev):
        got = torch.stack([torch.view_as_real(z) for z in bands[k]])
        assert float((torch.stack(want[1 + k]).double() - got).abs().max()) <= 2e-6 * float(got.abs().max()), k


@pytest.mark.parametrize("s", [1.0, 1.0 / math.pi])
@pytest.mark.parametrize("h,w", SIZES)
def test_closed_form_adjoint_equals_autograd(h, w, s):
    spec, x = _case(h, w)
    n = x.shape[0]
    x.requires_grad_()
    high, phase, amp, low = ref.analyze64(spec, x, s)
    assert all(float(a.detach().min()) > 0.0 for a in amp)            # (random images: no coefficient at the origin)
    dhigh, dlow = _randn(high.shape, 2), _randn(low.shape, 3)
    dphi = [_randn(p.shape, 10 + k) for k, p in enumerate(phase)]
    damp = [_randn(a.shape, 40 + k) for k, a in enumerate(amp)]
    loss = (high * dhigh).sum() + (low * dlow).sum()
    for k in range(spec.nlev):
        loss = loss + (phase[k] * dphi[k]).sum() + (amp[k] * damp[k]).sum()
    loss.backward()
    G = [ref.level_bands(ref.polar_to_coeff_grad(dphi[k], damp[k], phase[k].detach(), amp[k].detach(), s), n)
         for k in range(spec.nlev)]
    got = ref.analysis_adjoint64(spec, dhigh.squeeze(1), G, dlow.squeeze(1))
    err = float((got - x.grad).abs().max())
    print(f"{h}x{w} s={s:.4f}: max|closed form - autograd| {err:.3e}, max|grad| {float(x.grad.abs().max()):.3e}")
    assert err <= 1e-10
    # the complex surface (SCFpyr_PyTorch.build): upstream gradients of the (re, im) coefficients, some outputs unused
    x.grad = None
    high, bands, low = ref.build64(spec, x)
    Gc = [[torch.complex(_randn(z.shape, 100 + 4 * k + b), _randn(z.shape, 200 + 4 * k + b)) for b, z in enumerate(lv)]
          for k, lv in enumerate(bands)]
    Gc[1] = None
    loss = (low * dlow.squeeze(1)).sum()
    for k in range(spec.nlev):
        if Gc[k] is not None:
            loss = loss + sum((z.real * g.real).sum() + (z.imag * g.imag).sum() for z, g in zip(bands[k], Gc[k]))
    loss.backward()
    got = ref.analysis_adjoint64(spec, None, Gc, dlow.squeeze(1))
    assert float((got - x.grad).abs().max()) <= 1e-10


def test_zero_amplitude_drops_the_phase_term():
    dphi, damp = _randn((4, 1, 5, 6), 1), _randn((4, 1, 5, 6), 2)
    phi, amp = _randn((4, 1, 5, 6), 3), _randn((4, 1, 5, 6), 4).abs()
    amp[:, :, ::2] = 0.0
    G = ref.polar_to_coeff_grad(dphi, damp, phi, amp, 1.0 / math.pi)
    assert torch.isfinite(torch.view_as_real(G)).all()
    want = damp * torch.exp(1j * phi * math.pi)
    assert float((G - want)[:, :, ::2].abs().max()) <= 1e-15


def test_backward_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "vfi_hip.h")).read()
    import vfi_amd
    from vfi_amd import _lib
    raw = ctypes.CDLL(vfi_amd.library_path())
    for name in ("vfi_pyr_plan_prepare_analysis_adjoint", "vfi_pyr_analyze_backward"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    h = vfi_amd.lib()
    assert h.vfi_pyr_plan_prepare_analysis_adjoint(None) == -1          # argument checks need no GPU
    one = ctypes.c_void_p(16)
    # (plan, grad_high, grad_phase, grad_amp, phase, amp, plane_index, grad_low, phase_scale, level_mask, flags, grad_img, N, stream)
    assert h.vfi_pyr_analyze_backward(None, None, None, None, None, None, None, None, 1.0, 0, 0, one, 1, None) == -1
    assert h.vfi_pyr_analyze_backward(one, None, None, None, None, None, None, None, 1.0, 0, 0, None, 1, None) == -1
