"""CPU checks of the pyramid synthesis' gradient (vfi_pyr_synthesize_backward): the float64 restatement of the synthesis
(tests/pyramid_grad_ref.py) against the oracle, its autograd against gradcheck, and the closed-form adjoint the kernels
implement against that autograd -- which pins the math, c_k = h_k w_k / (H W) included, independently of any kernel."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from oracle import layout_cpu, pyramid_cpu, synth

import pyramid_grad_ref as ref


def _case(h, w, n=2, seed=1):
    height = layout_cpu.calc_pyr_height(h, w)
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    return spec, synth.synthetic_vals(seed, n, h, w, height)


@pytest.mark.parametrize("h,w", [(24, 30), (33, 40), (64, 96)])
def test_float64_restatement_matches_oracle(h, w):
    spec, v = _case(h, w)
    coeff = layout_cpu.values_to_coeff(v)
    a = pyramid_cpu.reconstruct(spec, coeff).double()
    b = ref.reconstruct64(spec, coeff)
    assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())


def test_gradcheck_of_the_restatement():
    h, w = 10, 12
    spec = pyramid_cpu.PyramidSpec(h, w, 4)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64, requires_grad=True)
    hi, lo = r(1, h, w), r(1, *spec.sizes[-1])
    bands = [r(1, *spec.sizes[k], 2) for k in range(spec.nlev) for _ in range(4)]

    def f(hi, lo, *bands):
        coeff = [hi] + [list(bands[4 * k:4 * k + 4]) for k in range(spec.nlev)] + [lo]
        return ref.reconstruct64(spec, coeff)

    assert torch.autograd.gradcheck(f, (hi, lo, *bands))
    phase, amp = r(4, 1, *spec.sizes[0]), r(4, 1, *spec.sizes[0])
    rest = [(r(4, 1, *spec.sizes[k]).detach(), r(4, 1, *spec.sizes[k]).detach()) for k in range(1, spec.nlev)]

    def fp(phase, amp):
        ps, am = [phase] + [p for p, _ in rest], [amp] + [a for _, a in rest]
        return ref.reconstruct64(spec, ref.polar_to_coeff(hi.detach().unsqueeze(1), ps, am, lo.detach().unsqueeze(1)))

    assert torch.autograd.gradcheck(fp, (phase, amp))


@pytest.mark.parametrize("h,w", [(24, 30), (33, 40), (48, 64)])
def test_closed_form_adjoint_equals_autograd(h, w):
    spec, v = _case(h, w)
    d = lambda t: t.double().requires_grad_()
    high, low = d(v.high_level), d(v.low_level)
    phase, amp = [d(p) for p in v.phase], [d(a) for a in v.amplitude]
    out = ref.reconstruct64(spec, ref.polar_to_coeff(high, phase, amp, low))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (out * g).sum().backward()
    ghi, gbands, glo = ref.adjoint64(spec, g)
    assert float((high.grad.squeeze(1) - ghi).abs().max()) <= 1e-10
    assert float((low.grad.squeeze(1) - glo).abs().max()) <= 1e-10
    for k in range(spec.nlev):
        dphi, damp = ref.polar_grads(gbands[k], v.phase[k], v.amplitude[k])
        assert float((phase[k].grad - dphi).abs().max()) <= 1e-10, k
        assert float((amp[k].grad - damp).abs().max()) <= 1e-10, k
    # the complex surface (SCFpyr_PyTorch.reconstruct): gradients of the (re, im) coefficients
    coeff = [d(t) if torch.is_tensor(t) else [d(b) for b in t] for t in layout_cpu.values_to_coeff(v)]
    ref.reconstruct64(spec, coeff).mul(g).sum().backward()
    for k in range(spec.nlev):
        for b in range(4):
            assert float((coeff[1 + k][b].grad - torch.view_as_real(gbands[k][b])).abs().max()) <= 1e-10


def test_zero_amplitude_gives_finite_gradients_and_no_phase_gradient():
    spec, v = _case(24, 30)
    g = torch.randn(2, 24, 30, dtype=torch.float64)
    _, gbands, _ = ref.adjoint64(spec, g)
    amp = torch.zeros_like(v.amplitude[0])
    dphi, damp = ref.polar_grads(gbands[0], v.phase[0], amp)
    assert torch.isfinite(dphi).all() and torch.isfinite(damp).all()
    assert float(dphi.abs().max()) == 0.0 and float(damp.abs().max()) > 0.0


def test_backward_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "vfi_hip.h")).read()
    import vfi_amd
    from vfi_amd import _lib
    raw = ctypes.CDLL(vfi_amd.library_path())
    for name in ("vfi_pyr_plan_prepare_adjoint", "vfi_pyr_synthesize_backward"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    h = vfi_amd.lib()
    assert h.vfi_pyr_plan_prepare_adjoint(None) == -1          # argument checks need no GPU
    assert h.vfi_pyr_synthesize_backward(None, None, 1, None, None, None, 0, 0, None, None, None, None, None) == -1


def test_steerable_utils_imports():
    """The reference's `import steerable.utils` (src/train/pyramid.py:8, src/train/train.py:8) resolves."""
    import importlib
    m = importlib.import_module("vfi_amd.steerable.utils")
    assert m.__doc__
