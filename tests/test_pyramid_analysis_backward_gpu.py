"""GPU checks of the pyramid analysis' gradient: Pyramid.filter / SCFpyr_PyTorch.build / band_filter under autograd
(vfi_pyr_analyze_backward) against the float64 closed-form adjoint of tests/pyramid_ana_grad_ref.py, which
tests/test_pyramid_ana_grad_host.py pins against autograd of a float64 restatement of the oracle."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import layout_cpu, pyramid_cpu
from vfi_amd.steerable.SCFpyr_PyTorch import Analysis, SCFpyr_PyTorch
from vfi_amd.train import loss as vfi_loss
from vfi_amd.train.pyramid import Pyramid

import pyramid_ana_grad_ref as ref

pytestmark = pytest.mark.gpu
S2 = math.sqrt(2)
# the first three run the generic engine (smooth and Bluestein lengths), 256 x 256 is the smallest that reaches the wave engine
SIZES = [(64, 96), (65, 77), (90, 120), (256, 256)]
N = 3


@functools.lru_cache(maxsize=None)
def _spec(h, w):
    height = layout_cpu.calc_pyr_height(h, w)
    return height, pyramid_cpu.PyramidSpec(h, w, height)


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).random(tuple(shape), dtype=np.float32))


def _randn(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(shape)).astype(np.float32))


def _close(got, want, what, rel=1e-4):
    """|got - want| <= rel * max|want|: the criterion of the synthesis adjoint's tests."""
    want = want.double()
    err = float((got.detach().double().cpu() - want).abs().max())
    scale = float(want.abs().max())
    print(f"{what}: max|err| {err:.3e}, max|grad| {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= rel * scale, f"{what}: max|err| {err:.3e} vs max|grad| {scale:.3e}"


def _polar_reference(spec, n, dhigh, dphi, damp, phase, amp, dlow, s):
    """analysis_adjoint64 for per-image (N*nb,1,h,w) gradients; entries of dphi that are None drop their level."""
    G = [None if dphi[k] is None else
         ref.level_bands(ref.polar_to_coeff_grad(dphi[k], damp[k], phase[k].cpu(), amp[k].cpu(), s), n) for k in range(spec.nlev)]
    return ref.analysis_adjoint64(spec, None if dhigh is None else dhigh.squeeze(1), G, None if dlow is None else dlow.squeeze(1))


def test_filter_and_build_outputs_carry_a_grad_fn(device):
    h, w = 64, 96
    height, _ = _spec(h, w)
    img = _rand((1, h, w), 0).to(device).requires_grad_()
    v = Pyramid(height, 4, S2, device).filter(img)
    for t in [v.high_level, v.low_level, *v.phase, *v.amplitude]:
        assert t.grad_fn is not None
    (v.high_level.sum() + v.low_level.sum() + sum(p.sum() for p in v.phase) + sum(a.sum() for a in v.amplitude)).backward()
    assert img.grad is not None and img.grad.shape == img.shape and torch.isfinite(img.grad).all()
    assert v.phase[0].grad_fn.name().startswith(Analysis.__name__)
    img2 = _rand((1, 1, h, w), 1).to(device).requires_grad_()
    coeff = SCFpyr_PyTorch(height, 4, S2, device).build(img2)
    assert coeff[0].grad_fn is not None and coeff[-1].grad_fn is not None and all(b.grad_fn is not None for lv in coeff[1:-1] for b in lv)
    (coeff[0].sum() + coeff[-1].sum() + sum(b.sum() for lv in coeff[1:-1] for b in lv)).backward()
    assert img2.grad is not None and img2.grad.shape == img2.shape and torch.isfinite(img2.grad).all()


@pytest.mark.parametrize("s", [1.0, 1.0 / math.pi], ids=["s1", "s1overpi"])
@pytest.mark.parametrize("h,w", SIZES)
def test_polar_gradients_match_float64_adjoint(h, w, s, device):
    height, spec = _spec(h, w)
    img = _rand((N, h, w), 2).to(device).requires_grad_()
    v = Pyramid(height, 4, S2, device).filter(img, phase_scale=s)
    dhigh, dlow = _randn(v.high_level.shape, 3), _randn(v.low_level.shape, 4)
    dphi = [_randn(p.shape, 10 + k) for k, p in enumerate(v.phase)]
    damp = [_randn(a.shape, 40 + k) for k, a in enumerate(v.amplitude)]
    outs = [v.high_level, *v.phase, *v.amplitude, v.low_level]
    torch.autograd.backward(outs, [g.to(device) for g in [dhigh, *dphi, *damp, dlow]])
    # the GPU's own fp32 (phase, amplitude) go to the reference: the check is not conditioned by 1/A of values that differ
    want = _polar_reference(spec, N, dhigh, dphi, damp, [p.detach() for p in v.phase], [a.detach() for a in v.amplitude], dlow, s)
    _close(img.grad, want, f"{h}x{w} s={s:.4f} image gradient")


@pytest.mark.parametrize("h,w", SIZES)
def test_complex_gradients_match_float64_adjoint(h, w, device):
    height, spec = _spec(h, w)
    img = _rand((N, 1, h, w), 5).to(device).requires_grad_()
    coeff = SCFpyr_PyTorch(height, 4, S2, device).build(img)
    dhigh, dlow = _randn(coeff[0].shape, 6), _randn(coeff[-1].shape, 7)
    G = [[_randn(b.shape, 100 + 4 * k + i) for i, b in enumerate(lv)] for k, lv in enumerate(coeff[1:-1])]
    outs = [coeff[0]] + [b for lv in coeff[1:-1] for b in lv] + [coeff[-1]]
    torch.autograd.backward(outs, [g.to(device) for g in [dhigh] + [g for lv in G for g in lv] + [dlow]])
    want = ref.analysis_adjoint64(spec, dhigh, [[torch.view_as_complex(g.double()) for g in lv] for lv in G], dlow)
    _close(img.grad.squeeze(1), want, f"{h}x{w} image gradient (complex surface)")


def test_adjoint_identity_720p(device):
    """sum(Re z Re G + Im z Im G) + <high, d high> + <low, d low> = <x, grad x> (build is linear in the image)."""
    h, w = 720, 1280
    height, _ = _spec(h, w)
    img = _rand((1, 1, h, w), 8).to(device).requires_grad_()
    coeff = SCFpyr_PyTorch(height, 4, S2, device).build(img)
    outs = [coeff[0]] + [b for lv in coeff[1:-1] for b in lv] + [coeff[-1]]
    grads = [_randn(t.shape, 300 + i).to(device) for i, t in enumerate(outs)]
    torch.autograd.backward(outs, grads)
    lhs = sum(float((t.detach().double() * g.double()).sum()) for t, g in zip(outs, grads))
    rhs = float((img.detach().double() * img.grad.double()).sum())
    print(f"adjoint identity 720x1280: lhs {lhs:.9e} rhs {rhs:.9e} rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_zero_amplitudes_drop_the_phase_term(device):
    """ABI level: amplitudes set exactly to 0 give a finite result, equal to the reference without those d phase terms."""
    h, w, s = 65, 77, 1.0 / math.pi
    height, spec = _spec(h, w)
    pyr = Pyramid(height, 4, S2, device)
    img = _rand((N, h, w), 9).to(device)
    v = pyr.filter(img, phase_scale=s)
    rng = np.random.default_rng(11)
    zeros = 0
    for k in (0, 2, spec.nlev - 1):
        flat = v.amplitude[k].view(-1)
        idx = torch.from_numpy(rng.choice(flat.numel(), size=min(150, flat.numel() // 2), replace=False)).to(device)
        flat[idx] = 0.0
        zeros += idx.numel()
    assert zeros >= 200
    dhigh, dlow = _randn(v.high_level.shape, 12), _randn(v.low_level.shape, 13)
    dphi = [_randn(p.shape, 20 + k) for k, p in enumerate(v.phase)]
    damp = [_randn(a.shape, 60 + k) for k, a in enumerate(v.amplitude)]
    grad_img = torch.empty_like(img)
    dev = lambda ts: [t.to(device) for t in ts]
    pyr.pyr.plan(h, w, N).analyze_backward(dhigh.squeeze(1).to(device), dev(dphi), dev(damp), v.phase, v.amplitude, None,
                                           dlow.squeeze(1).to(device), s, (1 << spec.nlev) - 1, 0, grad_img)
    assert torch.isfinite(grad_img).all()
    _close(grad_img, _polar_reference(spec, N, dhigh, dphi, damp, v.phase, v.amplitude, dlow, s), "image gradient with zero amplitudes")


def test_dropped_levels_no_high_and_an_unused_output(device):
    """level_mask with two bits clear, want_high=False, and an output (low) the loss does not depend on."""
    h, w = 90, 120
    height, spec = _spec(h, w)
    dropped = {1, spec.nlev - 2}
    mask = sum(1 << k for k in range(spec.nlev) if k not in dropped)
    img = _rand((N, h, w), 14).to(device).requires_grad_()
    v = Pyramid(height, 4, S2, device).filter(img, level_mask=mask, want_high=False)
    assert not torch.is_tensor(v.high_level) and all(not torch.is_tensor(v.phase[k]) for k in dropped)
    kept = [k for k in range(spec.nlev) if k not in dropped]
    unused = kept[1]                                  # a level whose outputs get no gradient at all
    only_amp = kept[2]                                # a level whose phase gets none
    dphi = [None if k in dropped or k in (unused, only_amp) else _randn(v.phase[k].shape, 70 + k) for k in range(spec.nlev)]
    damp = [None if k in dropped or k == unused else _randn(v.amplitude[k].shape, 90 + k) for k in range(spec.nlev)]
    outs = [v.phase[k] for k in range(spec.nlev) if dphi[k] is not None] + [v.amplitude[k] for k in range(spec.nlev) if damp[k] is not None]
    grads = [g.to(device) for g in dphi if g is not None] + [g.to(device) for g in damp if g is not None]
    torch.autograd.backward(outs, grads)
    dphi[only_amp] = torch.zeros_like(damp[only_amp])
    phase = [v.phase[k].detach() if torch.is_tensor(v.phase[k]) else None for k in range(spec.nlev)]
    amp = [v.amplitude[k].detach() if torch.is_tensor(v.amplitude[k]) else None for k in range(spec.nlev)]
    _close(img.grad, _polar_reference(spec, N, None, dphi, damp, phase, amp, None, 1.0), "image gradient of a level subset")


def test_band_filters_are_self_adjoint(device):
    h, w = 90, 120
    height, spec = _spec(h, w)
    pyr = Pyramid(height, 4, S2, device)
    mask = 0b1011
    x = _rand((N, h, w), 15).to(device).requires_grad_()
    g = _randn((N, h, w), 16).to(device)
    y = pyr.band_filter(x, mask, keep_low=True)
    assert y.grad_fn is not None
    y.backward(g)
    with torch.no_grad():
        assert torch.equal(x.grad, pyr.band_filter(g, mask, keep_low=True))
        assert torch.equal(y.detach(), pyr.band_filter(x.detach(), mask, keep_low=True))
    lhs, rhs = float((y.detach().double() * g.double()).sum()), float((x.detach().double() * x.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    # the pair: each image set's gradient is its own filter applied to g
    spec_a, spec_b = dict(level_mask=0b0011, keep_low=True), dict(level_mask=0b1100, keep_high=True)
    a, b = _rand((N, h, w), 17).to(device).requires_grad_(), _rand((N, h, w), 18).to(device).requires_grad_()
    y = pyr.band_filter_pair(a, spec_a, b, spec_b)
    y.backward(g)
    with torch.no_grad():
        ga, gb = pyr.band_filter(g, **spec_a), pyr.band_filter(g, **spec_b)
        assert torch.equal(y.detach(), pyr.band_filter_pair(a.detach(), spec_a, b.detach(), spec_b))
    assert torch.equal(a.grad, ga) and torch.equal(b.grad, gb)      # (the same library call on the same filter id)
    lhs = float((y.detach().double() * g.double()).sum())
    rhs = float((a.detach().double() * a.grad.double()).sum() + (b.detach().double() * b.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    # only one of the two needs a gradient
    a2 = a.detach().clone().requires_grad_()
    pyr.band_filter_pair(a2, spec_a, b.detach(), spec_b).backward(g)
    assert torch.equal(a2.grad, ga)


def test_inference_output_unchanged_by_requires_grad(device):
    h, w = 90, 120
    height, _ = _spec(h, w)
    pyr = Pyramid(height, 4, S2, device)
    img = _rand((N, h, w), 19).to(device)
    flat = lambda v: [v.high_level, *v.phase, *v.amplitude, v.low_level]
    plain = flat(pyr.filter(img, phase_scale=1.0 / math.pi))
    tracked = flat(pyr.filter(img.clone().requires_grad_(), phase_scale=1.0 / math.pi))
    with torch.no_grad():
        untracked = flat(pyr.filter(img.clone().requires_grad_(), phase_scale=1.0 / math.pi))
    for p, t, u in zip(plain, tracked, untracked):
        assert t.grad_fn is not None and u.grad_fn is None and p.grad_fn is None
        assert torch.equal(p, t.detach()) and torch.equal(p, u)
    scf = SCFpyr_PyTorch(height, 4, S2, device)
    cflat = lambda c: [c[0]] + [b for lv in c[1:-1] for b in lv] + [c[-1]]
    for p, t in zip(cflat(scf.build(img.unsqueeze(1))), cflat(scf.build(img.unsqueeze(1).clone().requires_grad_()))):
        assert t.grad_fn is not None and p.grad_fn is None and torch.equal(p, t.detach())
    # the PhaseNet layout stays outside autograd
    v, bufs, amp_max = pyr.filter(img.clone().requires_grad_(), concat_frames=1, phase_scale=1.0 / math.pi, amp_max_eps=1e-8)
    assert all(not t.requires_grad for t in [v.high_level, v.low_level, amp_max, *v.phase, *v.amplitude, *bufs])


@pytest.mark.parametrize("h,w", [(90, 120), (256, 256)])
def test_backward_is_deterministic(h, w, device):
    height, _ = _spec(h, w)
    pyr = Pyramid(height, 4, S2, device)
    img = _rand((N, h, w), 20).to(device)
    res = []
    for _ in range(2):
        x = img.clone().requires_grad_()
        v = pyr.filter(x)
        outs = [v.high_level, *v.phase, *v.amplitude, v.low_level]
        torch.autograd.backward(outs, [_randn(t.shape, 400 + i).to(device) for i, t in enumerate(outs)])
        res.append(x.grad)
    assert torch.equal(res[0], res[1])


def _fit_losses(pyr, device, steps):
    """An image fitted to a target in the pyramid domain: the loss is get_loss's form (src/train/loss.py:5-25) on the
    pyramid values themselves, per level the phase term plus the L1 of the amplitudes."""
    h, w = 90, 120
    target = _rand((1, h, w), 21).to(device)
    with torch.no_grad():
        vt = pyr.filter(target)
    x = _rand((1, h, w), 22).to(device).requires_grad_()
    opt = torch.optim.Adam([x], lr=0.02)
    losses = []
    for _ in range(steps):
        v = pyr.filter(x)
        loss = 0
        for k in range(len(v.phase)):
            loss = loss + vfi_loss.phase_term(v.phase[k], vt.phase[k], pyr.nbands) + vfi_loss.l1_loss(v.amplitude[k], vt.amplitude[k])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_fitting_an_image_through_filter(device):
    height, _ = _spec(90, 120)
    pyr = Pyramid(height, 4, S2, device)
    a = _fit_losses(pyr, device, 30)
    b = _fit_losses(pyr, device, 30)
    print("losses:", a[0], a[-1])
    assert a[-1] < a[0], a
    assert a == b
