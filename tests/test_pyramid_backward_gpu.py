"""GPU checks of the pyramid synthesis' gradient: Pyramid.inv_filter / SCFpyr_PyTorch.reconstruct under autograd
(vfi_pyr_synthesize_backward) against the float64 closed-form adjoint of tests/pyramid_grad_ref.py, which
tests/test_pyramid_grad_host.py pins against autograd of a float64 restatement of the oracle."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_DIR, ROOT
from oracle import color_cpu, layout_cpu, pyramid_cpu, synth
from vfi_amd.steerable.SCFpyr_PyTorch import SCFpyr_PyTorch
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.values import DecompValues

import pyramid_grad_ref as ref

pytestmark = pytest.mark.gpu
S2 = math.sqrt(2)
SIZES = [(64, 96), (65, 77), (90, 120), (256, 256), (720, 1280), (1080, 1920)]


def _leaf(t, device):
    return t.to(device).requires_grad_()


def _gradient_image(n, h, w, seed=5):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, h, w)).astype(np.float32))


def _close(got, want, what, rel=1e-4):
    """|got - want| <= rel * max|want| (per level / field)."""
    want = want.double()
    err = float((got.detach().double().cpu() - want).abs().max())
    scale = float(want.abs().max())
    assert err <= rel * scale, f"{what}: max|err| {err:.3e} vs max|grad| {scale:.3e}"


def _polar_backward(pyr, v, g, device):
    high, low = _leaf(v.high_level, device), _leaf(v.low_level, device)
    phase, amp = [_leaf(p, device) for p in v.phase], [_leaf(a, device) for a in v.amplitude]
    out = pyr.inv_filter(DecompValues(high, phase, amp, low))
    out.backward(g.to(device))
    return high.grad, [p.grad for p in phase], [a.grad for a in amp], low.grad


def test_inv_filter_output_carries_a_grad_fn(device):
    h, w = 64, 96
    height = layout_cpu.calc_pyr_height(h, w)
    v = synth.synthetic_vals(1, 1, h, w, height)
    high = _leaf(v.high_level, device)
    out = Pyramid(height, 4, S2, device).inv_filter(
        DecompValues(high, [p.to(device) for p in v.phase], [a.to(device) for a in v.amplitude], v.low_level.to(device)))
    assert out.grad_fn is not None
    out.sum().backward()
    assert high.grad is not None


@pytest.mark.parametrize("h,w", SIZES)
def test_polar_gradients_match_float64_adjoint(h, w, device):
    n = 3
    height = layout_cpu.calc_pyr_height(h, w)
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    v = synth.synthetic_vals(7, n, h, w, height)
    g = _gradient_image(n, h, w)
    gh, gp, ga, gl = _polar_backward(Pyramid(height, 4, S2, device), v, g, device)
    rhi, rb, rlo = ref.adjoint64(spec, g)
    _close(gh.squeeze(1), rhi, "high")
    _close(gl.squeeze(1), rlo, "low")
    for k in range(spec.nlev):
        dphi, damp = ref.polar_grads(rb[k], v.phase[k], v.amplitude[k])
        _close(gp[k], dphi, f"phase level {k}")
        _close(ga[k], damp, f"amplitude level {k}")


@pytest.mark.parametrize("h,w", SIZES)
def test_complex_gradients_match_float64_adjoint(h, w, device):
    n = 3
    height = layout_cpu.calc_pyr_height(h, w)
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    coeff = layout_cpu.values_to_coeff(synth.synthetic_vals(8, n, h, w, height))
    leaves = [_leaf(coeff[0], device)] + [[_leaf(b, device) for b in lv] for lv in coeff[1:-1]] + [_leaf(coeff[-1], device)]
    g = _gradient_image(n, h, w, seed=6)
    SCFpyr_PyTorch(height, 4, S2, device).reconstruct(leaves).backward(g.to(device))
    rhi, rb, rlo = ref.adjoint64(spec, g)
    _close(leaves[0].grad, rhi, "high")
    _close(leaves[-1].grad, rlo, "low")
    for k in range(spec.nlev):
        got = torch.stack([b.grad for b in leaves[1 + k]])
        want = torch.stack([torch.view_as_real(z) for z in rb[k]])
        _close(got, want, f"level {k}")


def test_adjoint_identity_1080p(device):
    """<reconstruct(v), g> = sum_i <v_i, grad_i> (the synthesis is linear in the complex surface's inputs)."""
    n, h, w = 3, 1080, 1920
    height = layout_cpu.calc_pyr_height(h, w)
    coeff = layout_cpu.values_to_coeff(synth.synthetic_vals(9, n, h, w, height))
    leaves = [_leaf(coeff[0], device)] + [[_leaf(b, device) for b in lv] for lv in coeff[1:-1]] + [_leaf(coeff[-1], device)]
    g = _gradient_image(n, h, w, seed=10).to(device)
    out = SCFpyr_PyTorch(height, 4, S2, device).reconstruct(leaves)
    out.backward(g)
    lhs = float((out.detach().double() * g.double()).sum())
    flat = [leaves[0]] + [b for lv in leaves[1:-1] for b in lv] + [leaves[-1]]
    rhs = sum(float((t.detach().double() * t.grad.double()).sum()) for t in flat)
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


def test_dropped_levels_and_high_level_zero(device):
    """PhaseNet's output: high_level = 0 and scalar-0 levels (src/phase_net/phase_net.py:91-93,127-128)."""
    n, h, w = 2, 90, 120
    height = layout_cpu.calc_pyr_height(h, w)
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    v = synth.synthetic_vals(11, n, h, w, height)
    dropped = {1, spec.nlev - 2}
    phase = [0 if k in dropped else _leaf(p, device) for k, p in enumerate(v.phase)]
    amp = [0 if k in dropped else _leaf(a, device) for k, a in enumerate(v.amplitude)]
    low = _leaf(v.low_level, device)
    pyr = Pyramid(height, 4, S2, device)
    pyr.set_full_size(h, w)
    out = pyr.inv_filter(DecompValues(0, phase, amp, low))
    g = _gradient_image(n, h, w, seed=12)
    grads = torch.autograd.grad(out, [t for t in phase + amp if torch.is_tensor(t)] + [low], g.to(device))
    _, rb, rlo = ref.adjoint64(spec, g)
    it = iter(grads)
    gp = [None if k in dropped else next(it) for k in range(spec.nlev)]
    ga = [None if k in dropped else next(it) for k in range(spec.nlev)]
    _close(next(it).squeeze(1), rlo, "low")
    for k in range(spec.nlev):
        if k in dropped:
            continue
        dphi, damp = ref.polar_grads(rb[k], v.phase[k], v.amplitude[k])
        _close(gp[k], dphi, f"phase level {k}")
        _close(ga[k], damp, f"amplitude level {k}")
    # the Function's own backward returns None for the scalar entries
    from vfi_amd.steerable.SCFpyr_PyTorch import Synthesis
    assert out.grad_fn.name().startswith(Synthesis.__name__)


def test_zero_amplitudes_give_finite_gradients(device):
    n, h, w = 2, 64, 96
    height = layout_cpu.calc_pyr_height(h, w)
    v = synth.synthetic_vals(13, n, h, w, height)
    v.amplitude[0].zero_()
    v.amplitude[2][:, :, ::3] = 0.0
    gh, gp, ga, gl = _polar_backward(Pyramid(height, 4, S2, device), v, _gradient_image(n, h, w), device)
    for t in [gh, gl] + gp + ga:
        assert torch.isfinite(t).all()
    assert float(gp[0].abs().max()) == 0.0 and float(ga[0].abs().max()) > 0.0
    assert float(gp[2][:, :, ::3].abs().max()) == 0.0


def test_needs_input_grad_subsets(device):
    n, h, w = 2, 65, 77
    height = layout_cpu.calc_pyr_height(h, w)
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    v = synth.synthetic_vals(14, n, h, w, height)
    g = _gradient_image(n, h, w, seed=15)
    _, rb, _ = ref.adjoint64(spec, g)
    pyr = Pyramid(height, 4, S2, device)
    amp = [a.to(device) for a in v.amplitude]
    amp[3].requires_grad_()
    phase = [p.to(device) for p in v.phase]
    phase[0].requires_grad_()
    high = v.high_level.to(device).requires_grad_()
    out = pyr.inv_filter(DecompValues(high, phase, amp, v.low_level.to(device)))
    (ga3,) = torch.autograd.grad(out, [amp[3]], g.to(device), retain_graph=True)
    _close(ga3, ref.polar_grads(rb[3], v.phase[3], v.amplitude[3])[1], "amplitude level 3")
    out.backward(g.to(device))
    assert amp[3].grad is not None and phase[0].grad is not None and high.grad is not None
    assert all(a.grad is None for k, a in enumerate(amp) if k != 3)
    _close(phase[0].grad, ref.polar_grads(rb[0], v.phase[0], v.amplitude[0])[0], "phase level 0")


def test_backward_is_deterministic(device):
    n, h, w = 3, 256, 256
    height = layout_cpu.calc_pyr_height(h, w)
    v = synth.synthetic_vals(16, n, h, w, height)
    pyr = Pyramid(height, 4, S2, device)
    g = _gradient_image(n, h, w)
    a = _polar_backward(pyr, v, g, device)
    b = _polar_backward(pyr, v, g, device)
    flat = lambda r: [r[0], *r[1], *r[2], r[3]]
    for x, y in zip(flat(a), flat(b)):
        assert torch.equal(x, y)


_WAVE_SCRIPT = r"""
import math, sys
import torch
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
from oracle import layout_cpu, synth
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.values import DecompValues
import numpy as np
dev = torch.device("cuda:0")
h, w, n = {h}, {w}, 3
height = layout_cpu.calc_pyr_height(h, w)
v = synth.synthetic_vals(17, n, h, w, height)
leaf = lambda t: t.to(dev).requires_grad_()
high, low = leaf(v.high_level), leaf(v.low_level)
phase, amp = [leaf(p) for p in v.phase], [leaf(a) for a in v.amplitude]
out = Pyramid(height, 4, math.sqrt(2), dev).inv_filter(DecompValues(high, phase, amp, low))
g = torch.from_numpy(np.random.default_rng(5).standard_normal((n, h, w)).astype(np.float32)).to(dev)
out.backward(g)
torch.save([high.grad.cpu(), low.grad.cpu()] + [p.grad.cpu() for p in phase] + [a.grad.cpu() for a in amp], {out!r})
"""


@pytest.mark.parametrize("h,w", [(256, 256), (720, 1280)])
def test_generic_engine_agrees_with_wave_engine(h, w, tmp_path):
    """VFI_PYR_WAVE=0 (read once per process: one fresh child per setting) runs every pass on the generic LDS engine."""
    res = []
    for wave in ("7", "0"):
        out = str(tmp_path / f"grads_{wave}.pt")
        script = _WAVE_SCRIPT.format(root=ROOT, pkg=PKG_DIR, tests=os.path.join(ROOT, "tests"), h=h, w=w, out=out)
        env = dict(os.environ, VFI_PYR_WAVE=wave)
        subprocess.run([sys.executable, "-c", script], env=env, check=True, timeout=600)
        res.append(torch.load(out))
    for i, (a, b) in enumerate(zip(*res)):
        err = float((a - b).abs().max())
        assert err <= 2e-5 * float(b.abs().max()), (i, err)


def test_inference_output_unchanged_by_requires_grad(device):
    n, h, w = 3, 90, 120
    height = layout_cpu.calc_pyr_height(h, w)
    v = synth.synthetic_vals(18, n, h, w, height)
    pyr = Pyramid(height, 4, S2, device)
    dv = lambda req: DecompValues(v.high_level.to(device).requires_grad_(req),
                                  [p.to(device).requires_grad_(req) for p in v.phase],
                                  [a.to(device).requires_grad_(req) for a in v.amplitude], v.low_level.to(device))
    plain = pyr.inv_filter(dv(False))
    tracked = pyr.inv_filter(dv(True))
    with torch.no_grad():
        untracked = pyr.inv_filter(dv(True))
    assert tracked.grad_fn is not None and untracked.grad_fn is None
    assert torch.equal(plain, tracked.detach()) and torch.equal(plain, untracked)


def _train_losses(pyr, device, steps, lr=0.02):
    """A tiny model trained through inv_filter: per level a 1x1 conv maps the (phase, amplitude) of frames 0 and 2 to the
    middle frame's; the loss is the reference's get_loss (src/train/loss.py:5-25): L1 + 0.005 * phase term."""
    f0, f1, f2 = (color_cpu.rgb2lab_single(torch.from_numpy(x)).to(device) for x in synth.translating_pair(11, 128, 128))
    nb = 4
    with torch.no_grad():
        v0, v1, v2 = pyr.filter(f0), pyr.filter(f1), pyr.filter(f2)
    nlev = len(v0.phase)
    convs = [torch.nn.Conv2d(4 * nb, 2 * nb, 1) for _ in range(nlev)]
    for c in convs:
        torch.nn.init.zeros_(c.weight)
        torch.nn.init.zeros_(c.bias)
    convs = torch.nn.ModuleList(convs).to(device)
    opt = torch.optim.Adam(convs.parameters(), lr=lr)
    high, low = (v0.high_level + v2.high_level) / 2, (v0.low_level + v2.low_level) / 2
    losses = []
    for _ in range(steps):
        phase, amp = [], []
        for k in range(nlev):
            sh = v0.phase[k].shape
            x = torch.cat([t[k].reshape(3, nb, *sh[2:]) for t in (v0.phase, v2.phase, v0.amplitude, v2.amplitude)], 1)
            y = convs[k](x)
            phase.append(y[:, :nb].reshape(sh))
            amp.append(y[:, nb:].reshape(sh))
        out = pyr.inv_filter(DecompValues(high, phase, amp, low))
        phase_loss = 0
        for pr, pt in zip(phase, v1.phase):
            d = pt.reshape(-1, nb, *pt.shape[2:]).permute(1, 0, 2, 3) - pr.reshape(-1, nb, *pr.shape[2:]).permute(1, 0, 2, 3)
            for o in d:
                phase_loss = phase_loss + torch.mean(torch.abs(torch.atan2(torch.sin(o), torch.cos(o)).reshape(-1)), 0)
        loss = torch.nn.functional.l1_loss(out, f1) + 0.005 * phase_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_training_through_inv_filter(device):
    height = layout_cpu.calc_pyr_height(128, 128)
    torch.manual_seed(0)
    gpu = _train_losses(Pyramid(height, 4, S2, device), device, 50)
    assert gpu[-1] <= 0.5 * gpu[0], gpu
    cpu = _train_losses(pyramid_cpu.Pyramid(height), torch.device("cpu"), 5)
    for a, b in zip(gpu[:5], cpu):
        assert abs(a - b) <= 0.02 * abs(b), (gpu[:5], cpu)
