"""CPU checks behind the AdaCoF network's HIP backward: which modules may enter training mode, the
float64 host models of the glue adjoints (tests/adacofnet_grad_ref.py, written the way csrc/vfi_adacofnet_grad.hip computes
them) against torch autograd and the adjoint identity, and the training dict's two smoothness terms against the values the
reference's own forward produced (tests/golden/adacofnet_smoothness.npz)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adacofnet_grad_ref as R
from conftest import GOLDEN

ARGS = types.SimpleNamespace(kernel_size=5, dilation=1, gpu_id=0)


# ---- train-mode permissions ---------------------------------------------------------------------------------------
def test_plain_adacofnet_may_train():
    from vfi_amd.adacof.models.adacofnet import AdaCoFNet
    net = AdaCoFNet(ARGS)
    assert not net.training
    net.train(True)
    assert net.training and net.get_kernel.training
    net.eval()
    assert not net.training and not net.get_kernel.training


def test_kernel_estimation_may_train():
    from vfi_amd.adacof.models.adacofnet import KernelEstimation
    est = KernelEstimation(5)
    est.train(True)
    assert est.training
    est.train(False)
    assert not est.training


def test_model_wrapping_the_plain_variant_may_train(monkeypatch):
    from vfi_amd.adacof import models
    from vfi_amd.adacof.models import adacofnet
    monkeypatch.setattr(adacofnet, "make_model", lambda args: adacofnet.AdaCoFNet(args))     # no device needed
    m = models.Model(types.SimpleNamespace(model="vfi_amd.adacof.models.adacofnet", **vars(ARGS)))
    m.train(True)
    assert m.training and m.model.training
    m.eval()
    assert not m.model.training


def test_fusion_variant_and_packed_module_still_refuse(monkeypatch):
    from vfi_amd.adacof import models
    from vfi_amd.fusion_net import fusion_adacofnet
    from vfi_amd.nn_util import PackedModule
    with pytest.raises(NotImplementedError):
        fusion_adacofnet.AdaCoFNet(ARGS).train(True)
    with pytest.raises(NotImplementedError):
        PackedModule().train(True)
    monkeypatch.setattr(fusion_adacofnet, "make_model", lambda args: fusion_adacofnet.AdaCoFNet(args))
    m = models.Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", **vars(ARGS)))
    with pytest.raises(NotImplementedError):
        m.train(True)


# ---- host models of the glue adjoints -----------------------------------------------------------------------------
def _t(x):
    return torch.from_numpy(x)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (2, 3), (5, 9)])
@pytest.mark.parametrize("masked", [False, True])
def test_upsample_adjoint_matches_autograd(h, w, masked):
    rng = np.random.default_rng(h * 10 + w)
    x = rng.standard_normal((2, 3, h, w))
    g = rng.standard_normal((2, 3, 2 * h, 2 * w))
    xt = _t(x).requires_grad_(True)
    (_up(torch.relu(xt) if masked else xt) * _t(g)).sum().backward()
    got = R.up2ac_adjoint(g, np.maximum(x, 0) if masked else None)
    np.testing.assert_allclose(got, xt.grad.numpy(), rtol=0, atol=1e-12)
    lhs = float((_up(_t(x)).numpy() * g).sum())
    rhs = float((x * R.up2ac_adjoint(g)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_upsample_sources_cover_every_output_with_unit_weight():
    for n in range(1, 12):
        tot = np.zeros(2 * n)
        for j in range(n):
            for o, w in R.up2ac_sources(j, n):
                tot[o] += w
        np.testing.assert_allclose(tot, 1.0, atol=1e-15)
        assert max(len(R.up2ac_sources(j, n)) for j in range(n)) <= 5


def test_avgpool_backward_with_skip_and_mask():
    rng = np.random.default_rng(1)
    z = np.round(rng.standard_normal((2, 3, 6, 8)), 1)
    z[0, 0, 0:2, 0:2] = 0.0                   # y == 0 gets no gradient
    gp, gk = rng.standard_normal((2, 3, 3, 4)), rng.standard_normal((2, 3, 6, 8))
    zt = _t(z).requires_grad_(True)
    y = torch.relu(zt)
    ((F.avg_pool2d(y, 2, 2) * _t(gp)).sum() + (y * _t(gk)).sum()).backward()
    got = R.avgpool_backward(np.maximum(z, 0), gp, gk)
    np.testing.assert_allclose(got, zt.grad.numpy(), rtol=0, atol=1e-12)
    assert (got[0, 0, 0:2, 0:2] == 0).all()
    zt.grad = None
    (F.avg_pool2d(torch.relu(zt), 2, 2) * _t(gp)).sum().backward()
    np.testing.assert_allclose(R.avgpool_backward(np.maximum(z, 0), gp), zt.grad.numpy(), rtol=0, atol=1e-12)
    x = rng.standard_normal((2, 3, 6, 8))      # adjoint identity of the pooling itself
    lhs = float((F.avg_pool2d(_t(x), 2, 2).numpy() * gp).sum())
    rhs = float((x * R.avgpool_backward(np.ones_like(x), gp)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_softmax_backward():
    rng = np.random.default_rng(2)
    z, g = rng.standard_normal((2, 9, 4, 5)) * 2, rng.standard_normal((2, 9, 4, 5))
    zt = _t(z).requires_grad_(True)
    w = torch.softmax(zt, 1)
    (w * _t(g)).sum().backward()
    np.testing.assert_allclose(R.softmax_backward(w.detach().numpy(), g), zt.grad.numpy(), rtol=0, atol=1e-12)
    # the Jacobian is symmetric: <J g, y> == <g, J y>
    y = rng.standard_normal(z.shape)
    wn = w.detach().numpy()
    lhs, rhs = float((R.softmax_backward(wn, g) * y).sum()), float((g * R.softmax_backward(wn, y)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def _maps(seed, n=2, f2=9, h=6, w=7):
    rng = np.random.default_rng(seed)
    sm = lambda z: np.exp(z) / np.exp(z).sum(1, keepdims=True)
    r = lambda c: rng.standard_normal((n, c, h, w))
    return [sm(r(f2) * 2), r(f2) * 3, r(f2) * 3, sm(r(f2) * 2), r(f2) * 3, r(f2) * 3, 1 / (1 + np.exp(-r(1)))]


def test_smoothness_forward_and_stencil():
    maps = _maps(3)
    leaves = [_t(x).requires_grad_(True) for x in maps]
    gs, go = R.smoothness(*leaves)
    m, hs, ho = R.smooth_forward(*maps)
    assert abs(hs - float(gs.detach())) <= 1e-12 and abs(ho - float(go.detach())) <= 1e-12
    (0.7 * gs - 1.3 * go).backward()
    np.testing.assert_allclose(-1.3 * R.charb_stencil(maps[6]), leaves[6].grad.numpy(), rtol=0, atol=1e-12)
    for s in (0, 1):
        w, a, b = maps[3 * s:3 * s + 3]
        z = np.zeros_like(w)
        # no sampler gradient: head_backward's smoothness part alone, before the softmax
        f2 = w.shape[1]
        qa, qb = 0.7 * R.charb_stencil(m[:, 2 * s:2 * s + 1]) / f2, 0.7 * R.charb_stencil(m[:, 2 * s + 1:2 * s + 2]) / f2
        np.testing.assert_allclose(qa * a + qb * b, leaves[3 * s].grad.numpy(), rtol=0, atol=1e-12)
        _, ga, gb = R.head_backward(z, z, z, w, a, b, m[:, 2 * s:2 * s + 1], m[:, 2 * s + 1:2 * s + 2], 0.7)
        np.testing.assert_allclose(ga, leaves[3 * s + 1].grad.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(gb, leaves[3 * s + 2].grad.numpy(), rtol=0, atol=1e-12)


def test_head_backward_through_the_softmax():
    rng = np.random.default_rng(4)
    n, f2, h, w = 2, 9, 5, 6
    z, a, b = (rng.standard_normal((n, f2, h, w)) * s for s in (2, 3, 3))
    gw, ga, gb = (rng.standard_normal((n, f2, h, w)) for _ in range(3))
    zt, at, bt = (_t(x).requires_grad_(True) for x in (z, a, b))
    wt = torch.softmax(zt, 1)
    term = lambda m: R.charbonnier(m[:, :, :, :-1] - m[:, :, :, 1:]) + R.charbonnier(m[:, :, :-1, :] - m[:, :, 1:, :])
    loss = (wt * _t(gw)).sum() + (at * _t(ga)).sum() + (bt * _t(gb)).sum() + 0.01 * (
        term((wt * at).mean(1, keepdim=True)) + term((wt * bt).mean(1, keepdim=True)))
    loss.backward()
    wn = wt.detach().numpy()
    m_a, m_b = (wn * a).mean(1, keepdims=True), (wn * b).mean(1, keepdims=True)
    gl, gal, gbe = R.head_backward(gw, ga, gb, wn, a, b, m_a, m_b, 0.01)
    np.testing.assert_allclose(gl, zt.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(gal, at.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(gbe, bt.grad.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("h0,w0", [(6, 8), (5, 7), (6, 3)])
def test_blend_and_sigmoid_head(h0, w0):
    rng = np.random.default_rng(h0 + w0)
    n, h, w = 2, 6, 8
    t1, t2, z = rng.standard_normal((n, 3, h, w)), rng.standard_normal((n, 3, h, w)), rng.standard_normal((n, 1, h, w))
    g = rng.standard_normal((n, 3, h0, w0))
    t1t, t2t, zt = (_t(x).requires_grad_(True) for x in (t1, t2, z))
    occ = torch.sigmoid(zt)
    frame1 = (occ * t1t + (1 - occ) * t2t)[:, :, :h0, :w0]
    term = R.charbonnier(occ[:, :, :, :-1] - occ[:, :, :, 1:]) + R.charbonnier(occ[:, :, :-1, :] - occ[:, :, 1:, :])
    ((frame1 * _t(g)).sum() + 0.005 * term).backward()
    g1, g2, gz = R.blend_backward(g, t1, t2, occ.detach().numpy(), 0.005)
    np.testing.assert_allclose(g1, t1t.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g2, t2t.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(gz, zt.grad.numpy(), rtol=0, atol=1e-12)
    # blend adjoint identity in (t1, t2) for fixed occ: <blend(t1, t2), g> == <t1, g1> + <t2, g2>
    lhs = float((frame1.detach().numpy() * g).sum())
    rhs = float((t1 * g1).sum() + (t2 * g2).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


# ---- the reference's own training dict ----------------------------------------------------------------------------
def test_training_dict_terms_match_the_reference():
    """g_Spatial, g_Occlusion and frame1 as the reference's AdaCoFNet.forward (training branch, float64) returned them for
    the fixture's maps and sides (tests/golden/make_golden_adacofnet_smoothness.py)."""
    d = np.load(os.path.join(GOLDEN, "adacofnet_smoothness.npz"))
    maps = [d[k].astype(np.float64) for k in ("w1", "a1", "b1", "w2", "a2", "b2", "occ")]
    _, gs, go = R.smooth_forward(*maps)
    assert abs(gs - float(d["g_Spatial"])) <= 1e-12 and abs(go - float(d["g_Occlusion"])) <= 1e-12
    ts, to = R.smoothness(*(_t(m) for m in maps))
    assert abs(float(ts) - float(d["g_Spatial"])) <= 1e-12 and abs(float(to) - float(d["g_Occlusion"])) <= 1e-12
    occ = maps[6]
    frame1 = occ * d["t1"].astype(np.float64) + (1 - occ) * d["t2"].astype(np.float64)
    np.testing.assert_allclose(frame1, d["frame1"], rtol=0, atol=1e-12)


def test_utility_charbonnier_on_the_cpu_is_the_reference_expression():
    from vfi_amd.adacof import utility
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn((2, 3, 5, 7), generator=g, dtype=torch.float64), torch.randn((2, 3, 5, 7), generator=g, dtype=torch.float64)
    want = torch.sqrt((a - b) ** 2 + 0.001 ** 2).mean()
    assert float(utility.Module_CharbonnierLoss()(a, b)) == float(want)
    assert float(utility.CharbonnierFunc(a - b)) == float(want)
    f = torch.rand((1, 3, 2, 2), generator=g)
    assert torch.allclose(utility.moduleNormalize(f), f - torch.tensor([0.4631, 0.4352, 0.3990]).view(1, 3, 1, 1))
    p = torch.nn.Parameter(torch.zeros(3))
    args = types.SimpleNamespace(optimizer="ADAMax", lr=1e-3, weight_decay=0, decay_type="step", lr_decay=20, gamma=0.5)
    opt = utility.make_optimizer(args, torch.nn.ParameterList([p]))
    assert isinstance(opt, torch.optim.Adamax) and opt.param_groups[0]["lr"] == 1e-3
    assert isinstance(utility.make_scheduler(args, opt), torch.optim.lr_scheduler.StepLR)
    args.decay_type = "step_10_30"
    assert list(utility.make_scheduler(args, opt).milestones) == [10, 30]
