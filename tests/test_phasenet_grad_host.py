"""CPU host models of every adjoint of the PhaseNet block backward against float64 autograd, and
`get_loss` against values the reference's own src/train/loss.py produced (tests/golden/phasenet_loss.npz)."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import phasenet_grad_ref as R
import test_fusionnet_grad_host as FH

RESIZE_SIZES = [((1, 1), (1, 1)), ((1, 1), (2, 3)), ((2, 3), (3, 4)), ((5, 7), (7, 10)), ((8, 11), (11, 16)),
                ((4, 4), (8, 8)), ((5, 5), (5, 5)), ((9, 13), (4, 5))]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("src,dst", RESIZE_SIZES)
def test_resize_model_matches_torch_and_its_own_adjoint(src, dst):
    rng = np.random.default_rng(src[0] * 100 + dst[1])
    x, g = rng.standard_normal((2, 3) + src), rng.standard_normal((2, 3) + dst)
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = F.interpolate(xt, size=dst, mode="bilinear", align_corners=False)
    (yt * torch.from_numpy(g)).sum().backward()
    # the model's weights carry the fp32 rounding of the coordinate (about coordinate * 2^-23): 1e-4 is far above it
    assert _rel(R.resize_forward(x, dst), yt.detach().numpy()) <= 1e-4
    adj = R.resize_adjoint(g, src)
    assert _rel(adj, xt.grad.numpy()) <= 1e-4
    lhs, rhs = float((R.resize_forward(x, dst) * g).sum()), float((x * adj).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))
    # the kernel's gather form (candidate range + re-evaluated forward arithmetic) is that transpose
    assert np.abs(R.resize_adjoint_gather(g, src) - adj).max() <= 1e-12


def test_resize_x2_equals_the_existing_x2_adjoint_model():
    rng = np.random.default_rng(0)
    x, g = rng.standard_normal((2, 3, 4, 4)), rng.standard_normal((2, 3, 8, 8))
    assert np.abs(R.resize_adjoint(g, (4, 4)) - FH.up2_adjoint(x, g, False)).max() <= 1e-12


@pytest.mark.parametrize("n_in,n_out", [(1, 1), (1, 7), (7, 1), (2, 3), (5, 7), (7, 10), (64, 92), (65, 92), (130, 184),
                                        (540, 764), (764, 1080), (1358, 1920), (13, 5), (100, 3), (3, 100), (17, 17)])
def test_candidate_range_covers_every_output_that_hits_a_source(n_in, n_out):
    """resize_candidates (integer arithmetic, one output of slack) never misses an output that reads the source with a
    non-zero fp32 weight (an output clamped to coordinate 0 names source 1 as its second tap, with weight 0)."""
    hits = {s: [] for s in range(n_in)}
    for o in range(n_out):
        i0, i1, l = R.resize_taps(o, n_in, n_out)
        if l != 1.0:
            hits[i0].append(o)
        if l != 0.0:
            hits[i1].append(o)
    for s in range(n_in):
        lo, hi = R.resize_candidates(s, n_in, n_out)
        assert 0 <= lo and hi <= n_out - 1
        assert all(lo <= o <= hi for o in hits[s]), (s, lo, hi, hits[s])


def test_activation_backward_formulas():
    g = torch.Generator().manual_seed(1)
    z = (torch.randn(4100, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    up = torch.randn(4100, generator=g, dtype=torch.float64)
    y = F.elu(z)
    (y * up).sum().backward()
    assert np.abs(R.elu_backward(up.numpy(), y.detach().numpy()) - z.grad.numpy()).max() <= 1e-12
    z.grad = None
    y = torch.tanh(z)
    (y * up).sum().backward()
    assert np.abs(R.tanh_backward(up.numpy(), y.detach().numpy()) - z.grad.numpy()).max() <= 1e-12


def test_blend_backward_formulas():
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    pred = torch.tanh(r(3, 8, 5, 7)).requires_grad_(True)
    amp_in, max_amp = torch.rand((3, 8, 5, 7), generator=g, dtype=torch.float64), torch.rand(3, generator=g, dtype=torch.float64) + 0.5
    gp, ga = r(3, 4, 5, 7), r(3, 4, 5, 7)
    phase, amp = R.emit(pred, amp_in, max_amp)
    ((phase * gp).sum() + (amp * ga).sum()).backward()
    want = pred.grad.numpy()
    assert np.abs(R.emit_backward(gp.numpy(), ga.numpy(), amp_in.numpy(), max_amp.numpy()) - want).max() <= 1e-12
    only_amp = R.emit_backward(None, ga.numpy(), amp_in.numpy(), max_amp.numpy())
    assert (only_amp[:, :4] == 0).all() and np.abs(only_amp[:, 4:] - want[:, 4:]).max() <= 1e-12
    p0 = torch.tanh(r(3, 1, 5, 7)).requires_grad_(True)
    low_in, max_low, gl = r(3, 2, 5, 7), torch.rand(3, generator=g, dtype=torch.float64) + 0.5, r(3, 1, 5, 7)
    (R.emit_low(p0, low_in, max_low) * gl).sum().backward()
    assert np.abs(R.emit_low_backward(gl.numpy(), low_in.numpy(), max_low.numpy()) - p0.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("ks", [1, 3])
def test_bn_unfold_matches_autograd(ks):
    """Gradients of the folded (wf, bf) unfold into those of (w, b, gamma, beta) of conv -> eval BatchNorm."""
    sd = {k: v.double() for k, v in R.block_state(5, 6, 1, ks, cout=4).items() if v.dtype.is_floating_point}
    w, b, gamma, beta = (sd[k].clone().requires_grad_(True) for k in R.BLOCK_KEYS[:4])
    mean, var, eps = sd["feature_map.1.running_mean"], sd["feature_map.1.running_var"], 1e-5
    assert float(var.min()) >= 0.5 and float(var.max()) <= 2.0 and float(mean.abs().max()) > 0.1
    g = torch.Generator().manual_seed(3)
    x, up = torch.randn((2, 6, 5, 7), generator=g, dtype=torch.float64), torch.randn((2, 4, 5, 7), generator=g, dtype=torch.float64)
    pad = lambda t: F.pad(t, (1, 1, 1, 1), mode="reflect") if ks == 3 else t
    y = F.batch_norm(F.conv2d(pad(x), w, b), mean, var, gamma, beta, False, 0.0, eps)
    (y * up).sum().backward()
    s = (gamma / torch.sqrt(var + eps)).detach()
    wf = (w.detach() * s.view(-1, 1, 1, 1)).requires_grad_(True)
    bf = ((b.detach() - mean) * s + beta.detach()).requires_grad_(True)
    yf = F.conv2d(pad(x), wf, bf)
    assert float((yf - y).detach().abs().max()) <= 1e-12
    (yf * up).sum().backward()
    got = R.bn_unfold(wf.grad, bf.grad, w.detach(), b.detach(), gamma.detach(), mean, var, eps)
    for a, p in zip(got, (w, b, gamma, beta)):
        assert float((a - p.grad).abs().max()) <= 1e-12 * max(1.0, float(p.grad.abs().max()))


# ---- the loss against the reference's own values -------------------------------------------------------------------------
def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "phasenet_loss.npz"))
    return {k: z[k] for k in z.files}


def test_loss_restatement_matches_reference_fixture(golden_dir):
    z = _fixture(golden_dir)
    t = lambda k: torch.from_numpy(z[k]).double()
    assert z["phase_o0"].shape == (8, 1, 5, 7) and z["phase_o1"].shape == (8, 1, 7, 10) and z["output"].shape == (2, 3, 12, 16)
    for i in (0, 1):        # the construction keeps the cut and the kink out of reach
        d = R.wrap(t(f"phase_t{i}") - t(f"phase_o{i}")).abs()
        assert 0.04 <= float(d.min()) and float(d.max()) <= math.pi - 0.04
    assert float((t("output") - t("target")).abs().min()) >= 0.009
    got = R.get_loss([t("phase_o0"), t("phase_o1")], [t("phase_t0"), t("phase_t1")], t("output"), t("target"), int(z["nbands"]),
                     float(z["weighting_factor"]))
    for a, k in zip(got, ("total_loss", "l_1_p", "phase_loss_p")):
        assert abs(float(a) - float(z[k])) <= 1e-6 * abs(float(z[k])), k
    # the single-reduction form the HIP node computes: nbands * mean over the whole level
    one = sum(4 * R.wrap(t(f"phase_t{i}") - t(f"phase_o{i}")).abs().mean() for i in (0, 1))
    l1 = (t("output") - t("target")).abs().mean()
    assert abs(float(l1 + 0.005 * one) - float(z["total_loss"])) <= 1e-12


def test_get_loss_on_cpu_tensors_matches_reference_fixture(golden_dir):
    """vfi_amd.train.loss.get_loss (the torch expression it takes for anything but HIP fp32 tensors) returns the reference's
    three values, and its gradients are those of the restatement."""
    from vfi_amd.train.loss import get_loss
    z = _fixture(golden_dir)
    t = lambda k: torch.from_numpy(z[k]).double()
    po = [t("phase_o0").requires_grad_(True), t("phase_o1").requires_grad_(True)]
    out = t("output").requires_grad_(True)
    vals_o, vals_t = types.SimpleNamespace(phase=po), types.SimpleNamespace(phase=[t("phase_t0"), t("phase_t1")])
    got = get_loss(vals_o, vals_t, out, t("target"), types.SimpleNamespace(nbands=4))
    for a, k in zip(got, ("total_loss", "l_1_p", "phase_loss_p")):
        assert abs(float(a.detach()) - float(z[k])) <= 1e-6 * abs(float(z[k])), k
    got[0].backward()
    po2 = [t("phase_o0").requires_grad_(True), t("phase_o1").requires_grad_(True)]
    out2 = t("output").requires_grad_(True)
    R.get_loss(po2, [t("phase_t0"), t("phase_t1")], out2, t("target"), 4)[0].backward()
    for a, b in zip(po + [out], po2 + [out2]):
        assert float((a.grad - b.grad).abs().max()) <= 1e-15


def test_block_in_training_mode_refuses_and_parents_still_refuse_train():
    from vfi_amd.phase_net.core import PhaseNetCore
    from vfi_amd.phase_net.phase_net import PhaseNetBlock
    blk = PhaseNetBlock(2, 64, 1, (1, 1))
    assert not blk.training
    blk.train(True)
    with pytest.raises(NotImplementedError, match="batch-statistics"):
        blk(torch.zeros(1, 2, 4, 4))
    with pytest.raises(NotImplementedError):
        PhaseNetCore(4, "cpu").train(True)
