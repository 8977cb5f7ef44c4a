"""GPU checks of FunctionAdaCoF.backward (one launch of vfi_adacof_backward): parity with the reference's own
backward kernels (tests/golden/adacof_grad_*.npz), with the float64 autograd of a torch restatement of the forward
for general channel counts / filter sizes, gradient subsets, determinism, a full-size band, and an end-to-end
training run of a small torch model through the op."""
import copy
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from adacof_grad_ref import adacof_restated, restated_grads
from conftest import GOLDEN
from vfi_amd.adacof.cupy_module.adacof import FunctionAdaCoF

pytestmark = pytest.mark.gpu

# Against the reference's fp32 kernels: the HIP kernel forms the same products, but with precomputed bilinear weights,
# fma contraction and the offset sums weighted once per tap instead of once per channel; the gradients are sums of
# 3 channel terms of magnitude <= ~15, so the differences are a few ulp of that.
ATOL_REF = 5e-5
# Against the float64 restatement: the same fp32 rounding, up to 6 channels.
ATOL_F64 = 1e-4

GRAD_CASES = sorted(glob.glob(os.path.join(GOLDEN, "adacof_grad_*.npz")))
NAMES = ("grad_weight", "grad_offset_i", "grad_offset_j")


def _dev(a, device, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).requires_grad_(grad)


def _case(seed, n, c, h, w, f, dil, amp=3.0):
    rng = np.random.default_rng(seed)
    hin, win = h + (f - 1) * dil, w + (f - 1) * dil
    lg = rng.standard_normal((n, f * f, h, w))
    return dict(input=rng.random((n, c, hin, win), dtype=np.float32),
                weight=(np.exp(lg) / np.exp(lg).sum(1, keepdims=True)).astype(np.float32),
                offset_i=np.clip(rng.standard_normal((n, f * f, h, w)) * amp, -8, 8).astype(np.float32),
                offset_j=np.clip(rng.standard_normal((n, f * f, h, w)) * amp, -8, 8).astype(np.float32),
                grad_output=rng.standard_normal((n, c, h, w)).astype(np.float32))


def _gpu_grads(c, dil, device, want=(True, True, True), want_input=False):
    x = _dev(c["input"], device, want_input)
    leaves = [_dev(c[k], device, g) for k, g in zip(("weight", "offset_i", "offset_j"), want)]
    out = FunctionAdaCoF.apply(x, *leaves, dil)
    wrt = [t for t in leaves if t.requires_grad] + ([x] if want_input else [])
    got = torch.autograd.grad(out, wrt, _dev(c["grad_output"], device))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("path", GRAD_CASES, ids=[os.path.basename(p)[12:-4] for p in GRAD_CASES])
def test_backward_matches_reference_fixture(path, device):
    g = np.load(path)
    got = _gpu_grads(g, int(g["dilation"]), device)
    for name, t in zip(NAMES, got):
        np.testing.assert_allclose(t.cpu().numpy(), g[name], rtol=0, atol=ATOL_REF, err_msg=name)


@pytest.mark.parametrize("c", [1, 3, 4, 6])
@pytest.mark.parametrize("f,dil", [(3, 1), (3, 2), (5, 1), (5, 2), (7, 1), (7, 2)])
@pytest.mark.parametrize("w", [20, 17])          # 17: odd width (partial tiles, unaligned rows)
def test_backward_general_channels_and_filters(c, f, dil, w, device):
    case = _case(100 * c + 10 * f + dil + w, 2, c, 11, w, f, dil)
    got = _gpu_grads(case, dil, device)
    ref = restated_grads(case["input"], case["weight"], case["offset_i"], case["offset_j"], dil, case["grad_output"])
    for name, t, r in zip(NAMES, got, ref):
        np.testing.assert_allclose(t.cpu().double().numpy(), r.numpy(), rtol=0, atol=ATOL_F64, err_msg=name)


def test_backward_gradient_subsets(device):
    case = _case(5, 1, 3, 24, 40, 5, 1)
    all3 = _gpu_grads(case, 1, device)
    x = _dev(case["input"], device)
    for want in ((False, False, True), (True, False, False), (False, True, False)):
        leaves = [_dev(case[k], device, g) for k, g in zip(("weight", "offset_i", "offset_j"), want)]
        out = FunctionAdaCoF.apply(x, *leaves, 1)
        out.backward(_dev(case["grad_output"], device))
        torch.cuda.synchronize()
        for leaf, full, g in zip(leaves, all3, want):
            if g:
                assert torch.equal(leaf.grad, full), want     # bit for bit the all-three values
            else:
                assert leaf.grad is None, want
        assert x.grad is None


def test_sum_backward_and_zero_input_gradient(device):
    case = _case(6, 1, 3, 16, 24, 5, 1)
    x = _dev(case["input"], device, True)
    leaves = [_dev(case[k], device, True) for k in ("weight", "offset_i", "offset_j")]
    FunctionAdaCoF.apply(x, *leaves, 1).sum().backward()    # grad_output is an expanded (non-contiguous) view
    torch.cuda.synchronize()
    ones = np.ones_like(case["grad_output"])
    ref = restated_grads(case["input"], case["weight"], case["offset_i"], case["offset_j"], 1, ones)
    for name, leaf, r in zip(NAMES, leaves, ref):
        np.testing.assert_allclose(leaf.grad.cpu().double().numpy(), r.numpy(), rtol=0, atol=ATOL_F64, err_msg=name)
    # the reference allocates the input gradient and never fills it (adacof.py:382)
    assert x.grad is not None and x.grad.shape == x.shape and not x.grad.any()


def test_backward_is_deterministic(device):
    case = _case(7, 2, 3, 64, 128, 5, 1, amp=6.0)
    a = _gpu_grads(case, 1, device)
    b = _gpu_grads(case, 1, device)
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("y0", [520, 1064])    # a middle band and the bottom band (taps clamp at the edge)
def test_backward_full_size_band(y0, device):
    """1080x1920 output, F = 5, offsets ~N(0, 2) clipped to +-8.  The taps of one output row depend only on that row's
    (w, alpha, beta) and the full input, so a 16-row band is checked against the restatement on the CPU."""
    h, w, f, band = 1080, 1920, 5, 16
    g = torch.Generator().manual_seed(y0)
    x = torch.rand((1, 3, h + f - 1, w + f - 1), generator=g)
    wt = torch.softmax(torch.randn((1, f * f, h, w), generator=g), 1)
    a = (torch.randn((1, f * f, h, w), generator=g) * 2).clamp(-8, 8)
    b = (torch.randn((1, f * f, h, w), generator=g) * 2).clamp(-8, 8)
    go = torch.randn((1, 3, h, w), generator=g)
    leaves = [t.to(device).requires_grad_() for t in (wt, a, b)]
    got = torch.autograd.grad(FunctionAdaCoF.apply(x.to(device), *leaves, 1), leaves, go.to(device))
    rows = slice(y0, y0 + band)
    ref = restated_grads(x, wt[:, :, rows], a[:, :, rows], b[:, :, rows], 1, go[:, :, rows], y0=y0)
    for name, t, r in zip(NAMES, got, ref):
        np.testing.assert_allclose(t[:, :, rows].cpu().double().numpy(), r.numpy(), rtol=0, atol=ATOL_F64,
                                   err_msg=name)


# ---- training through the op ----------------------------------------------------------------------------------
F_T, H_T, W_T = 5, 32, 48


class _KernelNet(nn.Module):
    """Predicts softmaxed AdaCoF weights and both offsets from two frames (plain torch.nn layers)."""

    def __init__(self):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(6, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=1), nn.ReLU())
        self.w = nn.Conv2d(16, F_T * F_T, 3, padding=1)
        self.a = nn.Conv2d(16, F_T * F_T, 3, padding=1)
        self.b = nn.Conv2d(16, F_T * F_T, 3, padding=1)

    def forward(self, f0, f1):
        h = self.body(torch.cat((f0, f1), 1))
        return torch.softmax(self.w(h), 1), self.a(h), self.b(h)


def _training_data():
    """A smooth random frame, a second frame, and a target = frame 0 shifted by (0.3, -0.4) px."""
    g = torch.Generator().manual_seed(0)
    big = Fn.interpolate(torch.rand((1, 3, H_T // 4 + 2, W_T // 4 + 2), generator=g), size=(H_T + 8, W_T + 8),
                         mode="bicubic", align_corners=False)
    f0 = big[:, :, 4:4 + H_T, 4:4 + W_T].contiguous()
    f1 = big[:, :, 5:5 + H_T, 3:3 + W_T].contiguous()
    yy = torch.arange(H_T).view(H_T, 1) + 4.3
    xx = torch.arange(W_T).view(1, W_T) + 3.6
    y0, x0 = yy.floor().long(), xx.floor().long()
    fy, fx = yy - y0, xx - x0
    tgt = (big[:, :, y0, x0] * (1 - fy) * (1 - fx) + big[:, :, y0 + 1, x0] * fy * (1 - fx)
           + big[:, :, y0, x0 + 1] * (1 - fy) * fx + big[:, :, y0 + 1, x0 + 1] * fy * fx)
    pad = (F_T - 1) // 2
    return f0, f1, Fn.pad(f0, (pad,) * 4, mode="replicate"), tgt


def test_training_step_gradients_match_float64(device):
    torch.manual_seed(0)
    net = _KernelNet().to(device)
    ref_net = copy.deepcopy(net).double().cpu()
    f0, f1, padded, tgt = _training_data()
    with torch.backends.cudnn.flags(enabled=True, allow_tf32=False):    # full fp32 convolutions for this comparison
        w, a, b = net(f0.to(device), f1.to(device))
        out = FunctionAdaCoF.apply(padded.to(device), w, a, b, 1)
        (out - tgt.to(device)).abs().mean().backward()
    # same step in float64 on the CPU; the L1 subgradient takes the GPU output's signs, so a pixel that sits on the
    # kink cannot flip between the two precisions
    sign = torch.sign(out.detach() - tgt.to(device)).double().cpu()
    rw, ra, rb = ref_net(f0.double(), f1.double())
    ref_out = adacof_restated(padded.double(), rw, ra, rb, 1)
    (ref_out * sign).sum().div(sign.numel()).backward()
    torch.cuda.synchronize()
    # fp32 (convolutions + this op) against fp64: relative to each gradient's own scale
    for (name, p), q in zip(net.named_parameters(), ref_net.parameters()):
        scale = float(q.grad.abs().max())
        np.testing.assert_allclose(p.grad.cpu().double().numpy(), q.grad.numpy(), rtol=1e-3, atol=1e-3 * scale,
                                   err_msg=name)


def test_training_reduces_loss(device):
    torch.manual_seed(0)
    net = _KernelNet().to(device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    f0, f1, padded, tgt = (t.to(device) for t in _training_data())
    losses = []
    for _ in range(50):
        w, a, b = net(f0, f1)
        loss = (FunctionAdaCoF.apply(padded, w, a, b, 1) - tgt).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < 0.5 * losses[0], losses
