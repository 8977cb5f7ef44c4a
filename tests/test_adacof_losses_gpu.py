"""The AdaCoF trainer's loss terms on the MI355X: the MSE / L1 autograd nodes, the VGG node against
float64 with pinned decisions, and `Loss` on the network.

VGG tolerances: the loss within 2e-4 relative of float64; the image gradient within 2e-4 relative L2 (the project's bound for
its conv stacks, section 12), exceeded only up to 4 x the error that float32 torch-CPU autograd of the same pinned
restatement (tests/adacof_loss_ref.py) makes against the float64 one -- measured here and printed."""
import types

import pytest
import torch
import torch.nn.functional as F

import adacof_loss_ref as LR
from oracle import nets_cpu
from vfi_amd.adacof import losses, utility
from vfi_amd.adacof.losses import vgg
from vfi_amd.adacof.models import Model

pytestmark = pytest.mark.gpu

DEFAULT = '1*Charb+0.01*g_Spatial+0.005*g_Occlusion'


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("shape", [(2, 3, 40, 50), (1, 3, 7, 9), (3, 1, 1, 5)])
@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_mse_and_l1_loss_nodes(kind, shape, device):
    mod = losses.Module_MSELoss() if kind == "mse" else losses.Module_L1Loss()
    fn = F.mse_loss if kind == "mse" else F.l1_loss
    g = torch.Generator().manual_seed(sum(shape))
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = fn(ad, bd)
    (want * 0.7).backward()
    x, t = a.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    got = mod(x, t)
    value, want = float(got.detach()), float(want.detach())
    assert got.dim() == 0 and type(got.grad_fn).__name__ == "_MeanBackward"
    assert abs(value - want) <= 1e-6 * want
    (got * 0.7).backward()
    assert torch.allclose(x.grad.cpu().double(), ad.grad, rtol=1e-5, atol=1e-9)
    assert torch.allclose(t.grad.cpu().double(), bd.grad, rtol=1e-5, atol=1e-9)
    assert torch.equal(mod(x, t).detach(), got.detach())
    # the target without a gradient: none is formed
    x2, t2 = a.to(device).requires_grad_(True), b.to(device)
    mod(x2, t2).backward()
    assert t2.grad is None and torch.allclose(x2.grad.cpu().double() * 0.7, ad.grad, rtol=1e-5, atol=1e-9)
    # the plain expression: float64, and when nothing requires grad
    x64, t64 = a.to(device).double().requires_grad_(True), b.to(device).double()
    p = mod(x64, t64)
    assert p.dtype == torch.float64 and type(p.grad_fn).__name__ != "_MeanBackward" and torch.equal(p, fn(x64, t64))
    q = mod(a.to(device), b.to(device))
    assert q.grad_fn is None and torch.equal(q, fn(a.to(device), b.to(device)))
    with torch.no_grad():
        assert torch.equal(mod(x, t), fn(x, t))


@pytest.fixture(scope="module")
def vgg_state():
    return LR.vgg16_state(7)


@pytest.fixture(scope="module")
def vgg_node(vgg_state, device):
    return vgg.VGG(weights=vgg_state).to(device)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", [(8, 8), (8, 40), (24, 16), (32, 32)])
def test_vgg_node_against_float64(h, w, b, vgg_state, vgg_node, device):
    g = torch.Generator().manual_seed(h * 100 + w + b)
    out, gt = torch.rand((b, 3, h, w), generator=g), torch.rand((b, 3, h, w), generator=g)
    x, t = out.to(device).requires_grad_(True), gt.to(device).requires_grad_(True)
    got = vgg_node(x, t)
    assert got.dim() == 0 and type(got.grad_fn).__name__ == "_VGGFunctionBackward"
    (got * 0.7).backward()
    got = got.detach()
    assert t.grad is None and all(p.grad is None for p in vgg_node.parameters())
    dec = LR.vgg_decisions(vgg_node, torch.cat([x.detach(), t.detach()], 0))
    assert len(dec) == 9 and all(0 < float(m.float().mean()) < 1 for m, _ in dec)        # every layer is alive and masked
    res = {}
    for dtype in (torch.float64, torch.float32):
        o = out.clone().to(dtype).requires_grad_(True)
        loss = LR.vgg_loss_pinned(vgg_state, o, gt.to(dtype), dec)
        (loss * 0.7).backward()
        res[dtype] = (float(loss.detach()), o.grad)
    want, gwant = res[torch.float64]
    e_loss, e_grad = abs(float(got) - want) / want, _rel(x.grad.cpu(), gwant)
    e32_loss, e32_grad = abs(res[torch.float32][0] - want) / want, _rel(res[torch.float32][1], gwant)
    print(f"VGG {b}x3x{h}x{w}: loss {float(got):.6e}, rel err {e_loss:.2e} (fp32 torch-CPU {e32_loss:.2e}); "
          f"image gradient rel L2 {e_grad:.2e} (fp32 torch-CPU {e32_grad:.2e})")
    assert want > 0 and float(gwant.norm()) > 0
    assert e_loss <= 2e-4
    assert e_grad <= max(2e-4, 4 * e32_grad)
    # the same bits on a second run
    x2 = out.to(device).requires_grad_(True)
    again = vgg_node(x2, gt.to(device))
    again.backward()
    assert torch.equal(again.detach(), got.detach())
    x3 = out.to(device).requires_grad_(True)
    vgg_node(x3, gt.to(device)).backward()
    assert torch.equal(x3.grad, x2.grad)
    # callers that do not backpropagate see no graph, and the same value
    plain = vgg_node(out.to(device), gt.to(device))
    assert plain.grad_fn is None and torch.equal(plain, got.detach())
    with torch.no_grad():
        assert vgg_node(x, t).grad_fn is None


def test_vgg_node_other_faces(vgg_state, vgg_node, device):
    with pytest.raises(ValueError, match="multiples of 8"):
        vgg_node(torch.zeros((1, 3, 12, 20), device=device, requires_grad=True), torch.zeros((1, 3, 12, 20), device=device))
    # float64 on the device: the plain torch restatement of the table
    g = torch.Generator().manual_seed(2)
    out, gt = torch.rand((1, 3, 16, 8), generator=g, dtype=torch.float64), torch.rand((1, 3, 16, 8), generator=g, dtype=torch.float64)
    seq = LR.vgg_sequential(vgg_state, torch.float64)
    with torch.no_grad():
        want = F.mse_loss(seq(out), seq(gt))
    got = vgg_node(out.to(device).requires_grad_(True), gt.to(device))
    assert got.dtype == torch.float64 and type(got.grad_fn).__name__ != "_VGGFunctionBackward"
    got = got.detach()
    assert abs(float(got) - float(want)) <= 1e-9 * float(want)
    # the packs are made once
    assert vgg_node.packed() is vgg_node.packed() and vgg_node.packed_transposed() is vgg_node.packed_transposed()


def _model(sd, device):
    model = Model(types.SimpleNamespace(model="vfi_amd.adacof.models.adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    model.load(sd)
    model.train(True)
    return model


def test_loss_on_the_network(vgg_state, device):
    sd = nets_cpu.adacofnet_random_state_dict(9, kernel_size=5)
    g = torch.Generator().manual_seed(4)
    f0, f1, f2 = (torch.rand((2, 3, 64, 64), generator=g).to(device) for _ in range(3))
    # the default loss: the expression tests/test_adacofnet_backward_gpu.py writes by hand, bit for bit
    by_hand = _model(sd, device)
    out = by_hand(f0, f2)
    want = utility.Module_CharbonnierLoss()(out["frame1"], f1) + 0.01 * out["g_Spatial"] + 0.005 * out["g_Occlusion"]
    want.backward()
    model = _model(sd, device)
    crit = losses.Loss(types.SimpleNamespace(loss=DEFAULT, gpu_id=0))
    got = crit(model(f0, f2), f1, [f0, f2])
    got.backward()
    assert torch.equal(got.detach(), want.detach())
    named = dict(by_hand.named_parameters())
    assert len(named) == 118
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, named[k].grad), k
    # more terms: the sum of the parts computed separately, in the reference's order
    crit = losses.Loss(types.SimpleNamespace(loss=DEFAULT + '+0.1*VGG+1*MSE+1*L1', vgg_weights=vgg_state, gpu_id=0))
    assert [l['type'] for l in crit.loss] == ['Charb', 'VGG', 'MSE', 'L1'] and crit.loss_module[1].vgg16_conv_4_3[0].weight.device == device
    model.zero_grad(set_to_none=True)
    out = model(f0, f2)
    got = crit(out, f1, [f0, f2])
    frame = out["frame1"].detach().requires_grad_(True)
    parts = [1.0 * utility.Module_CharbonnierLoss()(frame, f1), 0.1 * crit.loss_module[1](frame, f1),
             1.0 * losses.Module_MSELoss()(frame, f1), 1.0 * losses.Module_L1Loss()(frame, f1),
             0.01 * out["g_Spatial"].detach(), 0.005 * out["g_Occlusion"].detach()]
    assert torch.equal(got.detach(), sum(parts).detach())
    got.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert all(p.grad is None for p in crit.parameters())
