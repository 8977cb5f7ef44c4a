"""AdaCoFNet training on the MI355X: the HIP backward of the plain AdaCoF network against float64
autograd of its restatement (tests/adacofnet_grad_ref.py), every new ABI entry alone, determinism, the train / eval
contract, the packed-weight cache after an optimiser step, and a short training run with the reference's default loss
(src/adacof/train.py:31) and optimiser (Adamax, lr 1e-3).

Tolerance of the parameter gradients: relative L2 2e-4 per tensor (the project's, section 12); a tensor may exceed it only up
to 4 x the error float32 torch-CPU autograd of the same pinned restatement makes against the float64 one -- the test
measures that error itself (the factor 4: reduction order over 512-channel layers)."""
import types

import pytest
import torch
import torch.nn.functional as F

import adacofnet_grad_ref as R
from oracle import nets_cpu, synth
from vfi_amd import ops
from vfi_amd.adacof import utility
from vfi_amd.adacof.models import Model
from vfi_amd.adacof.models.adacofnet import AdaCoFNet, KernelEstimation

pytestmark = pytest.mark.gpu

HEADS = R.HEADS
LOSS_W = (1.0, 0.01, 0.005)          # 1*Charb + 0.01*g_Spatial + 0.005*g_Occlusion


def _args(ks=5, dil=1):
    return types.SimpleNamespace(kernel_size=ks, dilation=dil, gpu_id=0)


def _state(seed, ks=5, other=False):
    """Seeded weights (tests/trained_stats.py has no statistics for this net: its trained checkpoint is not in the
    reference snapshot); `other` draws a second set."""
    return nets_cpu.adacofnet_random_state_dict(seed + (100 if other else 0), kernel_size=ks)


def _net(sd, device, ks=5, dil=1):
    net = AdaCoFNet(_args(ks, dil)).to(device)
    net.load_state_dict(sd)
    return net


def _frames(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, h, w), generator=g), torch.rand((n, 3, h, w), generator=g)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _loss(out, g, ws):
    return ws[0] * (out["frame1"] * g.to(out["frame1"])).sum() + ws[1] * out["g_Spatial"] + ws[2] * out["g_Occlusion"]


def _hip_grads(net, f0, f2, g, ws, device):
    net.train(True)
    net.zero_grad(set_to_none=True)
    out = net(f0.to(device), f2.to(device))
    _loss(out, g.to(device), ws).backward()
    return out, {k: p.grad for k, p in net.named_parameters()}


def _decisions(net, f0, f2, device):
    """The product's fp32 forward, op by op (KernelEstimation.forward_train keeps every op's output): every ReLU mask and
    the four offset maps whose truncation picks the sampler's integer cells."""
    with torch.no_grad():
        _, _, x6 = ops.adacof_prepare(f0.to(device).contiguous(), f2.to(device).contiguous(), rgbx=False)
        keep = {}
        outs = net.get_kernel.forward_train(x6, keep)
    masks = {}
    for i in range(1, 6):
        for j, idx in enumerate((0, 2, 4)):
            masks[f"moduleConv{i}.{idx}"] = keep["enc"][i][j + 1]
            if i >= 2:
                masks[f"moduleDeconv{i}.{idx}"] = keep["dec"][i][j + 1]
        if i >= 2:
            masks[f"moduleUpsample{i}.1"] = keep["up"][i][1]
    for i, h in enumerate(HEADS):
        m, t, _ = keep["heads"][h]
        masks[f"{h}.0"], masks[f"{h}.2"], masks[f"{h}.4"] = keep["h0"][:, 64 * i:64 * (i + 1)], m, t
    return {k: (v > 0).cpu() for k, v in masks.items()}, tuple(outs[i].cpu() for i in (1, 2, 4, 5))


def _ref_grads(sd, f0, f2, g, ws, ks, dil, masks, offsets, dtype):
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    mk = {k: v.to(dtype) for k, v in masks.items()} if masks is not None else None
    out, _ = R.training_dict(P, f0.to(dtype), f2.to(dtype), ks, dil, masks=mk, offsets=offsets)
    _loss(out, g.to(dtype), ws).backward()
    return out, {k: v.grad for k, v in P.items()}


def _check_all(pg, r64, r32):
    worst = (0.0, None)
    assert len(r64) == 118
    for k, want in r64.items():
        assert pg[k] is not None, k
        err = _rel(pg[k].cpu(), want)
        bound = max(2e-4, 4 * _rel(r32[k], want))
        worst = max(worst, (err, k))
        assert err <= bound, (k, err, bound)
    print(f"worst per-tensor relative L2 {worst[0]:.3e} ({worst[1]})")


CASES = [  # (n, h, w, kernel_size, dilation, second weight set, loss weights)
    (2, 32, 32, 5, 1, False, LOSS_W),        # 1x1 bottleneck: the upsample adjoint at h = w = 1
    (2, 64, 96, 5, 1, True, LOSS_W),
    (1, 40, 50, 5, 1, False, LOSS_W),        # reflect-padded to 64x64, frame1 cropped: zero gradient in the pad
    (1, 64, 64, 3, 2, True, LOSS_W),
    (1, 40, 50, 5, 1, True, (1.0, 0.0, 0.0)),    # each of the three outputs alone
    (1, 64, 64, 5, 1, False, (0.0, 1.0, 0.0)),
    (1, 64, 64, 5, 1, False, (0.0, 0.0, 1.0)),
]


@pytest.mark.parametrize("n,h,w,ks,dil,other,ws", CASES)
def test_gradients_match_pinned_float64_reference(n, h, w, ks, dil, other, ws, device):
    sd = _state(3, ks, other)
    net = _net(sd, device, ks, dil)
    f0, f2 = _frames(11, n, h, w)
    g = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(5))
    out, pg = _hip_grads(net, f0, f2, g, ws, device)
    assert out["frame1"].shape == (n, 3, h, w) and out["g_Spatial"].dim() == 0 and out["g_Occlusion"].dim() == 0
    masks, offsets = _decisions(net, f0, f2, device)
    o64, r64 = _ref_grads(sd, f0, f2, g, ws, ks, dil, masks, offsets, torch.float64)
    _, r32 = _ref_grads(sd, f0, f2, g, ws, ks, dil, masks, offsets, torch.float32)
    assert float((out["frame1"].detach().cpu().double() - o64["frame1"].detach()).abs().max()) <= 2e-5
    for k in ("g_Spatial", "g_Occlusion"):
        assert abs(float(out[k].detach()) - float(o64[k].detach())) <= 1e-5 * max(1.0, abs(float(o64[k].detach()))), k
    _check_all(pg, r64, r32)


def test_gradients_agree_with_free_running_oracle(device):
    sd = _state(7)
    net = _net(sd, device)
    f0, f2 = _frames(2, 2, 64, 96)
    g = torch.randn((2, 3, 64, 96), generator=torch.Generator().manual_seed(1))
    _, pg = _hip_grads(net, f0, f2, g, LOSS_W, device)
    _, ref = _ref_grads(sd, f0, f2, g, LOSS_W, 5, 1, None, None, torch.float64)
    for k, want in ref.items():
        cos = float(F.cosine_similarity(pg[k].cpu().double().flatten(), want.flatten(), dim=0))
        assert cos >= 0.9999, (k, cos)


def test_backward_is_deterministic_and_eval_is_the_inference_path(device):
    sd = _state(4)
    net = _net(sd, device)
    f0, f2 = _frames(3, 2, 40, 50)
    g = torch.randn((2, 3, 40, 50), generator=torch.Generator().manual_seed(2))
    o1, p1 = _hip_grads(net, f0, f2, g, LOSS_W, device)
    o2, p2 = _hip_grads(net, f0, f2, g, LOSS_W, device)
    assert o1["frame1"].grad_fn is not None
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k
    for k in o1:
        assert torch.equal(o1[k].detach(), o2[k].detach()), k
    net.eval()
    e = net(f0.to(device), f2.to(device))            # grad mode on, parameters requiring grad: still no graph
    assert isinstance(e, torch.Tensor) and e.grad_fn is None and not e.requires_grad
    with torch.no_grad():
        e0 = net(f0.to(device), f2.to(device))
    assert torch.equal(e, e0)
    assert float((o1["frame1"].detach() - e).abs().max()) <= 2e-5


def test_only_the_occlusion_head_requires_grad(device):
    sd = _state(6)
    net = _net(sd, device)
    for k, p in net.named_parameters():
        p.requires_grad_("moduleOcclusion" in k)
    f0, f2 = _frames(1, 1, 64, 64)
    g = torch.randn((1, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    _, pg = _hip_grads(net, f0, f2, g, LOSS_W, device)
    masks, offsets = _decisions(net, f0, f2, device)
    _, r64 = _ref_grads(sd, f0, f2, g, LOSS_W, 5, 1, masks, offsets, torch.float64)
    for k, got in pg.items():
        if "moduleOcclusion" in k:
            assert _rel(got.cpu(), r64[k]) <= 2e-4, (k, _rel(got.cpu(), r64[k]))
        else:
            assert got is None, k


def test_kernel_estimation_and_model_train_on_their_own(device):
    sd = _state(9)
    model = Model(types.SimpleNamespace(model="vfi_amd.adacof.models.adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    model.load(sd)
    model.train(True)
    f0, f2 = _frames(4, 1, 64, 64)
    r0, r2 = (utility.moduleNormalize(f.to(device)) for f in (f0, f2))
    outs = model.get_kernel(r0, r2)
    gs = [torch.randn(o.shape, generator=torch.Generator().manual_seed(i)) for i, o in enumerate(outs)]
    sum((o * g.to(device)).sum() for o, g in zip(outs, gs)).backward()
    P = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    masks, _ = _decisions(model.model, f0, f2, device)
    mean = torch.tensor(nets_cpu.CHANNEL_MEANS, dtype=torch.float64).view(1, 3, 1, 1)
    x6 = torch.cat([f0.double() - mean, f2.double() - mean], 1)
    ref = R.kernel_estimation(P, x6, {k: v.double() for k, v in masks.items()})
    sum((o * g.double()).sum() for o, g in zip(ref, gs)).backward()
    for (k, p) in model.model.named_parameters():
        assert _rel(p.grad.cpu(), P[k].grad) <= 2e-4, (k, _rel(p.grad.cpu(), P[k].grad))
    est = KernelEstimation(5).to(device)
    est.eval()
    assert all(o.grad_fn is None for o in est(r0, r2))


def test_packed_cache_follows_optimiser_step(device):
    sd = _state(8)
    net = _net(sd, device)
    f0, f2 = (f.to(device) for f in _frames(4, 2, 64, 64))
    net.train(True)
    opt = torch.optim.Adamax(net.parameters(), lr=1e-2)
    out = net(f0, f2)
    (utility.Module_CharbonnierLoss()(out["frame1"], f0) + 0.01 * out["g_Spatial"] + 0.005 * out["g_Occlusion"]).backward()
    opt.step()
    net.eval()
    with torch.no_grad():
        got = net(f0, f2)
        fresh = _net(net.state_dict(), device)
        want = fresh(f0, f2)
        old = _net(sd, device)(f0, f2)
    assert torch.equal(got, want) and not torch.equal(got, old)


# ---- each new entry point alone, against float64 --------------------------------------------------------------------
def _up(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (2, 3), (5, 9), (16, 16), (3, 64)])
def test_upsample2x_backward(h, w, device):
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((2, 3, h, w), generator=g).round(decimals=1)
    x[0, 0, 0, 0] = 0.0
    gy = torch.randn((2, 3, 2 * h, 2 * w), generator=g)
    xd = x.double().requires_grad_(True)
    (_up(torch.relu(xd)) * gy.double()).sum().backward()
    got = ops.upsample2x_backward(gy.to(device), mask_src=torch.relu(x).to(device))
    assert torch.allclose(got.cpu().double(), xd.grad, rtol=1e-5, atol=1e-6)
    assert got[0, 0, 0, 0] == 0
    xd.grad = None
    (_up(xd) * gy.double()).sum().backward()
    got = ops.upsample2x_backward(gy.to(device))
    assert torch.allclose(got.cpu().double(), xd.grad, rtol=1e-5, atol=1e-6)
    # the forward it is the adjoint of is the product's own resize.  That kernel forms the source coordinate as the float
    # product o * (n-1)/(2n-1), off by at most 2^-23 (n-1) per axis, so each of an output's four tap weights is off by at most
    # twice that: |<fwd, g> - <x, adj>| <= 8 * 2^-23 * max(h, w) * max|x| * sum|g| (plus the sums' own fp32 rounding)
    fwd = ops.resize_bilinear(x.to(device), (2 * h, 2 * w), align_corners=True)
    lhs, rhs = float((fwd.double() * gy.to(device).double()).sum()), float((x.to(device).double() * got.double()).sum())
    bound = 8 * 2.0 ** -23 * max(h, w) * float(x.abs().max()) * float(gy.abs().sum())
    print(f"adjoint identity {h}x{w}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound + 1e-6 * float((fwd.abs().double().cpu() * gy.abs().double()).sum())


@pytest.mark.parametrize("h,w", [(2, 2), (6, 10), (8, 12)])
def test_pool2_avg_backward_and_relu_mask_on_channel_slices(h, w, device):
    g = torch.Generator().manual_seed(h + w)
    big = torch.relu(torch.randn((2, 9, h, w), generator=g)).round(decimals=1)
    gkb = torch.randn((2, 7, h, w), generator=g)
    y, gk = big[:, 2:7], gkb[:, 1:6]                      # batch stride != C*H*W
    gp = torch.randn((2, 5, h // 2, w // 2), generator=g)
    yd = y.double().requires_grad_(True)
    s = torch.relu(yd)
    ((F.avg_pool2d(s, 2, 2) * gp.double()).sum() + (s * gk.double()).sum()).backward()
    got = ops.pool2_avg_backward(big.to(device)[:, 2:7], gp.to(device), gkb.to(device)[:, 1:6])
    assert torch.allclose(got.cpu().double(), yd.grad, atol=1e-6)
    assert (got.cpu()[y == 0] == 0).all() and (y == 0).any()
    no_skip = ops.pool2_avg_backward(big.to(device)[:, 2:7], gp.to(device))
    assert torch.allclose(no_skip.cpu().double(), 0.25 * gp.double().repeat_interleave(2, 2).repeat_interleave(2, 3) * (y > 0), atol=1e-6)
    # relu mask: in place on a slice, with and without the addend, and out of place
    gb = gkb.to(device).clone()
    ops.relu_mask_(gb[:, 1:6], big.to(device)[:, 2:7], addend=got)
    assert torch.equal(gb[:, 1:6].cpu(), ((gk + got.cpu()) * (y > 0)))
    assert torch.equal(gb[:, :1].cpu(), gkb[:, :1]) and torch.equal(gb[:, 6:].cpu(), gkb[:, 6:])
    out = ops.relu_mask_(gkb.to(device)[:, 1:6], big.to(device)[:, 2:7], out=torch.empty((2, 5, h, w), device=device))
    assert torch.equal(out.cpu(), gk * (y > 0))
    assert torch.equal(ops.add(big.to(device)[:, 2:7], gkb.to(device)[:, 1:6]).cpu(), y + gk)
    # the 4-byte path (bases 4 bytes off 16-byte alignment) and the 16-byte path (dense copies) give the same bits
    def off(t):
        v = torch.empty(t.numel() + 1, device=device)[1:].view(t.shape)
        assert v.data_ptr() % 16 != 0
        return v.copy_(t)
    a, b, c = gkb.to(device)[:, 1:6].contiguous(), big.to(device)[:, 2:7].contiguous(), got.contiguous()
    assert a[0].numel() % 4 == 0 and torch.equal(ops.add(off(a), off(b)), ops.add(a, b))
    assert torch.equal(ops.relu_mask_(off(a), off(b), addend=off(c)), ops.relu_mask_(a.clone(), b, addend=c))


@pytest.mark.parametrize("n,f,h,w,h0,w0", [(2, 3, 6, 7, 6, 7), (1, 5, 32, 32, 20, 27), (2, 5, 33, 65, 33, 65)])
def test_head_entries_match_float64(n, f, h, w, h0, w0, device):
    gen = torch.Generator().manual_seed(n * f + h)
    r = lambda *s: torch.randn(s, generator=gen)
    f2 = f * f
    maps = [torch.softmax(r(n, f2, h, w) * 2, 1), r(n, f2, h, w) * 3, r(n, f2, h, w) * 3,
            torch.softmax(r(n, f2, h, w) * 2, 1), r(n, f2, h, w) * 3, r(n, f2, h, w) * 3, torch.sigmoid(r(n, 1, h, w))]
    dm = [t.to(device).contiguous() for t in maps]
    m, terms = ops.adacof_smooth_forward(*dm)
    hm, hs, ho = R.smooth_forward(*(t.double().numpy() for t in maps))
    assert torch.allclose(m.cpu().double(), torch.from_numpy(hm), rtol=1e-5, atol=1e-6)
    assert abs(float(terms[0]) - hs) <= 1e-5 * hs and abs(float(terms[1]) - ho) <= 1e-5 * ho
    assert torch.equal(ops.adacof_smooth_forward(*dm)[1], terms)
    up_s, up_o = torch.tensor(0.01, device=device), torch.tensor(0.005, device=device)
    t1, t2, g = r(n, 3, h, w), r(n, 3, h, w), r(n, 3, h0, w0)
    got = ops.adacof_blend_backward(g.to(device), t1.to(device), t2.to(device), dm[6], up_o)
    want = R.blend_backward(g.double().numpy(), t1.double().numpy(), t2.double().numpy(), maps[6].double().numpy(), 0.005)
    for a, b in zip(got, want):
        assert torch.allclose(a.cpu().double(), torch.from_numpy(b), rtol=1e-4, atol=1e-6)
    gw, ga, gb = r(n, f2, h, w), r(n, f2, h, w), r(n, f2, h, w)
    for s in (0, 1):
        w_, a_, b_ = maps[3 * s:3 * s + 3]
        got = ops.adacof_head_backward(gw.to(device), ga.to(device), gb.to(device), *dm[3 * s:3 * s + 3],
                                       m[:, 2 * s:2 * s + 1], m[:, 2 * s + 1:2 * s + 2], up_s)
        want = R.head_backward(*(t.double().numpy() for t in (gw, ga, gb, w_, a_, b_)), hm[:, 2 * s:2 * s + 1],
                               hm[:, 2 * s + 1:2 * s + 2], 0.01)
        for a, b in zip(got, want):
            assert torch.allclose(a.cpu().double(), torch.from_numpy(b), rtol=1e-4, atol=2e-6)
    gl, ga0, _ = ops.adacof_head_backward(gw.to(device), ga.to(device), gb.to(device), *dm[:3])     # no smoothness term
    assert torch.equal(ga0.cpu(), ga)
    assert torch.allclose(gl.cpu().double(), torch.from_numpy(R.softmax_backward(maps[0].double().numpy(), gw.double().numpy())),
                          rtol=1e-4, atol=1e-6)
    occ = dm[6]
    assert torch.allclose(ops.sigmoid_backward(occ, occ).cpu(), maps[6] * maps[6] * (1 - maps[6]), rtol=1e-6, atol=1e-7)
    pad = ops.replicate_pad(dm[1], 2)
    assert torch.equal(pad.cpu(), F.pad(maps[1], (2,) * 4, mode="replicate"))


@pytest.mark.parametrize("shape", [(2, 3, 40, 50), (1, 3, 7, 9), (3, 1, 1, 5)])
def test_charbonnier_loss_node(shape, device):
    g = torch.Generator().manual_seed(sum(shape))
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = torch.sqrt((ad - bd) ** 2 + 0.001 ** 2).mean()
    (want * 0.7).backward()
    x, t = a.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    got = utility.Module_CharbonnierLoss()(x, t)
    assert got.dim() == 0 and abs(float(got) - float(want)) <= 1e-6 * float(want)
    (got * 0.7).backward()
    assert torch.allclose(x.grad.cpu().double(), ad.grad, rtol=1e-5, atol=1e-9)
    assert torch.allclose(t.grad.cpu().double(), bd.grad, rtol=1e-5, atol=1e-9)
    again = utility.Module_CharbonnierLoss()(x, t)
    assert torch.equal(again.detach(), got.detach())
    f = utility.CharbonnierFunc(x - t)
    assert abs(float(f) - float(want)) <= 1e-6 * float(want)


def test_heads_bank_weight_gradient_equals_seven_calls(device):
    """The shared 64 -> 448 first convolution: one weight-gradient call on the concatenated gradient, split, equals the
    seven heads' own calls bit for bit when they sum the same number of partial slabs."""
    g = torch.Generator().manual_seed(0)
    n, h, w = 2, 32, 48
    x = torch.randn((n, 64, h, w), generator=g).to(device)
    dy = torch.randn((n, 448, h, w), generator=g).to(device)
    splits = ops.conv2d_backward_weight_splits(n, 64, h, w, 448, 3)
    assert splits != ops.conv2d_backward_weight_splits(n, 64, h, w, 64, 3)      # a shape where the default counts differ
    dw, db = ops.conv2d_backward_weight(x, dy, 3, "zeros", bias=True)
    for i in range(7):
        dwi, dbi = ops.conv2d_backward_weight(x, dy[:, 64 * i:64 * (i + 1)], 3, "zeros", bias=True, max_splits=splits)
        assert torch.equal(dwi, dw[64 * i:64 * (i + 1)]) and torch.equal(dbi, db[64 * i:64 * (i + 1)]), i


# ---- a short training run with the reference's default loss and optimiser -------------------------------------------
def _run(forward, params, batch, target, steps):
    opt = torch.optim.Adamax(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    crit = utility.Module_CharbonnierLoss()
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        out = forward(*batch)
        loss = LOSS_W[0] * crit(out["frame1"], target) + LOSS_W[1] * out["g_Spatial"] + LOSS_W[2] * out["g_Occlusion"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_training_run(device):
    sd = _state(12)
    trip = [synth.translating_pair(s, 64, 64) for s in range(4)]
    f0, f1, f2 = (torch.stack([torch.from_numpy(t[i]).reshape(3, 64, 64) for t in trip]).float() for i in range(3))
    net = _net(sd, device)
    net.train(True)
    gpu = _run(net, list(net.parameters()), (f0.to(device), f2.to(device)), f1.to(device), 30)
    assert gpu[-1] < gpu[0], gpu
    P = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    cpu = _run(lambda a, b: R.training_dict(P, a, b)[0], list(P.values()), (f0.double(), f2.double()), f1.double(), 5)
    for a, b in zip(gpu[:5], cpu):
        assert abs(a - b) <= 0.02 * abs(b), (gpu[:5], cpu)
