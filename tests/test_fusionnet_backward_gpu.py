"""FusionNet training on the MI355X: the HIP backward of FusionNet.forward against float64
references, the new ABI entries in isolation, determinism, the packed-weight cache after an optimiser step, and a
short training run mirroring the reference's loop (src/fusion_net/train.py, trainer.py:222-260)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nets_cpu
from vfi_amd import ops
from vfi_amd.fusion_net.fusion_net import FusionNet

pytestmark = pytest.mark.gpu

LIVE = [f"encoder_layers.{i}" for i in range(3)] + ["bottleneck_layer"] + [f"decoder_layers.{i}" for i in range(3)]
IN_NAMES = ("base", "adacof", "phase", "other", "maps")


def _state(seed, maps, trained=False):
    if not trained:
        return nets_cpu.fusionnet_random_state_dict(seed, uncertainty_maps=maps)
    import trained_stats     # the statistics are those of the 18-channel checkpoint: drop the maps' input channels
    sd = trained_stats.state_dict_like_trained("fusionnet", nets_cpu.fusionnet_random_state_dict(seed), seed=seed + 1)
    cin = 15 + maps
    return {k: (v[:, :cin].contiguous() if k in ("net.0.weight", "encoder_layers.0.weight") else v) for k, v in sd.items()}


def _inputs(seed, n, h, w, maps):
    g = torch.Generator().manual_seed(seed)
    r = lambda c: torch.rand((n, c, h, w), generator=g)
    return [r(3), r(3), r(3), r(6), r(maps) if maps else None]


def _net(sd, device, maps):
    net = FusionNet(uncertainty_maps=maps).to(device)
    net.load_state_dict(sd)
    return net


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ---- the reference: today's forward replayed op by op, decisions pinned, float64 autograd -------------------------
def _replay(net, ins, variant):
    """fp32 intermediates of the product's own kernels (ops.*): post-ReLU encoder outputs, bottleneck / decoder outputs,
    and the head's pre-clamp sum."""
    p = net.packed()
    parts = [t for t in ins if t is not None]
    x = torch.cat([t.contiguous() for t in parts], 1).contiguous()
    skips = []
    for i in range(3):
        s, x = ops.conv2d_pool2(x, p["enc"][i], True, "reflect", "relu")
        skips.append(s)
    x = ops.conv2d(x, p["mid"], "reflect", None)
    srcs = [x]
    for i, s in enumerate(skips[::-1]):
        x = ops.resize_bilinear(x, s.shape[2:], align_corners=False, relu_input=True, residual=s)
        x = ops.conv2d(x, p["dec"][i], "reflect", None)
        srcs.append(x)
    hb = ins[2] if variant == 1 else ins[0]
    pre = hb + torch.tanh(srcs[-1])          # recomputed exactly as the kernel: base + tanhf(x)
    out = ops.tanh_residual_clamp(srcs[-1].contiguous(), hb.contiguous())
    clamp_mask = (out == pre) | ((pre >= 0) & (pre <= 1))
    return [s.cpu() for s in skips], [s.cpu() for s in srcs], clamp_mask.cpu(), out.cpu()


def _pinned_grads(sd, ins, variant, grad_out, skips, srcs, clamp_mask):
    """float64 autograd through the oracle's layers with every ReLU mask, pool argmax and clamp mask taken from the
    product's fp32 intermediates."""
    P = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if k.split(".")[0] != "net"}
    X = [t.double().clone().requires_grad_(True) if t is not None else None for t in ins]
    x = torch.cat([t for t in X if t is not None], 1)

    def conv(name, x):
        k = P[name + ".weight"].shape[-1]
        return F.conv2d(F.pad(x, ((k - 1) // 2,) * 4, mode="reflect") if k > 1 else x, P[name + ".weight"], P[name + ".bias"])

    sk = []
    for i in range(3):
        s = conv(LIVE[i], x) * (skips[i] > 0)
        sk.append(s)
        _, idx = F.max_pool2d(skips[i], 2, 2, return_indices=True)
        x = s.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    x = conv(LIVE[3], x)
    for i, s in enumerate(sk[::-1]):
        x = F.interpolate(x * (srcs[i] > 0), scale_factor=2, mode="bilinear", align_corners=False) + s
        x = conv(LIVE[4 + i], x)
    hb = X[2] if variant == 1 else X[0]
    out = (hb + torch.tanh(x)) * clamp_mask
    (out * grad_out.double()).sum().backward()
    return {k: v.grad for k, v in P.items()}, [t.grad if t is not None else None for t in X]


def _hip_grads(net, ins, variant, grad_out, device):
    net.train(True)
    net.zero_grad(set_to_none=True)
    X = [t.to(device).requires_grad_(True) if t is not None else None for t in ins]
    out = net(*X, variant=variant)
    out.backward(grad_out.to(device))
    named = dict(net.named_parameters())
    return out, {k: named[k].grad for k in named if k.split(".")[0] != "net"}, [t.grad if t is not None else None for t in X]


CASES = [  # (n, h, w, variant, maps, trained)
    (2, 64, 64, 0, 3, False),
    (2, 64, 64, 1, 0, True),
    (1, 40, 72, 1, 3, False),
    (1, 40, 72, 0, 0, True),
    (2, 96, 160, 0, 3, True),
    (2, 96, 160, 1, 0, False),
    (16, 256, 256, 0, 0, True),
]


@pytest.mark.parametrize("n,h,w,variant,maps,trained", CASES)
def test_gradients_match_pinned_float64_reference(n, h, w, variant, maps, trained, device):
    sd = _state(3, maps, trained)
    net = _net(sd, device, maps)
    ins = _inputs(11, n, h, w, maps)
    g = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(5))
    out, pg, ig = _hip_grads(net, ins, variant, g, device)
    net.eval()
    with torch.no_grad():
        skips, srcs, cm, ref_out = _replay(net, [t.to(device) if t is not None else None for t in ins], variant)
    assert torch.equal(out.detach().cpu(), ref_out)
    rp, ri = _pinned_grads(sd, ins, variant, g, skips, srcs, cm)
    for k in rp:
        assert pg[k] is not None, k
        assert _rel(pg[k].cpu(), rp[k]) <= 2e-4, (k, _rel(pg[k].cpu(), rp[k]))
    for name, a, b in zip(IN_NAMES, ig, ri):
        if b is None:
            assert a is None
            continue
        assert _rel(a.cpu(), b) <= 2e-4, (name, _rel(a.cpu(), b))
    assert all(p.grad is None for k, p in net.named_parameters() if k.startswith("net."))


@pytest.mark.parametrize("variant,maps", [(0, 3), (1, 0)])
def test_gradients_agree_with_free_running_oracle(variant, maps, device):
    sd = _state(7, maps)
    net = _net(sd, device, maps)
    ins = _inputs(2, 2, 64, 64, maps)
    g = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(1))
    _, pg, ig = _hip_grads(net, ins, variant, g, device)
    P = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    X = [t.double().clone().requires_grad_(True) if t is not None else None for t in ins]
    (nets_cpu.fusionnet_forward(P, *X, variant) * g.double()).sum().backward()
    cos = lambda a, b: float(F.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))
    for k in pg:
        assert cos(pg[k].cpu(), P[k].grad) >= 0.9999, k
    for name, a, t in zip(IN_NAMES, ig, X):
        if t is not None:
            assert cos(a.cpu(), t.grad) >= 0.9999, name


def test_backward_is_deterministic_and_output_bitwise_equal_to_no_grad(device):
    sd = _state(4, 3)
    net = _net(sd, device, 3)
    ins = _inputs(3, 2, 96, 160, 3)
    g = torch.randn((2, 3, 96, 160), generator=torch.Generator().manual_seed(2))
    o1, p1, i1 = _hip_grads(net, ins, 0, g, device)
    o2, p2, i2 = _hip_grads(net, ins, 0, g, device)
    assert o1.grad_fn is not None
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k
    for a, b in zip(i1, i2):
        assert torch.equal(a, b)
    with torch.no_grad():
        o0 = net(*(t.to(device) for t in ins), variant=0)
    assert o0.grad_fn is None and torch.equal(o1.detach(), o0)


def test_needs_input_grad_subsets(device):
    sd = _state(6, 0)
    net = _net(sd, device, 0)
    ins = [t.to(device) if t is not None else None for t in _inputs(1, 1, 64, 64, 0)]
    g = torch.randn((1, 3, 64, 64), device=device)
    # eval mode, parameters only: the inference path (no graph) -- training mode records it
    net.eval()
    assert net(*ins).grad_fn is None
    net.train(True)
    net(*ins).backward(g)
    assert all(p.grad is not None for k, p in net.named_parameters() if not k.startswith("net."))
    assert all(t.grad is None for t in ins if t is not None)
    # only `base`, parameters frozen
    for p in net.parameters():
        p.requires_grad_(False)
        p.grad = None
    b = ins[0].clone().requires_grad_(True)
    out = net(b, *ins[1:])
    out.backward(g)
    assert b.grad is not None and b.grad.shape == b.shape
    assert all(p.grad is None for p in net.parameters())
    # the same through the pinned reference
    with torch.no_grad():
        skips, srcs, cm, _ = _replay(net, ins, 0)
    _, ri = _pinned_grads(sd, [t.cpu() if t is not None else None for t in ins], 0, g.cpu(), skips, srcs, cm)
    assert _rel(b.grad.cpu(), ri[0]) <= 2e-4


def test_train_mode_allowed_only_for_fusionnet():
    from vfi_amd.nn_util import PackedModule
    net = FusionNet()
    net.train(True)
    assert net.training
    net.eval()
    with pytest.raises(NotImplementedError):
        PackedModule().train(True)


def test_packed_cache_follows_optimiser_step(device):
    sd = _state(8, 3)
    net = _net(sd, device, 3)
    net.train(True)
    ins = [t.to(device) for t in _inputs(4, 2, 64, 64, 3)]
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-2)
    F.l1_loss(net(*ins), ins[1]).backward()
    opt.step()
    with torch.no_grad():
        got = net(*ins)
        fresh = FusionNet(uncertainty_maps=3).to(device)
        fresh.load_state_dict(net.state_dict())
        _, _, _, want = _replay(fresh, ins, 0)
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(want, _replay(_net(sd, device, 3), ins, 0)[3])


# ---- each new ABI entry against torch float64 on identical fp32 inputs ---------------------------------------------
def _conv_ref(x, w, pad_mode):
    k = w.shape[-1]
    p = (k - 1) // 2
    if p and pad_mode == "reflect":
        return F.conv2d(F.pad(x, (p,) * 4, mode="reflect"), w)
    return F.conv2d(x, w, padding=p)


@pytest.mark.parametrize("n,cin,cout,h,w,ks,pad", [
    (2, 18, 32, 24, 40, 5, "reflect"), (1, 15, 32, 16, 16, 5, "reflect"), (2, 32, 3, 20, 36, 1, "reflect"),
    (1, 64, 128, 8, 8, 3, "reflect"), (1, 128, 128, 5, 9, 3, "reflect"), (2, 128, 64, 10, 18, 5, "reflect"),
    (1, 7, 5, 3, 3, 5, "reflect"), (1, 3, 3, 2, 2, 3, "reflect"), (1, 18, 32, 3, 3, 5, "zeros"),
    (1, 33, 70, 13, 45, 3, "zeros"), (1, 130, 40, 9, 33, 1, "zeros"), (2, 64, 32, 33, 31, 5, "zeros")])
def test_conv_backward_entries_match_float64(n, cin, cout, h, w, ks, pad, device):
    g = torch.Generator().manual_seed(n * 1000 + cin + cout + h)
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, ks, ks), generator=g) * 0.1
    dy = torch.randn((n, cout, h, w), generator=g)
    xd, wd = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    (_conv_ref(xd, wd, pad) * dy.double()).sum().backward()
    dw, db = ops.conv2d_backward_weight(x.to(device), dy.to(device), ks, pad, bias=True)
    dx = ops.conv2d_backward_data(dy.to(device), ops.packed_transposed(wt.to(device)), pad)
    assert _rel(dw.cpu(), wd.grad) <= 2e-5, _rel(dw.cpu(), wd.grad)
    assert _rel(db.cpu(), dy.double().sum((0, 2, 3))) <= 1e-5
    assert _rel(dx.cpu(), xd.grad) <= 2e-5, _rel(dx.cpu(), xd.grad)
    dw2, _ = ops.conv2d_backward_weight(x.to(device), dy.to(device), ks, pad, bias=False)
    assert torch.equal(dw, dw2)


def test_conv_backward_weight_on_channel_slices(device):
    """x and dy as channel slices of wider tensors (batch strides), as FusionNet's concat buffers are."""
    g = torch.Generator().manual_seed(9)
    big = torch.randn((2, 40, 16, 24), generator=g)
    dyb = torch.randn((2, 50, 16, 24), generator=g)
    x, dy = big[:, 5:23], dyb[:, 10:42]
    xd = x.double().requires_grad_(True)
    wd = torch.zeros((32, 18, 5, 5), dtype=torch.float64, requires_grad=True)
    (_conv_ref(xd, wd, "reflect") * dy.double()).sum().backward()
    dw, _ = ops.conv2d_backward_weight(big.to(device)[:, 5:23], dyb.to(device)[:, 10:42], 5, "reflect")
    assert _rel(dw.cpu(), wd.grad) <= 2e-5


def test_tanh_residual_clamp_backward_saturation(device):
    x = torch.tensor([0.0, 0.5, -0.5, 3.0, -3.0, 0.0, 0.0, 1.0]).view(1, 1, 2, 4)
    base = torch.tensor([0.0, 0.2, 0.9, 0.9, 0.1, 1.0, 1.5, -0.9]).view(1, 1, 2, 4)
    t = torch.tanh(x.double())
    g = torch.linspace(-1, 2, 8).view(1, 1, 2, 4)
    xd, bd = x.double().requires_grad_(True), base.double().requires_grad_(True)
    ((bd + torch.tanh(xd)).clamp(0, 1) * g.double()).sum().backward()
    gx, gb = ops.tanh_residual_clamp_backward(x.to(device), base.to(device), g.to(device))
    fwd = (base + torch.tanh(x))
    m = ((fwd >= 0) & (fwd <= 1)).double()
    assert torch.allclose(gb.cpu().double(), g.double() * m, atol=0)
    assert torch.allclose(gx.cpu().double(), g.double() * (1 - t * t) * m, rtol=1e-6, atol=1e-7)
    assert gb[0, 0, 0, 0] == g[0, 0, 0, 0] and gb[0, 0, 1, 1] == g[0, 0, 1, 1]     # exactly 0 and exactly 1 pass
    assert gb[0, 0, 1, 2] == 0 and gb[0, 0, 1, 3] == 0
    _, gb_only = ops.tanh_residual_clamp_backward(x.to(device), base.to(device), g.to(device), need_x=False)
    assert torch.equal(gb_only, gb)


def test_pool2_max_backward_ties_and_relu(device):
    g = torch.Generator().manual_seed(3)
    y = torch.relu(torch.randn((2, 5, 8, 12), generator=g)).round(decimals=1)
    y[0, 0, 0:2, 0:2] = 0.7                 # four-way positive tie -> top-left
    y[0, 1, 2:4, 2:4] = torch.tensor([[0.1, 0.5], [0.5, 0.2]])   # tie at (0,1) and (1,0) -> (0,1)
    y[1, 2, 4:6, 6:8] = 0.0                 # all zero: routed to top-left, then masked
    gp = torch.randn((2, 5, 4, 6), generator=g)
    gs = torch.randn((2, 5, 8, 12), generator=g)
    yd = y.double().requires_grad_(True)
    s = torch.relu(yd)
    ((F.max_pool2d(s, 2, 2) * gp.double()).sum() + (s * gs.double()).sum()).backward()
    got = ops.pool2_max_backward(y.to(device), gp.to(device), gs.to(device))
    assert torch.allclose(got.cpu().double(), yd.grad, atol=1e-6)
    assert got[0, 0, 0, 0] == gp[0, 0, 0, 0] + gs[0, 0, 0, 0] and got[0, 0, 0, 1] == gs[0, 0, 0, 1]
    assert got[0, 1, 2, 3] == gp[0, 1, 1, 1] + gs[0, 1, 2, 3] and got[0, 1, 3, 2] == gs[0, 1, 3, 2]
    assert (got[1, 2, 4:6, 6:8] == 0).all()
    no_skip = ops.pool2_max_backward(y.to(device), gp.to(device))
    yd.grad = None
    (F.max_pool2d(torch.relu(yd), 2, 2) * gp.double()).sum().backward()
    assert torch.allclose(no_skip.cpu().double(), yd.grad, atol=1e-6)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (4, 4), (5, 9), (32, 32), (3, 64)])
def test_resize_bilinear_backward(h, w, device):
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((2, 3, h, w), generator=g)
    gy = torch.randn((2, 3, 2 * h, 2 * w), generator=g)
    xd = x.double().requires_grad_(True)
    (F.interpolate(torch.relu(xd), scale_factor=2, mode="bilinear", align_corners=False) * gy.double()).sum().backward()
    got = ops.resize_bilinear_backward(x.to(device), gy.to(device), relu_input=True)
    assert torch.allclose(got.cpu().double(), xd.grad, rtol=1e-6, atol=1e-6)
    xd.grad = None
    (F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False) * gy.double()).sum().backward()
    got = ops.resize_bilinear_backward(x.to(device), gy.to(device), relu_input=False)
    assert torch.allclose(got.cpu().double(), xd.grad, rtol=1e-6, atol=1e-6)
    # an exact x2 has coordinates and weights exact in fp32 (0, 1/4, 3/4, 1) and both adjoints add in ascending order:
    # the any-size adjoint gives the same bits
    assert torch.equal(got, ops.resize_bilinear_adjoint(gy.to(device), (h, w)))


# ---- a short training run, mirroring the reference's loop (Adam 1e-4, L1) ------------------------------------------
def _train_losses(forward, params, batches, steps):
    opt = torch.optim.Adam(params, lr=1e-4)
    losses = []
    for i in range(steps):
        ins, target = batches[i % len(batches)]
        opt.zero_grad()
        loss = F.l1_loss(forward(ins), target)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses


def test_training_run(device):
    sd = _state(12, 0)
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(4):
        target = torch.rand((4, 3, 64, 64), generator=g)
        noisy = lambda s: (target + s * torch.randn(target.shape, generator=g)).clamp(0, 1)
        batches.append(([target.clone(), noisy(0.1), noisy(0.1), torch.cat([noisy(0.3), noisy(0.3)], 1), None], target))
    net = _net(sd, device, 0)
    net.train(True)
    on_dev = [([t.to(device) if t is not None else None for t in ins], tgt.to(device)) for ins, tgt in batches]
    gpu = _train_losses(lambda ins: net(*ins), [p for k, p in net.named_parameters() if not k.startswith("net.")], on_dev, 50)
    assert gpu[-1] <= 0.5 * gpu[0], gpu
    P = {k: v.clone().requires_grad_(not k.startswith("net.")) for k, v in sd.items()}
    cpu = _train_losses(lambda ins: nets_cpu.fusionnet_forward(P, *ins, 0), [v for k, v in P.items() if v.requires_grad],
                        batches, 5)
    for a, b in zip(gpu[:5], cpu):
        assert abs(a - b) <= 0.02 * abs(b), (gpu[:5], cpu)
