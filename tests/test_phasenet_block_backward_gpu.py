"""PhaseNet block training on the MI355X, through the public surface: the resize adjoint, the
activation and blend adjoints and the loss nodes against their host models (tests/phasenet_grad_ref.py), the block's
gradients against float64 autograd of its restatement, the train / eval and cache contracts, and one composed level step
with a short Adam run.

Tolerance of the block gradients: relative L2 2e-4 per tensor (the project's, section 12); a tensor may exceed it only up to
4 x the error float32 torch-CPU autograd of the same restatement makes against the float64 one (section 13's rule)."""
import math
import os
import types

import numpy as np
import pytest
import torch

import phasenet_grad_ref as R
import trained_stats
from vfi_amd import _lib, ops
from vfi_amd.phase_net import grad as G
from vfi_amd.phase_net.phase_net import PhaseNetBlock
from vfi_amd.train.loss import get_loss

pytestmark = pytest.mark.gpu

RESIZE_SIZES = [((1, 1), (1, 1)), ((1, 1), (2, 3)), ((2, 3), (3, 4)), ((5, 7), (7, 10)), ((8, 11), (11, 16)),
                ((4, 4), (8, 8)), ((5, 5), (5, 5)), ((9, 13), (4, 5)), ((3, 65), (4, 92)), ((6, 130), (9, 184))]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _misaligned(t):
    """t's values, dense, at a base 4 bytes off 16-byte alignment: the elementwise pass then takes its 4-byte path."""
    v = torch.empty(t.numel() + 1, device=t.device)[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0
    return v.copy_(t)


# ---- resize adjoint --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", RESIZE_SIZES)
def test_resize_adjoint(src, dst, device):
    g = torch.Generator().manual_seed(src[1] * 100 + dst[0])
    x = torch.randn((2, 3) + src, generator=g)
    gy = torch.randn((2, 3) + dst, generator=g)
    xd = x.to(device).requires_grad_(True)
    y = G.resize_bilinear(xd, dst)
    assert y.grad_fn is not None and torch.equal(y.detach(), ops.resize_bilinear(x.to(device), dst, align_corners=False))
    (y * gy.to(device)).sum().backward()
    want = R.resize_adjoint(gy.double().numpy(), src)
    err = _rel(xd.grad, want)
    print(f"resize adjoint {src} -> {dst}: relative L2 against the host model {err:.3e}")
    assert err <= 1e-6
    # adjoint identity against the product's own forward, in fp32
    lhs = float((y.detach().double() * gy.to(device).double()).sum())
    rhs = float((x.to(device).double() * xd.grad.double()).sum())
    scale = float((y.detach().abs().double().cpu() * gy.abs().double()).sum())
    print(f"  adjoint identity |lhs - rhs| / sum|y g| = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-5 * scale
    with torch.no_grad():
        assert G.resize_bilinear(xd, dst).grad_fn is None
    assert G.resize_bilinear(x.to(device), dst).grad_fn is None


def test_resize_adjoint_on_channel_slices(device):
    g = torch.Generator().manual_seed(7)
    big = torch.randn((2, 9, 7, 10), generator=g).to(device)
    out = torch.full((2, 7, 5, 7), 3.0, device=device)
    gy, gx = big[:, 2:5], out[:, 1:4]                       # batch strides != C*H*W on both sides
    ops.resize_bilinear_adjoint(gy, (5, 7), out=gx)
    want = R.resize_adjoint(gy.cpu().double().numpy(), (5, 7))
    assert _rel(gx, want) <= 1e-6
    assert bool((out[:, :1] == 3.0).all()) and bool((out[:, 4:] == 3.0).all())
    assert torch.equal(ops.resize_bilinear_adjoint(gy.contiguous(), (5, 7)), gx)


# ---- activation and blend adjoints -----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 1023, 4100])
@pytest.mark.parametrize("act", ["elu", "tanh"])
def test_act_backward(act, count, device):
    g = torch.Generator().manual_seed(count)
    z = torch.randn((2, 1, 1, count), generator=g) * 2
    y = torch.nn.functional.elu(z) if act == "elu" else torch.tanh(z)
    up = torch.randn((2, 1, 1, count), generator=g)
    model = R.elu_backward if act == "elu" else R.tanh_backward
    want = model(up.double().numpy(), y.double().numpy())
    got = ops.act_backward_(up.to(device), y.to(device), act, out=torch.empty((2, 1, 1, count), device=device))
    assert np.abs(got.cpu().double().numpy() - want).max() <= 1e-6
    inplace = up.to(device).clone()
    assert ops.act_backward_(inplace, y.to(device), act) is inplace and torch.equal(inplace, got)
    if count % 4 == 0:                                      # `got` took 16-byte accesses: the 4-byte path gives the same bits
        scalar = ops.act_backward_(_misaligned(up.to(device)), _misaligned(y.to(device)), act)
        assert torch.equal(scalar, got)


@pytest.mark.parametrize("act", ["elu", "tanh"])
def test_act_backward_on_a_misaligned_slice(act, device):
    g = torch.Generator().manual_seed(3)
    yb = torch.tanh(torch.randn((2, 5, 3, 7), generator=g)).to(device)
    gb = torch.randn((2, 6, 3, 7), generator=g).to(device)
    keep = gb.clone()
    y, gr = yb[:, 1:4], gb[:, 1:5][:, :3]                   # 21-float channels: bases off 16-byte alignment, odd strides
    assert gr.data_ptr() % 16 != 0
    model = R.elu_backward if act == "elu" else R.tanh_backward
    want = model(gr.cpu().double().numpy(), y.cpu().double().numpy())
    # four of the 21-float channels are 84 floats: misaligned in place (4-byte path), 16-byte path on dense copies
    y4, g4 = yb[:, 1:5], gb[:, 1:5]
    assert torch.equal(ops.act_backward_(g4, y4, act, out=torch.empty((2, 4, 3, 7), device=device)),
                       ops.act_backward_(g4.contiguous(), y4.contiguous(), act))
    ops.act_backward_(gr, y, act)
    assert np.abs(gr.cpu().double().numpy() - want).max() <= 1e-6
    assert torch.equal(gb[:, :1], keep[:, :1]) and torch.equal(gb[:, 4:], keep[:, 4:])


@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (2, 2), (31, 33), (41, 100)])
def test_blend_adjoints(h, w, device):
    g = torch.Generator().manual_seed(h * w)
    r = lambda *s: torch.randn(s, generator=g)
    n = 3
    pred, big = torch.tanh(r(n, 8, h, w)), torch.rand((n, 20, h, w), generator=g)
    max_amp = torch.rand(n, generator=g) + 0.5
    amp_in = big[:, 11:19]                                   # a channel slice, as in the block input buffer
    gp, ga = r(n * 4, 1, h, w), r(n * 4, 1, h, w)
    pd = pred.to(device).requires_grad_(True)
    ad = big.to(device)[:, 11:19]
    phase, amp = G.blend_level(pd, ad, max_amp.to(device))
    wp, wa = R.emit(pred.double().numpy(), amp_in.double().numpy(), max_amp.double().numpy())
    assert phase.shape == (n * 4, 1, h, w) and amp.shape == (n * 4, 1, h, w)
    assert np.abs(phase.detach().cpu().double().numpy().reshape(wp.shape) - wp).max() <= 1e-6
    assert np.abs(amp.detach().cpu().double().numpy().reshape(wa.shape) - wa).max() <= 1e-6
    ((phase * gp.to(device)).sum() + (amp * ga.to(device)).sum()).backward()
    g4 = lambda t: t.double().numpy().reshape(n, 4, h, w)
    want = R.emit_backward(g4(gp), g4(ga), amp_in.double().numpy(), max_amp.double().numpy())
    assert np.abs(pd.grad.cpu().double().numpy() - want).max() <= 1e-5
    # the NULL variants: one output's gradient alone
    for a, b in ((gp, None), (None, ga)):
        got = ops.phasenet_emit_backward(a.to(device) if a is not None else None, b.to(device) if b is not None else None,
                                         ad, max_amp.to(device))
        want = R.emit_backward(g4(a) if a is not None else None, g4(b) if b is not None else None, amp_in.double().numpy(),
                               max_amp.double().numpy())
        assert np.abs(got.cpu().double().numpy() - want).max() <= 1e-5
    pd.grad = None
    G.blend_level(pd, ad, max_amp.to(device))[1].sum().backward()      # autograd hands the node one None
    assert bool((pd.grad[:, :4] == 0).all()) and bool((pd.grad[:, 4:] != 0).any())
    # low level
    p0, low_in, max_low, gl = torch.tanh(r(n, 1, h, w)), r(n, 2, h, w), torch.rand(n, generator=g) + 0.5, r(n, 1, h, w)
    p0d = p0.to(device).requires_grad_(True)
    low = G.blend_low(p0d, low_in.to(device), max_low.to(device))
    assert np.abs(low.detach().cpu().double().numpy() - R.emit_low(p0.double().numpy(), low_in.double().numpy(),
                                                                    max_low.double().numpy())).max() <= 1e-5
    (low * gl.to(device)).sum().backward()
    want = R.emit_low_backward(gl.double().numpy(), low_in.double().numpy(), max_low.double().numpy())
    assert np.abs(p0d.grad.cpu().double().numpy() - want).max() <= 1e-5
    assert G.blend_low(p0.to(device), low_in.to(device), max_low.to(device)).grad_fn is None


# ---- the loss ----------------------------------------------------------------------------------------------------------
def test_loss_on_the_reference_fixture(golden_dir, device):
    z = np.load(os.path.join(golden_dir, "phasenet_loss.npz"))
    t = lambda k: torch.from_numpy(z[k]).to(device)
    pyr = types.SimpleNamespace(nbands=4)

    def run():
        po = [t("phase_o0").requires_grad_(True), t("phase_o1").requires_grad_(True)]
        out = t("output").requires_grad_(True)
        vals_o, vals_t = types.SimpleNamespace(phase=po), types.SimpleNamespace(phase=[t("phase_t0"), t("phase_t1")])
        got = get_loss(vals_o, vals_t, out, t("target"), pyr)
        got[0].backward()
        return got, po, out
    got, po, out = run()
    assert got[0].dim() == 0
    for a, k in zip(got, ("total_loss", "l_1_p", "phase_loss_p")):
        print(f"{k}: {float(a.detach()):.9g} (reference {float(z[k]):.9g})")
        assert abs(float(a.detach()) - float(z[k])) <= 1e-5 * abs(float(z[k])), k
    # gradients are +-const: d/d phase_o = -sign(wrap(phase_t - phase_o)) * 0.005 * nbands / count, d/d output = sign / count
    for i, p in enumerate(po):
        d = R.wrap(torch.from_numpy(z[f"phase_t{i}"]).double() - torch.from_numpy(z[f"phase_o{i}"]).double())
        want = -torch.sign(d) * 0.005 * 4 / d.numel()
        assert float((p.grad.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    d = torch.from_numpy(z["output"]).double() - torch.from_numpy(z["target"]).double()
    want = torch.sign(d) / d.numel()
    assert float((out.grad.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    again, po2, out2 = run()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(got, again))
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(po + [out], po2 + [out2]))
    # the target side's gradient (either output of vfi_l1_backward may be NULL)
    ga, gb = ops.l1_backward(t("output"), t("target"), torch.ones((), device=device), need_a=False, need_b=True)
    assert ga is None and float((gb.cpu().double() + want).abs().max()) <= 1e-6 * float(want.abs().max())


# ---- block gradients ---------------------------------------------------------------------------------------------------
def _block(sd, cin, pred, ks, device):
    blk = PhaseNetBlock(cin, 64, pred, (ks, ks)).to(device)
    blk.load_state_dict(sd)
    return blk


def _trained_like(layer, cin, pred, ks, seed):
    """A block state dict drawn to the statistics of the reference's trained phase_net.pt (tests/trained_stats.py)."""
    template = {f"layers.{layer}.{k}": v for k, v in R.block_state(0, cin, pred, ks).items()}
    sd = trained_stats.state_dict_like_trained("phasenet", template, seed)
    return {k[len(f"layers.{layer}."):]: v for k, v in sd.items()}


def _ref_block_grads(sd, x, gf, gc, dtype):
    P = {k: (v.to(dtype).clone().requires_grad_(k in R.BLOCK_KEYS) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    xr = x.to(dtype).clone().requires_grad_(True)
    f, c = R.block(P, xr)
    ((f * gf.to(dtype)).sum() + (c * gc.to(dtype)).sum()).backward()
    grads = {k: P[k].grad for k in R.BLOCK_KEYS}
    grads["x"] = xr.grad
    return (f.detach(), c.detach()), grads


def _hip_block_grads(blk, x, gf, gc, device, x_grad=True):
    blk.zero_grad(set_to_none=True)
    xd = x.to(device).requires_grad_(x_grad)
    f, c = blk(xd)
    ((f * gf.to(device)).sum() + (c * gc.to(device)).sum()).backward()
    grads = {k: p.grad for k, p in blk.named_parameters()}
    grads["x"] = xd.grad
    return (f.detach(), c.detach()), grads


BLOCK_CASES = [  # (cin, pred, ks, n, h, w, trained-statistics layer or None)
    (2, 1, 1, 3, 5, 7, None),            # block 0
    (81, 8, 1, 3, 9, 13, None),          # a level-1 block
    (88, 8, 3, 3, 24, 40, None),
    (88, 8, 3, 3, 37, 70, None),         # partial Winograd and weight-gradient tiles on both axes
    (88, 8, 3, 3, 24, 40, 3),            # drawn to the trained checkpoint's statistics
]


@pytest.mark.parametrize("cin,pred,ks,n,h,w,trained", BLOCK_CASES)
def test_block_gradients_match_float64_autograd(cin, pred, ks, n, h, w, trained, device):
    sd = R.block_state(3 + cin, cin, pred, ks) if trained is None else _trained_like(trained, cin, pred, ks, 1)
    g = torch.Generator().manual_seed(h * w)
    x = torch.randn((n, cin, h, w), generator=g)
    gf, gc = torch.randn((n, 64, h, w), generator=g), torch.randn((n, pred, h, w), generator=g)
    blk = _block(sd, cin, pred, ks, device)
    (f, c), got = _hip_block_grads(blk, x, gf, gc, device)
    (f64, c64), r64 = _ref_block_grads(sd, x, gf, gc, torch.float64)
    _, r32 = _ref_block_grads(sd, x, gf, gc, torch.float32)
    assert _rel(f, f64) <= 2e-4 and _rel(c, c64) <= 2e-4
    worst = (0.0, None)
    for k, want in r64.items():
        assert got[k] is not None, k
        err, lost32 = _rel(got[k], want), _rel(r32[k], want)
        print(f"  {k:28s} relative L2 {err:.3e} (float32 torch-CPU autograd: {lost32:.3e})")
        worst = max(worst, (err, k))
        assert err <= max(2e-4, 4 * lost32), (k, err, lost32)
    print(f"block {cin}->64->64->{pred} ks={ks} {n}x{h}x{w} trained={trained}: worst per-tensor relative L2 {worst[0]:.3e} ({worst[1]})")


# ---- behaviour -----------------------------------------------------------------------------------------------------------
def test_block_forward_is_the_three_inference_launches(device):
    for cin, pred, ks, h, w in ((2, 1, 1, 5, 7), (88, 8, 3, 24, 40)):
        sd = R.block_state(1, cin, pred, ks)
        blk = _block(sd, cin, pred, ks, device)
        x = torch.randn((3, cin, h, w), generator=torch.Generator().manual_seed(0)).to(device)
        with torch.no_grad():
            f0, c0 = blk(x)
        assert f0.grad_fn is None and c0.grad_fn is None
        fm = blk.feature_map
        mode = "reflect" if ks == 3 else "zeros"
        t = ops.conv2d(x, ops.PackedConv(fm[0].weight, fm[0].bias, bn=fm[1].fold_args()), mode, "elu")
        f = ops.conv2d(t, ops.PackedConv(fm[3].weight, fm[3].bias), mode, "elu")
        c = ops.conv2d(f, ops.PackedConv(blk.prediction_map[0].weight, blk.prediction_map[0].bias), "zeros", "tanh")
        assert torch.equal(f0, f) and torch.equal(c0, c)
        f1, c1 = blk(x)                                     # grad mode on, parameters require grad: the node
        assert f1.grad_fn is not None and c1.grad_fn is not None
        assert torch.equal(f1.detach(), f0) and torch.equal(c1.detach(), c0)
        for p in blk.parameters():
            p.requires_grad_(False)
        assert blk(x)[0].grad_fn is None                    # nothing requires grad: the plain launches


def test_block_in_training_mode_raises(device):
    blk = _block(R.block_state(1, 2, 1, 1), 2, 1, 1, device)
    blk.train(True)
    with pytest.raises(NotImplementedError, match="batch-statistics"):
        blk(torch.zeros((1, 2, 4, 4), device=device))
    blk.eval()
    blk(torch.zeros((1, 2, 4, 4), device=device))


def test_no_input_gradient_skips_conv1_data_gradient_and_backward_repeats(device):
    cin, pred, ks, n, h, w = 88, 8, 3, 3, 24, 40
    sd = R.block_state(2, cin, pred, ks)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((n, cin, h, w), generator=g)
    gf, gc = torch.randn((n, 64, h, w), generator=g), torch.randn((n, pred, h, w), generator=g)
    blk = _block(sd, cin, pred, ks, device)

    def dgrad_calls(x_grad):
        _lib.PROFILE = rec = _lib.Recorder()
        try:
            _, grads = _hip_block_grads(blk, x, gf, gc, device, x_grad=x_grad)
            calls = sum(1 for name, *_ in rec.rows if name == "vfi_conv2d_backward_data")
        finally:
            _lib.PROFILE = None
        return grads, calls
    with_x, calls_x = dgrad_calls(True)
    no_x, calls_no = dgrad_calls(False)
    assert (calls_x, calls_no) == (3, 2)
    assert no_x["x"] is None and with_x["x"] is not None
    again, _ = dgrad_calls(True)
    for k in with_x:
        assert torch.equal(with_x[k], again[k]), k
        if k != "x":
            assert torch.equal(with_x[k], no_x[k]), k
    # only the head requires grad: everything below it is skipped
    for k, p in blk.named_parameters():
        p.requires_grad_(k.startswith("prediction_map"))
    _, head_only = _hip_block_grads(blk, x, gf, gc, device, x_grad=False)
    for k, v in head_only.items():
        if k.startswith("prediction_map"):
            assert torch.equal(v, with_x[k]), k
        else:
            assert v is None, k


def test_packed_cache_follows_optimiser_step(device):
    cin, pred, ks = 88, 8, 3
    sd = R.block_state(8, cin, pred, ks)
    blk = _block(sd, cin, pred, ks, device)
    x = torch.randn((3, cin, 24, 40), generator=torch.Generator().manual_seed(1)).to(device)
    opt = torch.optim.Adam(blk.parameters(), lr=1e-2)
    f, c = blk(x)
    (f.abs().mean() + c.abs().mean()).backward()
    opt.step()
    with torch.no_grad():
        got = blk(x)
        want = _block(blk.state_dict(), cin, pred, ks, device)(x)
        old = _block(sd, cin, pred, ks, device)(x)
    for a, b, o in zip(got, want, old):
        assert torch.equal(a, b) and not torch.equal(a, o)


# ---- one composed level step from public pieces ------------------------------------------------------------------------
def _level_data(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)
    n = 3
    return {"low_in": r(n, 2, 6, 8), "max_low": torch.rand(n, generator=g) + 0.5,
            "phase": (torch.rand((n, 8, 9, 11), generator=g) * 2 - 1), "amp": torch.rand((n, 8, 9, 11), generator=g),
            "max_amp": torch.rand(n, generator=g) + 0.5,
            "phase_t": (torch.rand((n * 4, 1, 9, 11), generator=g) * 2 - 1) * math.pi,
            "amp_t": torch.rand((n * 4, 1, 9, 11), generator=g), "low_t": r(n, 1, 6, 8)}


def _hip_level_loss(blk0, blk1, data):
    from vfi_amd.train.loss import l1_loss, phase_term
    return R.level_step(blk0, blk1, data, G.resize_bilinear, blk=lambda b, x: b(x), blend=G.blend_level, blend_low_=G.blend_low,
                        phase_loss=lambda o, t: phase_term(o, t, 4), l1=l1_loss)


def test_composed_level_step_gradients_and_adam_run(device):
    sd0, sd1 = R.block_state(20, 2, 1, 1), R.block_state(21, 81, 8, 1)
    data = _level_data(5)
    on_dev = {k: v.to(device) for k, v in data.items()}
    blk0, blk1 = _block(sd0, 2, 1, 1, device), _block(sd1, 81, 8, 1, device)
    loss = _hip_level_loss(blk0, blk1, on_dev)
    loss.backward()

    def ref(dtype):
        P = [{k: (v.to(dtype).clone().requires_grad_(k in R.BLOCK_KEYS) if v.dtype.is_floating_point else v) for k, v in sd.items()}
             for sd in (sd0, sd1)]
        val = R.level_step(P[0], P[1], {k: v.to(dtype) for k, v in data.items()}, R.torch_resize)
        val.backward()
        return val, P
    l64, P64 = ref(torch.float64)
    _, P32 = ref(torch.float32)
    print(f"level step loss {float(loss.detach()):.7f} (float64 {float(l64.detach()):.7f})")
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-5 * abs(float(l64.detach()))
    for i, blk in enumerate((blk0, blk1)):
        for k, p in blk.named_parameters():
            want = P64[i][k].grad
            err, lost32 = _rel(p.grad, want), _rel(P32[i][k].grad, want)
            print(f"  block {i} {k:28s} relative L2 {err:.3e} (float32 torch-CPU autograd: {lost32:.3e})")
            assert err <= max(2e-4, 4 * lost32), (i, k, err, lost32)

    def run(params, step_loss, steps):
        opt = torch.optim.Adam(params, lr=1e-3)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            val = step_loss()
            val.backward()
            opt.step()
            losses.append(float(val.detach()))
        return losses
    gpu = run(list(blk0.parameters()) + list(blk1.parameters()), lambda: _hip_level_loss(blk0, blk1, on_dev), 30)
    P = [{k: (v.double().clone().requires_grad_(k in R.BLOCK_KEYS) if v.dtype.is_floating_point else v) for k, v in sd.items()}
         for sd in (sd0, sd1)]
    d64 = {k: v.double() for k, v in data.items()}
    cpu = run([P[i][k] for i in (0, 1) for k in R.BLOCK_KEYS], lambda: R.level_step(P[0], P[1], d64, R.torch_resize), 30)
    print("Adam run, HIP :", " ".join(f"{v:.5f}" for v in gpu))
    print("Adam run, CPU :", " ".join(f"{v:.5f}" for v in cpu))
    assert gpu[-1] < gpu[0], gpu
    for a, b in zip(gpu, cpu):
        assert abs(a - b) <= 0.02 * abs(b), (gpu, cpu)
