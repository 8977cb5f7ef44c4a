"""SSIM as a loss on the MI355X: vfi_ssim_loss_forward, vfi_ssim_loss_backward and
vfi_avg_pool_backward through the C ABI against float64, vfi_amd.evaluation.ssim.SSIMLoss end to end, and the two places it
plugs into.

References and bounds: tests/ssim_loss_ref.py -- scoring_ref.ssim_ref's expression on a batch in float64, gradients by
autograd; a value within max(2e-5, 4 * mean|map32 - map64|) per image, a gradient within glue_ref.tol_of(g32, g64).  Every
figure is printed before it is asserted.  T = ssim_loss_ref.TILE = 32 is the tile of both kernels."""
import math
import types

import pytest
import torch

import glue_ref as G
import scoring_ref as SR
import ssim_loss_ref as R
from vfi_amd import _lib, ops
from vfi_amd.evaluation import evaluate_image as ei
from vfi_amd.evaluation import ssim as ssim_mod

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.ENTRY_CASES]
WALK = pytest.param(R.WALK_CASE, id=R.case_id(R.WALK_CASE) + "-walk")
C1, C2 = SR.K1 ** 2, SR.K2 ** 2


def _separate(t, device):
    """t one float into an allocation of its own between NaN canaries -> (flat canary buffer, view)"""
    flat = G.canary_buffer(t.numel() + 2, device)
    v = G.fview(flat, t.shape, 1)
    v.copy_(t.to(device))
    return flat, v


def _halves(x, y, device):
    """x and y as the two halves of one (N, 2, C, H, W) tensor one float into its allocation: batch stride 2 C H W"""
    n, c, h, w = x.shape
    chw = c * h * w
    flat = G.canary_buffer(2 * n * chw + 2, device)
    both = G.fview(flat, (n, 2, c, h, w), 1)
    both.copy_(torch.stack([x, y], 1).to(device))
    strides = (2 * chw, h * w, w, 1)
    return flat, G.fview(flat, x.shape, 1, strides), G.fview(flat, x.shape, 1 + chw, strides), both


def _forward(xv, yv, ks, sigma, device, c1=C1, c2=C2):
    """vfi_ssim_loss_forward into a canary buffer, the workspace NaN -> (N,) values; checks that nothing else was written"""
    n, c, h, w = xv.shape
    oflat = G.canary_buffer(n + 4, device)
    out = G.fview(oflat, (n,), 2)
    ws = torch.full((_lib.REDUCE_WORKSPACE_FLOATS,), float("nan"), device=device)
    _lib.call("vfi_ssim_loss_forward", xv.data_ptr(), xv.stride(0), yv.data_ptr(), yv.stride(0), out.data_ptr(), ws.data_ptr(),
              n, c, h, w, ks, float(sigma), float(c1), float(c2), _lib.stream_ptr())
    G.assert_untouched(oflat, out, what="forward out")
    return out.clone()


def _backward(xv, yv, up, ks, sigma, device, pad=3, c1=C1, c2=C2):
    """vfi_ssim_loss_backward into a slice (batch stride C H W + pad) of a canary buffer -> dense copy of grad_x"""
    n, c, h, w = xv.shape
    chw = c * h * w
    gflat = G.canary_buffer(n * (chw + pad) + 2, device)
    gx = G.fview(gflat, (n, c, h, w), 1, (chw + pad, h * w, w, 1))
    upd = up.to(device)
    _lib.call("vfi_ssim_loss_backward", xv.data_ptr(), xv.stride(0), yv.data_ptr(), yv.stride(0), upd.data_ptr(), gx.data_ptr(),
              chw + pad, n, c, h, w, ks, float(sigma), float(c1), float(c2), _lib.stream_ptr())
    G.assert_untouched(gflat, gx, what="grad_x")
    return gx.clone()


def _check_values(got, c, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    for i in range(got.numel()):
        err = abs(float(got[i]) - float(c["v64"][i]))
        print(f"{what} image {i}: loss {float(got[i]):.7f} err {err:.3e} bound {c['bound'][i]:.3e} (float32 reference {abs(float(c['v32'][i]) - float(c['v64'][i])):.3e})")
        assert err <= c["bound"][i], (what, i, err, c["bound"][i])


@pytest.mark.parametrize("layout", ["separate", "halves"])
@pytest.mark.parametrize("case", [pytest.param(c, id=i) for c, i in zip(R.ENTRY_CASES, IDS)] + [WALK])
def test_entries_against_float64(case, layout, device):
    shape, ks, sigma = case
    c = R.case(shape, ks, sigma)
    if layout == "separate":
        xflat, xv = _separate(c["x"], device)
        yflat, yv = _separate(c["y"], device)
        guards = [(xflat, xv), (yflat, yv)]
    else:
        flat, xv, yv, both = _halves(c["x"], c["y"], device)
        guards = [(flat, both)]
    loss = _forward(xv, yv, ks, sigma, device)
    _check_values(loss, c, f"{R.case_id(case)} {layout} forward")
    gx = _backward(xv, yv, c["up"], ks, sigma, device)
    G.assert_close(gx, c["gx32"], c["gx64"], f"{R.case_id(case)} {layout} grad_x (largest entry {float(c['gx64'].abs().max()):.3e})")
    gy = _backward(yv, xv, c["up"], ks, sigma, device)                      # the roles exchanged: the target's gradient
    G.assert_close(gy, c["gy32"], c["gy64"], f"{R.case_id(case)} {layout} grad_y by the exchanged call")
    for flat, v in guards:                                                   # the inputs and their canaries are as they were
        G.assert_untouched(flat, v, what="inputs")
    assert torch.equal(xv.cpu(), c["x"]) and torch.equal(yv.cpu(), c["y"])


@pytest.mark.parametrize("case", [pytest.param(c, id=i) for c, i in zip(R.ENTRY_CASES, IDS)] + [WALK])
def test_equal_images_give_exactly_zero(case, device):
    shape, ks, sigma = case
    c = R.case(shape, ks, sigma)
    x = c["x"].to(device)
    loss = _forward(x, x.clone(), ks, sigma, device)
    assert bool((loss == 0).all()) and not bool(torch.signbit(loss).any()), loss
    assert bool((ops.ssim_loss_forward(x, x, ks, sigma) == 0).all())
    assert bool((ssim_mod.ssim(x, x, kernel_size=ks, kernel_sigma=sigma, downsample=False) == 1).all())


@pytest.mark.parametrize("case", [R.ENTRY_CASES[1], R.ENTRY_CASES[5], R.ENTRY_CASES[9], R.ENTRY_CASES[10]],
                         ids=[IDS[1], IDS[5], IDS[9], IDS[10]])
def test_bits_do_not_depend_on_the_batch(case, device):
    """an image's value and gradient: alone, at each position of a batch of 3 (and of 6: two launch pairs), and twice"""
    shape, ks, sigma = case
    shape3 = (3,) + tuple(shape[1:])
    x, y = (t.to(device) for t in R.batch_inputs(shape3, 500))
    up = torch.tensor([0.9, 0.9, 0.9], device=device)
    one = lambda a, b: (ops.ssim_loss_forward(a, b, ks, sigma), ops.ssim_loss_backward(a, b, up[:a.shape[0]], ks, sigma))
    v1, g1 = one(x[:1], y[:1])
    v1b, g1b = one(x[:1], y[:1])
    assert torch.equal(v1, v1b) and torch.equal(g1, g1b)
    for pos in range(3):
        order = [(pos + k) % 3 for k in range(3)]                  # image 0 sits at position (3 - pos) % 3
        at = order.index(0)
        v3, g3 = one(x[order].contiguous(), y[order].contiguous())
        assert torch.equal(v3[at], v1[0]) and torch.equal(g3[at], g1[0]), (pos, at)
    x6, y6 = torch.cat([x[1:], x[1:], x[:1], x[1:2]], 0), torch.cat([y[1:], y[1:], y[:1], y[1:2]], 0)       # image 0 at position 4
    v6 = ops.ssim_loss_forward(x6, y6, ks, sigma)
    g6 = ops.ssim_loss_backward(x6, y6, torch.full((6,), 0.9, device=device), ks, sigma)
    assert torch.equal(v6[4], v1[0]) and torch.equal(g6[4], g1[0])
    assert torch.equal(v6[0], v6[5]) and torch.equal(g6[0], g6[5]) and torch.equal(v6[1], v6[3])       # across the two launches


@pytest.mark.parametrize("planes,h,w,f", [(3, 7, 10, 3), (2, 9, 8, 2), (1, 5, 5, 1), (2, 13, 11, 4), (1, 70, 33, 5)])
def test_avg_pool_backward_entry(planes, h, w, f, device):
    """g / f^2 on every pixel of a window, exactly 0 on the rows and columns the floor drops, nothing else written"""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(planes * 100 + h)
    g = torch.randn((planes, h // f, w // f), generator=gen)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        z = torch.zeros((1, planes, h, w), dtype=dtype, requires_grad=True)
        (F.avg_pool2d(z, f) * g.to(dtype)).sum().backward()
        ref[dtype] = z.grad[0]
    gflat, gv = _separate(g, device)
    oflat = G.canary_buffer(planes * h * w + 2, device)
    out = G.fview(oflat, (planes, h, w), 1)
    _lib.call("vfi_avg_pool_backward", gv.data_ptr(), out.data_ptr(), planes, h, w, f, _lib.stream_ptr())
    G.assert_untouched(oflat, out, what="avg_pool_backward out")
    G.assert_untouched(gflat, gv, what="avg_pool_backward grad")
    G.assert_close(out, ref[torch.float32], ref[torch.float64], f"avg_pool_backward {planes}x{h}x{w} f {f}")
    ho, wo = (h // f) * f, (w // f) * f
    dropped = torch.cat([out[:, ho:, :].flatten(), out[:, :, wo:].flatten()]).cpu()
    assert dropped.numel() == planes * (h * w - ho * wo) + planes * (h - ho) * (w - wo)
    assert bool((dropped == 0).all()) and not bool(torch.signbit(dropped).any())
    if f in (1, 2, 4):                                                   # 1 / f^2 is a power of two: the products are exact
        assert torch.equal(out.cpu(), ref[torch.float32])


# ---- the module ---------------------------------------------------------------------------------------------------------
def _reduced(v, reduction):
    return v if reduction == 'none' else (v.mean() if reduction == 'mean' else v.sum())


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("case", R.ENTRY_CASES, ids=IDS)
def test_module_against_float64(case, reduction, device):
    shape, ks, sigma = case
    c = R.case(shape, ks, sigma)
    n = shape[0]
    crit = ssim_mod.SSIMLoss(kernel_size=ks, kernel_sigma=sigma, reduction=reduction)
    x, y = c["x"].to(device).requires_grad_(True), c["y"].to(device).requires_grad_(True)
    got = crit(x, y)
    assert got.shape == ((n,) if reduction == 'none' else ()) and got.dtype == torch.float32
    if reduction == 'none':
        (got * c["up"].to(device)).sum().backward()
        _check_values(got.detach(), c, f"{R.case_id(case)} module")
        ref = (c["gx32"], c["gx64"], c["gy32"], c["gy64"])
    else:
        got.backward()
        want = float(_reduced(c["v64"], reduction))
        bound = float(_reduced(torch.tensor(c["bound"], dtype=torch.float64), reduction))
        err = abs(float(got.detach()) - want)
        print(f"{R.case_id(case)} module {reduction}: {float(got.detach()):.7f} err {err:.3e} bound {bound:.3e}")
        assert err <= bound
        ref = R.reduced_grads(shape, ks, sigma, reduction)
    G.assert_close(x.grad, ref[0], ref[1], f"{R.case_id(case)} module {reduction} grad to the prediction")
    G.assert_close(y.grad, ref[2], ref[3], f"{R.case_id(case)} module {reduction} grad to the target")
    # the no-grad face has the node's bits; so has a call whose arguments need no gradient
    with torch.no_grad():
        assert torch.equal(crit(x, y), got.detach())
    assert torch.equal(crit(x.detach(), y.detach()), got.detach())
    assert torch.equal(ssim_mod.ssim(x.detach(), y.detach(), kernel_size=ks, kernel_sigma=sigma),
                       1 - ssim_mod.SSIMLoss(kernel_size=ks, kernel_sigma=sigma, reduction='none')(x.detach(), y.detach()))


@pytest.mark.parametrize("case", R.POOLED_CASES, ids=[R.case_id(c) for c in R.POOLED_CASES])
def test_module_pooled_against_float64(case, device):
    """f = 2 (384 x 385: the last column dropped) and f = 3 (641 x 643: two rows and one column dropped)"""
    shape, ks, sigma = case
    c = R.case(shape, ks, sigma, True)
    f = c["f"]
    assert f == SR.pool_factor(*shape[2:]) == {384: 2, 641: 3}[shape[2]]
    x, y = c["x"].to(device).requires_grad_(True), c["y"].to(device).requires_grad_(True)
    got = ssim_mod.SSIMLoss(reduction='none')(x, y)
    _check_values(got.detach(), c, f"{R.case_id(case)} pooled by {f}")
    (got * c["up"].to(device)).sum().backward()
    G.assert_close(x.grad, c["gx32"], c["gx64"], f"{R.case_id(case)} grad to the prediction")
    G.assert_close(y.grad, c["gy32"], c["gy64"], f"{R.case_id(case)} grad to the target")
    h, w = shape[2:]
    ho, wo = (h // f) * f, (w // f) * f
    assert (ho, wo) != (h, w)
    for g in (x.grad, y.grad):
        dropped = torch.cat([g[:, :, ho:, :].flatten(), g[:, :, :, wo:].flatten()])
        assert dropped.numel() > 0 and bool((dropped == 0).all())
        assert float(g[:, :, ho - 1, :wo].abs().max()) > 0 and float(g[:, :, :ho, wo - 1].abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(ssim_mod.SSIMLoss(reduction='none')(x, y), got.detach())


@pytest.mark.parametrize("i", range(len(SR.SSIM_CASES)), ids=[SR.case_id(c) for c in SR.SSIM_CASES])
def test_module_on_the_scoring_cases(i, device):
    """1 - SSIMLoss(reduction='none') within the bound evaluate_image.ssim is held to, on the same images"""
    (_, downsample, _), c = SR.SSIM_CASES[i], SR.ssim_case(i)
    x, y = c["x"].unsqueeze(0).to(device), c["y"].unsqueeze(0).to(device)
    got = 1 - ssim_mod.SSIMLoss(reduction='none', downsample=downsample)(x, y)
    err = abs(float(got[0]) - c["ref64"])
    metric = ei.ssim(x[0], y[0], downsample=downsample)
    print(f"{SR.case_id(SR.SSIM_CASES[i])}: f {c['f']} err {err:.3e} bound {c['bound']:.3e}; evaluate_image.ssim err {abs(metric - c['ref64']):.3e}")
    assert err <= c["bound"]
    assert abs(float(got[0]) - metric) <= 2 * c["bound"]


def test_module_refuses_before_any_launch(device, monkeypatch):
    """10 x 40, an even window, 384 x 10: ValueError with no call into the library.  384 x 20 is not among them: piq's factor
    comes from the short side, round(20 / 256) = 0 -> 1, so it is not pooled, its map is 374 x 10, and piq scores it; it is
    checked against float64 instead (tests/test_ssim_loss_host.py says why nothing can be too small after pooling)."""
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    z = lambda *s: torch.zeros(s, device=device, requires_grad=True)
    with pytest.raises(ValueError, match="smaller than the 11-tap window"):
        ssim_mod.SSIMLoss()(z(1, 3, 10, 40), z(1, 3, 10, 40))
    with pytest.raises(ValueError, match="smaller than the 11-tap window"):
        ssim_mod.SSIMLoss()(z(1, 1, 384, 10), z(1, 1, 384, 10))
    with pytest.raises(ValueError, match="kernel_size"):
        ssim_mod.ssim(z(1, 3, 40, 40), z(1, 3, 40, 40), kernel_size=10)
    with pytest.raises(ValueError, match="kernel_size"):
        ssim_mod.SSIMLoss(kernel_size=4)
    with pytest.raises(ValueError, match="must be equal"):
        ssim_mod.SSIMLoss()(z(1, 3, 40, 40), z(1, 1, 40, 40))
    assert calls == []
    x, y = R.batch_inputs((1, 1, 384, 20), 77)
    got = ssim_mod.ssim(x.to(device), y.to(device))
    s64, m64 = SR.ssim_ref(x[0, :], y[0, :], torch.float64)
    _, m32 = SR.ssim_ref(x[0, :], y[0, :], torch.float32)
    bound = max(2e-5, 4.0 * (m32.double() - m64).abs().mean().item())
    print(f"384x20: err {abs(float(got[0]) - s64):.3e} bound {bound:.3e}")
    assert abs(float(got[0]) - s64) <= bound and calls == ["vfi_ssim_loss_forward"]
    # the entries themselves: status codes, nothing written
    flat = G.canary_buffer(64, device)
    out = G.fview(flat, (1,), 8)
    t = torch.zeros((1, 1, 12, 12), device=device)
    for args in ((1, 1, 10, 12, 11), (1, 1, 12, 12, 10), (0, 1, 12, 12, 11), (1, 0, 12, 12, 11)):
        n, c, h, w, ks = args
        st = _lib.lib().vfi_ssim_loss_forward(t.data_ptr(), 144, t.data_ptr(), 144, out.data_ptr(), flat.data_ptr() + 64, n, c, h, w, ks,
                                              1.5, C1, C2, _lib.stream_ptr())
        assert st == (-2 if h < ks else -1), args
        st = _lib.lib().vfi_ssim_loss_backward(t.data_ptr(), 144, t.data_ptr(), 144, t.data_ptr(), out.data_ptr(), 144, n, c, h, w, ks,
                                               1.5, C1, C2, _lib.stream_ptr())
        assert st == (-2 if h < ks else -1), args
    torch.cuda.synchronize()
    G.assert_untouched(flat, what="refused calls")


# ---- where it plugs in ----------------------------------------------------------------------------------------------------
def test_adacof_loss_with_an_ssim_term(device):
    from oracle import nets_cpu
    from vfi_amd.adacof import losses, utility
    from vfi_amd.adacof.models import Model
    model = Model(types.SimpleNamespace(model="vfi_amd.adacof.models.adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    model.load(nets_cpu.adacofnet_random_state_dict(9, kernel_size=5))
    model.train(True)
    g = torch.Generator().manual_seed(4)
    f0, f1, f2 = (torch.rand((2, 3, 64, 64), generator=g).to(device) for _ in range(3))
    crit = losses.Loss(types.SimpleNamespace(loss='1*Charb+0.1*SSIM', gpu_id=0))
    assert [l['type'] for l in crit.loss] == ['Charb', 'SSIM'] and isinstance(crit.loss_module[1], ssim_mod.SSIMLoss)
    out = model(f0, f2)
    got = crit(out, f1, [f0, f2])
    frame = out["frame1"].detach().requires_grad_(True)
    term = crit.loss_module[1](frame, f1)
    assert term.dim() == 0 and torch.equal(term.detach(), ssim_mod.SSIMLoss(reduction='none')(frame.detach(), f1).mean())
    assert 0 < float(term.detach()) < 2
    parts = [1.0 * utility.Module_CharbonnierLoss()(frame, f1), 0.1 * term]
    assert torch.equal(got.detach(), sum(parts).detach())
    got.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    # the term's gradient reaches the network: the same step without it gives other gradients
    with_term = [p.grad.clone() for p in model.parameters()]
    model.zero_grad()
    losses.Loss(types.SimpleNamespace(loss='1*Charb', gpu_id=0))(model(f0, f2), f1, [f0, f2]).backward()
    assert any(not torch.equal(a, p.grad) for a, p in zip(with_term, model.parameters()))


def _fusion_models(device, h, w):
    """the seeded networks of tests/test_trainer_gpu.py"""
    import numpy as np
    from oracle import pipeline_cpu
    from vfi_amd.adacof.models import Model
    from vfi_amd.fusion_net.fusion_net import FusionNet
    from vfi_amd.phase_net.phase_net import PhaseNet
    from vfi_amd.train.pyramid import Pyramid
    from vfi_amd.train.utils import calc_pyr_height
    weights = pipeline_cpu.seeded_weights(0)
    fusion = FusionNet().to(device)
    fusion.load_state_dict(weights["fusionnet"])
    pyr = Pyramid(height=calc_pyr_height(torch.empty(3, h, w, device="meta")), nbands=4, scale_factor=np.sqrt(2), device=device)
    phase_net = PhaseNet(pyr, device, num_img=2)
    phase_net.load_state_dict(weights["phasenet"])
    adacof = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    adacof.load(weights["adacof"])
    adacof.eval()
    return adacof, fusion, pyr, phase_net


def _seed(s):
    import random
    import numpy as np
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.mark.parametrize("ssim_weight", [0.1, 0])
def test_fusion_net_trainer_step(ssim_weight, tmp_path, device):
    """one FusionNet Trainer epoch of one batch against the same loop written out; at weight 0 that loop is the parent's"""
    import train_batch_ref as TR
    from vfi_amd.fusion_net.train_batch import fusion_net_inputs
    from vfi_amd.fusion_net.trainer import Trainer
    from vfi_amd.train.datareader import DBreader_Vimeo90k, TripletLoader
    h, w, lr = 64, 96, 1e-4
    root = TR.write_triplets(str(tmp_path / "vimeo"), 2, 72, 104, seed=2, smooth=True)
    loader = lambda: TripletLoader(DBreader_Vimeo90k(root, random_crop=(h, w)), 2, shuffle=True, workers=2, device=device)
    adacof, fusion, pyr, phase_net = _fusion_models(device, h, w)
    _seed(9)
    args = types.SimpleNamespace(epochs=1, gpu_id=0, test_paths=None, save=False, ssim_weight=ssim_weight)
    trainer = Trainer(args, loader(), fusion, phase_net, adacof, my_pyr=pyr, lr=lr, out_dir=str(tmp_path / "out"))
    assert (trainer.ssim is None) == (ssim_weight == 0) and trainer.lpips is None and trainer.max_step == 1
    trainer.train()
    history = list(trainer.loss_history)
    trainer.close()

    adacof2, ref, pyr2, phase_net2 = _fusion_models(device, h, w)
    ref.train()
    _seed(9)
    opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=0.0)
    term = ssim_mod.SSIMLoss(reduction='none') if ssim_weight else None
    manual, l1s = [], []
    for batch in loader():
        inputs = fusion_net_inputs(adacof2, phase_net2, pyr2, batch.lab_frame1, batch.lab_frame2, batch.rgb_frame1, batch.rgb_frame2)
        final = torch.clip(ref(*inputs, variant=0), 0, 1)
        loss = torch.nn.L1Loss()(batch.rgb_target, final)            # the parent's loss
        l1s.append(float(loss.detach()))
        if term is not None:
            loss = loss + ssim_weight * term(final, batch.rgb_target).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        manual.append(float(loss.detach()))
    print(f"ssim_weight {ssim_weight}: loss history {history}, by hand {manual}, its L1 part {l1s}")
    assert len(history) == 1 and math.isfinite(history[0]) and history == manual
    assert (history[0] > l1s[0]) if ssim_weight else (history == l1s)
    for (k, p), (k2, q) in zip(fusion.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
