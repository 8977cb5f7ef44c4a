"""LPIPS on the MI355X: the two head entries alone against float64, the module end to end against
float64 autograd of the decision-pinned restatement (tests/lpips_ref.py), and the three places it plugs into.

Bounds.  The yardstick of a case is the error that the same restatement makes in float32 on the CPU against float64 on the
same inputs -- the worst over the batch sizes and images of that case -- relative to the per-image value and to the largest
gradient entry.  The product gets four times it: the margin covers a different but fixed order of summation, nothing more.
Both figures are printed."""
import math
import types

import pytest
import torch

import lpips_ref as LR
from vfi_amd import ops
from vfi_amd.evaluation import evaluate_image as ei
from vfi_amd.evaluation import lpips

pytestmark = pytest.mark.gpu

# (C, HW): the tile widths 1, 4, 16, 64 of the kernels (HW < 8, < 128, < 65536, above), tails, one channel, more channels than
# channel groups, and, last, more tiles than blocks of the forward's grid (1024), so that a block walks several
HEAD_CASES = [(1, 1), (3, 9), (64, 35), (64, 256), (65, 257), (512, 1), (512, 4), (5, 2050), (2, 65606)]
NAN = float("nan")


def _guarded(t, device):
    """t one float into an allocation of its own, between NaN canaries -> (allocation, view of t's shape)"""
    buf = torch.full((t.numel() + 2,), NAN, device=device)
    buf[1:-1] = t.flatten().to(device)
    return buf, buf[1:-1].view(t.shape)


def _intact(buf):
    return bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1])) and not bool(torch.isnan(buf[1:-1]).any())


def _value_err(got, want):
    return float(((got.double().cpu() - want).abs() / want.abs().clamp_min(1e-300)).max())


def _grad_err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _upstream(n):
    return torch.linspace(0.5, 1.5, n) if n > 1 else torch.tensor([0.7])


def _head_reference(x, y, w, dtype):
    xx = x.clone().to(dtype).requires_grad_(True)
    v = LR.head(xx, y.to(dtype), w)
    (v * _upstream(x.shape[0]).to(dtype)).sum().backward()
    return v.detach(), xx.grad


@pytest.fixture(scope="module")
def head_refs():
    """per case and batch size: inputs, float64 value and gradient; per case: the float32 torch-CPU yardsticks"""
    refs, yard = {}, {}
    for c, hw in HEAD_CASES:
        worst_v = worst_g = 0.0
        for n in (1, 3):
            x, y, w = LR.head_inputs(n, c, hw)
            v64, g64 = _head_reference(x, y, w, torch.float64)
            v32, g32 = _head_reference(x, y, w, torch.float32)
            refs[c, hw, n] = (x, y, w, v64, g64)
            worst_v, worst_g = max(worst_v, _value_err(v32, v64)), max(worst_g, _grad_err(g32, g64))
        yard[c, hw] = (worst_v, worst_g)
    return refs, yard


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c,hw", HEAD_CASES)
def test_head_entries_against_float64(c, hw, n, head_refs, device):
    refs, yard = head_refs
    x, y, w, v64, g64 = refs[c, hw, n]
    yv, yg = yard[c, hw]
    xy_buf, xy = _guarded(torch.cat([x, y], 0), device)          # y's base: N * C * HW + 1 floats into the allocation
    xd, yd = xy[:n], xy[n:]
    w_buf, wd = _guarded(w, device)
    up_buf, up = _guarded(_upstream(n), device)
    prior_buf, prior = _guarded(torch.arange(n, dtype=torch.float32) + 0.25, device)

    got = ops.lpips_head_forward(xd, yd, wd)
    assert got.shape == (n,)
    ev = _value_err(got, v64)
    with_prior = ops.lpips_head_forward(xd, yd, wd, prior)
    assert torch.equal(with_prior, prior + got)                  # prior + this tap's value, one rounding

    g_buf, gd = _guarded(torch.zeros_like(x), device)
    assert ops.lpips_head_backward(xd, yd, wd, up, relu_mask=False, out=gd) is gd
    eg = _grad_err(gd, g64)
    print(f"head C={c} HW={hw} N={n}: value rel err {ev:.2e} (fp32 torch-CPU, worst of the case {yv:.2e}); "
          f"gradient err / largest entry {eg:.2e} (fp32 torch-CPU {yg:.2e})")
    assert all(_intact(b) for b in (xy_buf, w_buf, up_buf, prior_buf, g_buf))
    assert ev <= 4 * yv
    assert eg <= 4 * yg
    # a pixel where x is zero: gradient 0, also where y is not
    dead = (x == 0).all(1, keepdim=True).expand_as(x)
    assert bool((gd.cpu()[dead] == 0).all()) and bool((g64[dead] == 0).all())
    if hw >= 3:
        assert bool(dead[:, :, 0].all()) and bool(dead[:, :, 2].all()) and not bool((y[:, :, 0] == 0).all())
    # with the mask: zero wherever x is not positive, and `above` added exactly
    above_buf, above = _guarded(torch.randn(x.shape, generator=torch.Generator().manual_seed(c + hw)), device)
    m_buf, md = _guarded(torch.zeros_like(x), device)
    ops.lpips_head_backward(xd, yd, wd, up, above=above, relu_mask=True, out=md)
    assert all(_intact(b) for b in (above_buf, m_buf, xy_buf))
    assert torch.equal(md, torch.where(xd > 0, above + gd, torch.zeros_like(gd)))
    masked = ops.lpips_head_backward(xd, yd, wd, up, relu_mask=True)
    assert torch.equal(masked, torch.where(xd > 0, gd, torch.zeros_like(gd)))
    # in place on `above`
    inplace = above.clone()
    ops.lpips_head_backward(xd, yd, wd, up, above=inplace, relu_mask=True, out=inplace)
    assert torch.equal(inplace, md)
    # two runs: equal bits
    assert torch.equal(ops.lpips_head_forward(xd, yd, wd), got)
    assert torch.equal(ops.lpips_head_backward(xd, yd, wd, up, relu_mask=False), gd)
    # x against itself: exactly 0, value and gradient
    assert bool((ops.lpips_head_forward(xd, xd, wd) == 0).all())
    assert bool((ops.lpips_head_backward(xd, xd, wd, up, relu_mask=False) == 0).all())


@pytest.mark.parametrize("c,hw", HEAD_CASES)
def test_head_bits_do_not_depend_on_the_batch(c, hw, head_refs, device):
    x, y, w = (t.to(device) for t in head_refs[0][c, hw, 3][:3])
    up = torch.full((3,), 0.7, device=device)
    batch = ops.lpips_head_forward(x, y, w)
    gbatch = ops.lpips_head_backward(x, y, w, up)
    for order in ([2, 0, 1], [1, 2, 0]):
        assert torch.equal(ops.lpips_head_forward(x[order].contiguous(), y[order].contiguous(), w), batch[order])
        assert torch.equal(ops.lpips_head_backward(x[order].contiguous(), y[order].contiguous(), w, up), gbatch[order])
    for i in range(3):
        assert torch.equal(ops.lpips_head_forward(x[i:i + 1], y[i:i + 1], w), batch[i:i + 1])
        assert torch.equal(ops.lpips_head_backward(x[i:i + 1], y[i:i + 1], w, up[:1]), gbatch[i:i + 1])
    # more images than one launch of the forward takes
    many = ops.lpips_head_forward(x.repeat(3, 1, 1), y.repeat(3, 1, 1), w)
    assert torch.equal(many, batch.repeat(3))


def test_normalize_and_its_adjoint(device):
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 5, 7), generator=g)
    buf, xd = _guarded(x, device)
    want = LR.normalize(x.double())
    got = ops.lpips_normalize(xd)
    assert float((got.cpu().double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max()) and _intact(buf)
    std = torch.tensor(LR.STD).view(1, 3, 1, 1)
    assert torch.equal(ops.lpips_normalize(xd, adjoint=True).cpu(), x / std)


# ---- the module ---------------------------------------------------------------------------------------------------------
MODULE_CASES = [(16, 16), (16, 48), (48, 16), (32, 32)]


@pytest.fixture(scope="module")
def vgg_state():
    return LR.vgg16_state(11)


@pytest.fixture(scope="module")
def heads():
    return LR.head_weights(11)


@pytest.fixture(scope="module")
def node(vgg_state, heads, device):
    return lpips.LPIPS(vgg_state, heads).to(device).eval()


def _images(b, h, w):
    g = torch.Generator().manual_seed(h * 100 + w + b)
    x = torch.rand((b, 3, h, w), generator=g)
    return x, (x + 0.2 * torch.randn((b, 3, h, w), generator=g)).clamp(0, 1)


@pytest.fixture(scope="module")
def module_runs(node, vgg_state, heads, device):
    """per (h, w, b): the product's scores and image gradient, float64 autograd of the pinned restatement, and the errors of
    the same restatement in float32 on the CPU"""
    runs = {}
    for h, w in MODULE_CASES:
        for b in (1, 3):
            x, y = _images(b, h, w)
            xd = x.to(device).requires_grad_(True)
            yd = y.to(device).requires_grad_(True)
            got = node(xd, yd)
            up = _upstream(b)
            (got * up.to(device)).sum().backward()
            dec = LR.lpips_decisions(node, xd.detach(), yd.detach())
            res = {}
            for dtype in (torch.float64, torch.float32):
                xx = x.clone().to(dtype).requires_grad_(True)
                v = LR.lpips_pinned(vgg_state, heads, xx, y.to(dtype), dec)
                (v * up.to(dtype)).sum().backward()
                res[dtype] = (v.detach(), xx.grad)
            runs[h, w, b] = dict(x=x, y=y, xd=xd, yd=yd, got=got, dec=dec, want=res[torch.float64], cpu32=res[torch.float32])
    return runs


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", MODULE_CASES)
def test_module_against_float64(h, w, b, module_runs, node, device):
    r = module_runs[h, w, b]
    got, xd, yd = r["got"], r["xd"], r["yd"]
    assert got.shape == (b,) and type(got.grad_fn).__name__ == "_LPIPSFunctionBackward"
    assert yd.grad is None and all(p.grad is None and not p.requires_grad for p in node.parameters())
    assert len(r["dec"]) == 13 and all(0 < float(m.float().mean()) < 1 for m, _ in r["dec"])     # every layer alive and masked
    (v64, g64), (v32, g32) = r["want"], r["cpu32"]
    # the yardstick of the case: the worse of its two batch sizes
    yv = max(_value_err(module_runs[h, w, k]["cpu32"][0], module_runs[h, w, k]["want"][0]) for k in (1, 3))
    yg = max(_grad_err(module_runs[h, w, k]["cpu32"][1], module_runs[h, w, k]["want"][1]) for k in (1, 3))
    ev, eg = _value_err(got.detach(), v64), _grad_err(xd.grad, g64)
    print(f"LPIPS {b}x3x{h}x{w}: scores {[f'{v:.5f}' for v in got.tolist()]}, rel err {ev:.2e} (fp32 torch-CPU, worst of the case "
          f"{yv:.2e}); image gradient err / largest entry {eg:.2e} (fp32 torch-CPU {yg:.2e})")
    assert float(v64.min()) > 0 and float(g64.abs().max()) > 0
    assert ev <= 4 * yv
    assert eg <= 4 * yg
    # the no-grad face: the node's value bit for bit; a second run of the node: the same bits
    plain = node(xd.detach(), yd.detach())
    assert plain.grad_fn is None and plain.shape == (b,) and torch.equal(plain, got.detach())
    with torch.no_grad():
        assert torch.equal(node(xd, yd), got.detach())
    x2 = r["x"].to(device).requires_grad_(True)
    again = node(x2, yd.detach())
    (again * _upstream(b).to(device)).sum().backward()
    assert torch.equal(again.detach(), got.detach()) and torch.equal(x2.grad, xd.grad)


def test_module_other_faces(node, vgg_state, heads, device):
    with pytest.raises(ValueError, match="multiples of 16"):
        node(torch.zeros((1, 3, 24, 16), device=device, requires_grad=True), torch.zeros((1, 3, 24, 16), device=device))
    with pytest.raises(ValueError, match="at least 16"):
        node(torch.zeros((1, 3, 8, 16), device=device), torch.zeros((1, 3, 8, 16), device=device))
    # the metric face where planes get odd: the plain table with MaxPool2d's floor.  2e-4 relative: the project's bound for
    # its fp32 convolution stacks against float64, decisions not pinned
    for h, w in ((17, 23), (30, 18), (24, 16)):
        x, y = _images(2, h, w)
        want = LR.lpips_plain(vgg_state, heads, x.double(), y.double())
        got = node(x.to(device), y.to(device))
        err = _value_err(got, want)
        print(f"LPIPS metric face 2x3x{h}x{w}: {got.tolist()}, rel err {err:.2e}")
        assert got.shape == (2,) and got.grad_fn is None and err <= 2e-4
    # float64 on the device: plain torch, differentiable
    x, y = _images(1, 16, 32)
    g64 = node(x.double().to(device).requires_grad_(True), y.double().to(device))
    assert g64.dtype == torch.float64 and type(g64.grad_fn).__name__ != "_LPIPSFunctionBackward"
    assert _value_err(g64.detach(), LR.lpips_plain(vgg_state, heads, x.double(), y.double())) <= 1e-9
    # reductions; the packs are made once
    mean = lpips.LPIPS(vgg_state, heads, reduction="mean").to(device)
    x, y = _images(3, 16, 16)
    assert torch.equal(mean(x.to(device), y.to(device)), node(x.to(device), y.to(device)).mean())
    assert node.packed() is node.packed() and node.packed_transposed() is node.packed_transposed()


# ---- where it plugs in --------------------------------------------------------------------------------------------------
def test_evaluate_image_fills_the_lpips_column(node, device):
    g = torch.Generator().manual_seed(5)
    pred = torch.rand((3, 72, 72), generator=g)
    tgt = (pred + 0.05 * torch.randn((3, 72, 72), generator=g)).clamp(0, 1)
    without = ei.evaluate_image(types.SimpleNamespace(dim=64), pred.to(device), tgt.to(device))
    with_ = ei.evaluate_image(types.SimpleNamespace(dim=64, lpips=node), pred.to(device), tgt.to(device))
    assert math.isnan(without[1]) and with_.shape == (7,)
    c = lambda t: t[:, 4:68, 4:68].unsqueeze(0).contiguous().to(device)
    assert with_[1] == float(node(c(pred), c(tgt))[0]) and with_[1] > 0
    for k in (0, 2, 3, 4, 5, 6):
        assert with_[k] == without[k]
    assert math.isnan(ei.evaluate_image(types.SimpleNamespace(dim=64, lpips=None), pred.to(device), tgt.to(device))[1])


def test_adacof_loss_with_an_lpips_term(vgg_state, heads, device):
    from oracle import nets_cpu
    from vfi_amd.adacof import losses, utility
    from vfi_amd.adacof.models import Model
    model = Model(types.SimpleNamespace(model="vfi_amd.adacof.models.adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    model.load(nets_cpu.adacofnet_random_state_dict(9, kernel_size=5))
    model.train(True)
    g = torch.Generator().manual_seed(4)
    f0, f1, f2 = (torch.rand((2, 3, 64, 64), generator=g).to(device) for _ in range(3))
    crit = losses.Loss(types.SimpleNamespace(loss='1*Charb+0.1*LPIPS', vgg_weights=vgg_state, lpips_weights=heads, gpu_id=0))
    assert [l['type'] for l in crit.loss] == ['Charb', 'LPIPS'] and isinstance(crit.loss_module[1], lpips.LPIPS)
    assert crit.loss_module[1].features[0].weight.device == device
    out = model(f0, f2)
    got = crit(out, f1, [f0, f2])
    frame = out["frame1"].detach().requires_grad_(True)
    term = crit.loss_module[1](frame, f1)
    assert term.dim() == 0 and torch.equal(term.detach(), lpips.LPIPS(vgg_state, heads).to(device)(frame.detach(), f1).mean())
    parts = [1.0 * utility.Module_CharbonnierLoss()(frame, f1), 0.1 * term]
    assert torch.equal(got.detach(), sum(parts).detach())
    got.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert all(p.grad is None for p in crit.parameters())


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


@pytest.mark.parametrize("lpips_weight", [0.1, 0])
def test_fusion_net_trainer_step(lpips_weight, vgg_state, heads, tmp_path, device):
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
    args = types.SimpleNamespace(epochs=1, gpu_id=0, test_paths=None, save=False, lpips_weight=lpips_weight, vgg_weights=vgg_state,
                                 lpips_weights=heads)
    trainer = Trainer(args, loader(), fusion, phase_net, adacof, my_pyr=pyr, lr=lr, out_dir=str(tmp_path / "out"))
    assert (trainer.lpips is None) == (lpips_weight == 0) and trainer.max_step == 1
    trainer.train()
    history = list(trainer.loss_history)
    trainer.close()

    adacof2, ref, pyr2, phase_net2 = _fusion_models(device, h, w)
    ref.train()
    _seed(9)
    opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=0.0)
    term = lpips.LPIPS(vgg_state, heads).to(device) if lpips_weight else None
    manual, l1s = [], []
    for batch in loader():
        inputs = fusion_net_inputs(adacof2, phase_net2, pyr2, batch.lab_frame1, batch.lab_frame2, batch.rgb_frame1, batch.rgb_frame2)
        final = torch.clip(ref(*inputs, variant=0), 0, 1)
        loss = torch.nn.L1Loss()(batch.rgb_target, final)            # the parent's loss
        l1s.append(float(loss.detach()))
        if term is not None:
            loss = loss + lpips_weight * term(final, batch.rgb_target).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        manual.append(float(loss.detach()))
    print(f"lpips_weight {lpips_weight}: loss history {history}, by hand {manual}, its L1 part {l1s}")
    assert len(history) == 1 and math.isfinite(history[0]) and history == manual
    assert (history[0] > l1s[0]) if lpips_weight else (history == l1s)
    for (k, p), (k2, q) in zip(fusion.named_parameters(), ref.named_parameters()):
        assert k == k2 and torch.equal(p, q), k
