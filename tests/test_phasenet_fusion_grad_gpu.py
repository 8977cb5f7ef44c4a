"""Training PhaseNet with three and four input images on the MI355X, through the public surface: the
three adjoints (vfi_phasenet_emit_n_backward, vfi_phasenet_emit_low_n_backward, vfi_phasenet_predict_n_backward) against their
float64 closed forms (tests/phasenet_fusion_grad_ref.py) and the composition, the head adjoint where a block walks a second
tile, the head and blend nodes, the differentiable walk of PhaseNetCore(num_img = 3 | 4) on fixed and on batch statistics
against float64 autograd of its restatement, the unchanged routes, architecture.PhaseNet fed by fusion_img_batch as one training
step, and a short Adam run.

Tolerances are sections 14 / 16's, unchanged.  grad_feat and grad_pred elementwise: 1e-5 * max(1, |ref|max).  Parameter
gradients: relative L2 2e-4 per tensor; a tensor may exceed it only up to 4 x the error float32 torch-CPU autograd of the same
restatement makes against the float64 one.  Conv 1's bias on batch statistics has an exactly zero gradient (the batch's mean
takes its shift out again): float64 autograd gives rounding noise for it, the same rule is applied, and it is the only tensor
left out of the printed worst figure -- which the walk test asserts."""
import functools
import itertools
import math

import pytest
import torch

import phasenet_bn_ref as B
import phasenet_fusion_grad_ref as FG
import phasenet_fusion_ref as FR
import phasenet_grad_ref as R
import phasenet_walk_ref as W
import pyramid_grad_ref as PR
from oracle import pyramid_cpu, synth
from vfi_amd import _lib, ops
from vfi_amd.phase_net import grad as G
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
from vfi_amd.phase_net.core import PhaseNetCore
from vfi_amd.phase_net.phase_net import PhaseNetBlock
from vfi_amd.train.fusion import fusion_img_batch
from vfi_amd.train.loss import get_loss, l1_loss, phase_term
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.train.utils import calc_pyr_height, get_concat_layers_inf, preprocess, separate_vals

pytestmark = pytest.mark.gpu
ZERO_GRADIENT = "feature_map.0.bias"            # on batch statistics only


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _maxerr(a, b):
    return float((torch.as_tensor(a).detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


def _record(fn):
    _lib.PROFILE = rec = _lib.Recorder()
    try:
        out = fn()
    finally:
        _lib.PROFILE = None
    return out, [row[0] for row in rec.rows]


# ---- the three adjoints alone ------------------------------------------------------------------------------------------------
HEAD_SHAPES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 1023: (31, 33), 4100: (41, 100)}
NAN = float("nan")


def _head_case(num_img, n, hw, layout, device, seed=0, shape=None):
    """Operands of the three adjoints, dense; or as channel slices of the real buffers -- pred and f in the (64 + P)-channel
    [feature | pred] buffer, amp_in inside the block input of 64 + P + 8 F channels, grad_pred_in in a slice, the low level's in
    wider holders -- ; or the same buffers starting one float off 16-byte alignment.  grad_phase, grad_amp, grad_low dense.  For
    four images the planes that are never read hold NaN."""
    g = torch.Generator().manual_seed(seed + 100000 * num_img + n * 10000 + hw)
    r = lambda *s: torch.randn(s, generator=g)
    h, w = shape or HEAD_SHAPES[hw]
    pl, pb = FR.pred_channels(num_img)

    def holder(c):
        if layout == "misaligned":
            return torch.empty(n * c * h * w + 1, device=device)[1:].view(n, c, h, w)
        return torch.empty((n, c, h, w), device=device)
    amp, low = torch.rand((n, 4 * num_img, h, w), generator=g), torch.rand((n, num_img, h, w), generator=g) * 2 - 1
    if num_img == 4:
        amp[:, 8:], low[:, 2:] = NAN, NAN
    host = dict(f=r(n, 64, h, w), pred=torch.tanh(r(n, pb, h, w)), amp=amp, gc=r(n, pb, h, w), gp=r(n * 4, 1, h, w),
                ga=r(n * 4, 1, h, w), w=r(pb, 64, 1, 1) / 8, mx=torch.rand(n, generator=g) + 0.5, low=low,
                pred_low=torch.tanh(r(n, pl, h, w)), gl=r(n, 1, h, w), mxl=torch.rand(n, generator=g) + 0.5)
    dev = {k: v.to(device) for k, v in host.items()}
    if layout != "dense":
        c_x = 64 + pb + 8 * num_img
        assert (64 + pb, c_x) == {2: (72, 88), 3: (76, 100), 4: (72, 104)}[num_img]
        fp, x, gb, lo, pl_b = holder(64 + pb), holder(c_x), holder(64 + pb), holder(num_img + 2), holder(64 + pl)
        a0 = 64 + 4 * num_img                      # the reference's order [feature | phase | amp | prediction]
        fp[:, :64], fp[:, 64:], x[:, a0:a0 + 4 * num_img], gb[:, 64:] = dev["f"], dev["pred"], dev["amp"], dev["gc"]
        lo[:, 1:1 + num_img], pl_b[:, 64:] = dev["low"], dev["pred_low"]
        dev.update(f=fp[:, :64], pred=fp[:, 64:], amp=x[:, a0:a0 + 4 * num_img], gc=gb[:, 64:], low=lo[:, 1:1 + num_img],
                   pred_low=pl_b[:, 64:])
        if layout == "misaligned":
            assert dev["f"].data_ptr() % 16 != 0
    return host, dev


def _head_model(host, num_img, gp, ga, gc):
    d = lambda t: t.double()
    n, _, h, w = host["f"].shape
    g4 = lambda t: d(t).reshape(n, 4, h, w)
    return FG.head_backward(d(host["f"]), d(host["pred"]), d(host["amp"]), d(host["mx"]), d(host["w"]).view(-1, 64), num_img,
                            g4(host["gp"]) if gp else None, g4(host["ga"]) if ga else None, d(host["gc"]) if gc else None)


def _head_call(dev, num_img, up, **kw):
    return ops.phasenet_predict_n_backward(dev["f"], dev["pred"], dev["amp"], dev["mx"], dev["w"], num_img, *up, **kw)


@pytest.mark.parametrize("num_img", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_head_adjoint_against_float64_and_the_composition(hw, n, num_img, device):
    worst = 0.0
    pb = FR.pred_channels(num_img)[1]
    for layout in ("dense", "slices", "misaligned"):
        host, dev = _head_case(num_img, n, hw, layout, device)
        for gp, ga, gc in itertools.product((True, False), repeat=3):
            up = (dev["gp"] if gp else None, dev["ga"] if ga else None, dev["gc"] if gc else None)
            gf, gw, gb = _head_call(dev, num_img, up)
            wf, ww, wb = _head_model(host, num_img, gp, ga, gc)
            assert gw.shape == (pb, 64, 1, 1) and gb.shape == (pb,)
            err = _maxerr(gf, wf)
            worst = max(worst, err)
            assert err <= 1e-5 * max(1.0, float(wf.abs().max())), (layout, gp, ga, gc, err)
            if gp or ga or gc:
                assert _rel(gw.view(pb, 64), ww) <= 2e-4 and _rel(gb, wb) <= 2e-4, (layout, gp, ga, gc)
                cf, cw, cb = G.head_backward_composed(dev["f"], dev["pred"], dev["amp"], dev["mx"], dev["w"], *up, num_img=num_img)
                assert _rel(gw, cw) <= 2e-4 and _rel(gb, cb) <= 2e-4 and _maxerr(gf, cf) <= 1e-5 * max(1.0, float(wf.abs().max()))
            else:
                assert not bool(gf.any()) and not bool(gw.any()) and not bool(gb.any())
            again = _head_call(dev, num_img, up)
            assert all(torch.equal(a, b) for a, b in zip((gf, gw, gb), again)), "two runs differ"
            if num_img != 3:        # the two-image entry point itself, on the first eight amplitude planes
                two = ops.phasenet_predict_backward(dev["f"], dev["pred"], dev["amp"][:, :8], dev["mx"], dev["w"], *up)
                assert all(torch.equal(a, b) for a, b in zip((gf, gw, gb), two)), (layout, gp, ga, gc)
    print(f"head adjoint num_img={num_img} N={n} HW={hw}: worst |grad_f error| {worst:.3e}")


@pytest.mark.parametrize("num_img", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_emit_adjoints_against_float64(hw, n, num_img, device):
    worst = 0.0
    h, w = HEAD_SHAPES[hw]
    d = lambda t: t.double()
    for layout in ("dense", "slices", "misaligned"):
        host, dev = _head_case(num_img, n, hw, layout, device, seed=1)
        for gp, ga in ((True, True), (True, False), (False, True)):
            up = (dev["gp"] if gp else None, dev["ga"] if ga else None)
            got = ops.phasenet_emit_n_backward(*up, dev["pred"], dev["amp"], dev["mx"], num_img)
            want = FG.emit_n_backward(d(host["gp"]).view(n, 4, h, w) if gp else None, d(host["ga"]).view(n, 4, h, w) if ga else None,
                                      d(host["pred"]), d(host["amp"]), d(host["mx"]), num_img)
            err = _maxerr(got, want)
            worst = max(worst, err)
            assert got.shape == want.shape and err <= 1e-5 * max(1.0, float(want.abs().max())), (layout, gp, ga, err)
            assert torch.equal(got, ops.phasenet_emit_n_backward(*up, dev["pred"], dev["amp"], dev["mx"], num_img))
            if num_img != 3:
                assert torch.equal(got, ops.phasenet_emit_backward(*up, dev["amp"][:, :8], dev["mx"]))
        with pytest.raises(_lib.VfiLibraryError):
            ops.phasenet_emit_n_backward(None, None, dev["pred"], dev["amp"], dev["mx"], num_img)
        got = ops.phasenet_emit_low_n_backward(dev["gl"], dev["pred_low"], dev["low"], dev["mxl"], num_img)
        want = FG.emit_low_n_backward(d(host["gl"]), d(host["pred_low"]), d(host["low"]), d(host["mxl"]), num_img)
        err = _maxerr(got, want)
        worst = max(worst, err)
        assert got.shape == want.shape and err <= 1e-5 * max(1.0, float(want.abs().max())), (layout, err)
        assert torch.equal(got, ops.phasenet_emit_low_n_backward(dev["gl"], dev["pred_low"], dev["low"], dev["mxl"], num_img))
        if num_img != 3:
            assert torch.equal(got, ops.phasenet_emit_low_backward(dev["gl"], dev["low"][:, :2], dev["mxl"]))
    print(f"emit adjoints num_img={num_img} N={n} HW={hw}: worst |grad_pred error| {worst:.3e}")


@pytest.mark.parametrize("num_img", [3, 4])
def test_adjoint_output_subsets_and_out_slices(num_img, device):
    host, dev = _head_case(num_img, 3, 1023, "slices", device, seed=3)
    up = (dev["gp"], dev["ga"], dev["gc"])
    full = _head_call(dev, num_img, up)
    for nf, nw, nb in itertools.product((True, False), repeat=3):
        if not (nf or nw or nb):
            with pytest.raises(_lib.VfiLibraryError):
                _head_call(dev, num_img, up, need_feat=False, need_weight=False, need_bias=False)
            continue
        got = _head_call(dev, num_img, up, need_feat=nf, need_weight=nw, need_bias=nb)
        for a, b, need in zip(got, full, (nf, nw, nb)):
            assert (a is None) if not need else torch.equal(a, b)
    big = torch.full((3, 70, 31, 33), 7.0, device=device)          # grad_f written into a channel slice, nothing beside it
    _head_call(dev, num_img, up, need_weight=False, need_bias=False, out=big[:, 3:67])
    assert torch.equal(big[:, 3:67], full[0]) and bool((big[:, :3] == 7.0).all()) and bool((big[:, 67:] == 7.0).all())
    pl, pb = FR.pred_channels(num_img)
    big = torch.full((3, pb + 5, 31, 33), 7.0, device=device)
    want = ops.phasenet_emit_n_backward(dev["gp"], dev["ga"], dev["pred"], dev["amp"], dev["mx"], num_img)
    ops.phasenet_emit_n_backward(dev["gp"], dev["ga"], dev["pred"], dev["amp"], dev["mx"], num_img, out=big[:, 2:2 + pb])
    assert torch.equal(big[:, 2:2 + pb], want) and bool((big[:, :2] == 7.0).all()) and bool((big[:, 2 + pb:] == 7.0).all())
    big = torch.full((3, pl + 5, 31, 33), 7.0, device=device)
    want = ops.phasenet_emit_low_n_backward(dev["gl"], dev["pred_low"], dev["low"], dev["mxl"], num_img)
    ops.phasenet_emit_low_n_backward(dev["gl"], dev["pred_low"], dev["low"], dev["mxl"], num_img, out=big[:, 2:2 + pl])
    assert torch.equal(big[:, 2:2 + pl], want) and bool((big[:, :2] == 7.0).all()) and bool((big[:, 2 + pl:] == 7.0).all())


@pytest.mark.parametrize("num_img", [2, 3, 4])
def test_saturated_predictions_give_zero_gz(num_img, device):
    host, dev = _head_case(num_img, 3, 1023, "dense", device, seed=5)
    dev["pred"] = torch.where(dev["pred"] > 0, 1.0, -1.0)
    gf, gw, gb = _head_call(dev, num_img, (dev["gp"], dev["ga"], dev["gc"]))
    assert not bool(gf.any()) and not bool(gw.any()) and not bool(gb.any())


@pytest.mark.parametrize("num_img", [2, 3])
@pytest.mark.parametrize("shape", [(210, 211), (212, 209)])
def test_head_adjoint_where_a_block_walks_a_second_tile(shape, num_img, device):
    """1024 block partials at most and 128-pixel tiles: with N * ceil(HW / 128) = 3 * 347 = 1041 tiles, blocks 0..16 take a second
    tile -- in another sample -- and carry their accumulators across the leading barrier.  210 x 211 takes the 4-byte path,
    212 x 209 the 16-byte one."""
    n, (h, w) = 3, shape
    assert n * -(-(h * w) // 128) == 1041 and ((h * w) % 4 == 0) == (shape == (212, 209))
    host, dev = _head_case(num_img, n, h * w, "dense", device, seed=7, shape=shape)
    up = (dev["gp"], dev["ga"], dev["gc"])
    gf, gw, gb = _head_call(dev, num_img, up)
    wf, ww, wb = _head_model(host, num_img, True, True, True)
    err = _maxerr(gf, wf)
    print(f"second tile num_img={num_img} {h}x{w}: |grad_f error| {err:.3e}, grad_w relative L2 {_rel(gw.view(-1, 64), ww):.3e}, "
          f"grad_b {_rel(gb, wb):.3e}")
    assert err <= 1e-5 * max(1.0, float(wf.abs().max()))
    assert _rel(gw.view(-1, 64), ww) <= 2e-4 and _rel(gb, wb) <= 2e-4
    assert all(torch.equal(a, b) for a, b in zip((gf, gw, gb), _head_call(dev, num_img, up))), "two runs differ"


# ---- the nodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [3, 4])
def test_head_and_blend_nodes(num_img, device):
    pl, pb = FR.pred_channels(num_img)
    cin = 64 + pb + 8 * num_img
    sd = R.block_state(4, cin, pb, 3)
    blk = PhaseNetBlock(cin, 64, pb, (3, 3)).to(device)
    blk.load_state_dict(sd)
    pm = blk.prediction_map[0]
    for h, w in ((9, 13), (40, 104)):               # conv + emit inside the library, and the streaming kernel
        g = torch.Generator().manual_seed(h)
        f, amp = torch.randn((3, 64, h, w), generator=g).to(device), torch.rand((3, 4 * num_img, h, w), generator=g).to(device)
        mx = (torch.rand(3, generator=g) + 0.5).to(device)
        gp, ga, gc = (torch.randn(s, generator=g).to(device) for s in ((12, 1, h, w), (12, 1, h, w), (3, pb, h, w)))
        want = ops.phasenet_predict_n(f, ops.PackedConv(pm.weight, pm.bias), amp, mx, num_img)
        fd = f.clone().requires_grad_(True)
        (got, calls) = _record(lambda: G.level_head(blk, fd, amp, mx, num_img))
        assert calls.count("vfi_phasenet_predict_n") == 1 and all(o.grad_fn is not None for o in got)
        assert all(torch.equal(a.detach(), b) for a, b in zip(got, want))
        with torch.no_grad():
            plain = G.level_head(blk, fd, amp, mx, num_img)
        assert all(o.grad_fn is None and torch.equal(o, b) for o, b in zip(plain, want))
        ((got[0] * gc).sum() + (got[1] * gp).sum() + (got[2] * ga).sum()).backward()
        df, dw, db = ops.phasenet_predict_n_backward(f, want[0], amp, mx, pm.weight, num_img, gp, ga, gc)
        direct = (df, dw, db)
        if not (G.HEAD_ONE_PASS and (G.HEAD_ONE_PASS_THREE or num_img != 3)):      # the route the walk takes, called directly
            direct = G.head_backward_composed(f, want[0], amp, mx, pm.weight, gp, ga, gc, num_img=num_img)
        assert all(torch.equal(a, b) for a, b in zip((fd.grad, pm.weight.grad, pm.bias.grad), direct))
        for one_pass in (False, True):              # both routes of the node give the composition's / the kernel's values
            G.HEAD_ONE_PASS_THREE, keep = one_pass, G.HEAD_ONE_PASS_THREE
            try:
                fd2 = f.clone().requires_grad_(True)
                out, calls = _record(lambda: G.level_head(blk, fd2, amp, mx, num_img))
                _, back = _record(lambda: ((out[0] * gc).sum() + (out[1] * gp).sum() + (out[2] * ga).sum()).backward())
            finally:
                G.HEAD_ONE_PASS_THREE = keep
            composed = num_img == 3 and not one_pass
            assert ("vfi_phasenet_emit_n_backward" in back) == composed and ("vfi_phasenet_predict_n_backward" in back) != composed
            assert _maxerr(fd2.grad, df) <= 1e-5 * max(1.0, float(df.abs().max()))
        blk.zero_grad(set_to_none=True)
        # the blends on their own
        pred = want[0].clone().requires_grad_(True)
        ph, am = G.blend_level(pred, amp, mx, num_img)
        assert torch.equal(ph.detach(), want[1]) and torch.equal(am.detach(), want[2])
        ((ph * gp).sum() + (am * ga).sum()).backward()
        assert torch.equal(pred.grad, ops.phasenet_emit_n_backward(gp, ga, want[0], amp, mx, num_img))
        low_in, pred_low = torch.rand((3, num_img, h, w), generator=g).to(device), torch.tanh(torch.randn((3, pl, h, w), generator=g)).to(device)
        gl = torch.randn((3, 1, h, w), generator=g).to(device)
        pd = pred_low.clone().requires_grad_(True)
        low = G.blend_low(pd, low_in, mx, num_img)
        assert torch.equal(low.detach(), ops.phasenet_emit_low_n(pred_low, low_in, mx, num_img))
        (low * gl).sum().backward()
        assert torch.equal(pd.grad, ops.phasenet_emit_low_n_backward(gl, pred_low, low_in, mx, num_img))


# ---- the whole walk ----------------------------------------------------------------------------------------------------------
WALKS = {"65x77": (65, 77, 9, None, "seeded"), "128x160": (128, 160, 10, None, "trained"), "128x160-m4": (128, 160, 10, 4, "seeded")}
N_WALK = 3


def _state(kind, num_img):
    return FR.net_state(31, num_img) if kind == "seeded" else FR.trained_like_state(31, num_img)


def _core(sd, height, num_img, device, batch_stats=False):
    core = PhaseNetCore(height, device, num_img=num_img).fine_tune(fusion=True, batch_stats=batch_stats)
    core.load_state_dict(sd)
    return core


def _lab_like_images(seed, count, h, w, device):
    """`count` channel-images with the textures of synth.translating_pair, each shifted differently."""
    imgs = [torch.from_numpy(synth.translating_pair(seed + i, h, w, shift=(1.5 + i, -0.75 * i))[i % 3]) for i in range((count + 2) // 3)]
    return torch.cat(imgs, 0)[:count].contiguous().to(device)


def _normalised(core, h, w, height, device, n=N_WALK):
    """Normalised values of a real analysis of n * num_img Lab-like images (n = 3: a frame's three channels), the fused route
    of architecture.PhaseNet.forward: (values, walk inputs on the host)."""
    imgs = _lab_like_images(3, n * core.num_img, h, w, device)
    pyr = Pyramid(height=height, nbands=4, scale_factor=W.S2, device=device)
    vals, bufs = pyr.filter(imgs, concat_frames=core.num_img, phase_scale=1.0 / math.pi, pred_channels=core.pred_channels)
    nv = core.normalize_vals(vals, concat=bufs)
    c = lambda t: t.detach().cpu().clone()
    inp = {"low": c(nv.low_level), "max_low": c(core.max_low_level), "phase": [c(p) for p in nv.phase],
           "amp": [c(a) for a in nv.amplitude], "max_amp": [c(x) for x in core.max_amplitudes]}
    return nv, inp


@functools.lru_cache(maxsize=None)
def _walk_reference(name, num_img, bn, dev):
    """float64 and float32 torch-CPU autograd of the restated walk, computed once per configuration and left unchanged."""
    h, w, height, m, kind = WALKS[name]
    sd = _state(kind, num_img)
    _, inp = _normalised(_core(sd, height, num_img, dev), h, w, height, dev)
    m_ = height - 2 if m is None else m
    walk = FG.bn_walk if bn else FG.walk
    out = {}
    for dtype in (torch.float64, torch.float32):
        P = FG.net_params(sd, dtype)
        low, phases, amps = walk(P, W.to_dtype(inp, dtype), m_, num_img)
        if dtype == torch.float64:
            tgt = W.walk_targets(17, low, phases, amps)
            out["outputs"] = (low.detach(), [p.detach() for p in phases], [a.detach() for a in amps])
            out["buffers"] = {k: v.clone() for k, v in B.named_buffers(P).items()}
        W.walk_loss(low, phases, amps, W.to_dtype(tgt, dtype)).backward()
        out[dtype] = W.named_grads(P)
    return sd, tgt, out


def _hip_walk(core, nv, m, tgt, device):
    vals = core(nv, m)
    L = core.height - 2
    m_ = L if m is None else m
    phases, amps = list(vals.phase[::-1][:m_]), list(vals.amplitude[::-1][:m_])          # coarsest first
    t = W.to_dtype(tgt, torch.float32, device)
    loss = W.walk_loss(vals.low_level, phases, amps, t, phase_term=lambda o, tt: phase_term(o, tt, 4), l1=l1_loss)
    return vals, (vals.low_level, phases, amps), loss


@pytest.mark.parametrize("bn", [False, True], ids=["fixed", "batch"])
@pytest.mark.parametrize("num_img", [3, 4])
@pytest.mark.parametrize("name", list(WALKS))
def test_walk_gradients_match_float64_autograd(name, num_img, bn, device):
    h, w, height, m, kind = WALKS[name]
    sd, tgt, ref = _walk_reference(name, num_img, bn, device)
    core = _core(sd, height, num_img, device, batch_stats=bn)
    assert core.fine_tuning and core.batch_stats == bn and all(b.batch_stats == bn for b in core.layers) and not core.training
    nv, _ = _normalised(core, h, w, height, device)
    assert nv.low_level.shape[:2] == (N_WALK, num_img) and nv.amplitude[0].shape[1] == 4 * num_img
    vals, (low, phases, amps), loss = _hip_walk(core, nv, m, tgt, device)
    assert low.grad_fn is not None and all(p.grad_fn is not None for p in phases + amps)
    L = height - 2
    m_ = L if m is None else m
    assert len(vals.phase) == L and all(not torch.is_tensor(p) for p in vals.phase[:L - len(phases)])
    assert vals.high_level.shape[1] == 1 and not bool(vals.high_level.any())
    rl, rp, ra = ref["outputs"]
    for got, want in zip([low] + phases + amps, [rl] + rp + ra):
        assert _rel(got.detach(), want) <= 2e-4
    loss.backward()
    worst, left_out = (0.0, None), []
    for k, p in core.named_parameters():
        want, lost = ref[torch.float64][k], ref[torch.float32][k]
        if want is None:
            assert p.grad is None, f"{k}: a block above level m must get None, not zeros"
            continue
        assert p.grad is not None, k
        err, lost32 = _rel(p.grad, want), _rel(lost, want)
        if bn and k.endswith(ZERO_GRADIENT):
            left_out.append(k)
        else:
            worst = max(worst, (err, k))
        assert err <= max(2e-4, 4 * lost32), (k, err, lost32)
    # only conv 1's bias on batch statistics is left out of the relative measure, in the blocks that ran
    assert left_out == ([f"layers.{i}.{ZERO_GRADIENT}" for i in range(min(m_, 7) + 1)] if bn else [])
    print(f"fusion walk num_img={num_img} {name} ({kind}, {'batch' if bn else 'fixed'} statistics): worst per-tensor relative L2 "
          f"{worst[0]:.3e} ({worst[1]})")
    if m is not None:
        assert all(p.grad is None for k, p in core.named_parameters() if int(k.split(".")[1]) > m)
    buffers = dict(core.named_buffers())
    for k, want in ref["buffers"].items():
        i = int(k.split(".")[1])
        if k.endswith("num_batches_tracked"):
            served = 0 if (not bn or i > m_) else (max(1, m_ - 6) if i == 7 else 1)
            assert int(buffers[k]) == int(want) == served, k
        elif not bn or i > m_:
            assert torch.equal(buffers[k].cpu(), sd[k]), k
        else:
            assert _rel(buffers[k], want) <= 2e-4, (k, _rel(buffers[k], want))


# ---- the unchanged routes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [3, 4])
def test_fusion_network_without_the_switch_runs_the_inference_route(num_img, device):
    name = "65x77"
    h, w, height, m, kind = WALKS[name]
    sd = _state(kind, num_img)
    core = PhaseNetCore(height, device, num_img=num_img)
    core.load_state_dict(sd)
    nv, _ = _normalised(core, h, w, height, device)
    flat = lambda v: [v.low_level, v.high_level] + list(v.phase) + list(v.amplitude)
    with torch.no_grad():
        core(nv, m)                                              # builds the inference packs, once
        base, calls = _record(lambda: core(nv, m))
    assert calls.count("vfi_phasenet_predict_n") == height - 2 and calls.count("vfi_phasenet_emit_low_n") == 1
    plain, calls_plain = _record(lambda: core(nv, m))            # grad mode on, parameters require grad, never switched
    assert calls_plain == calls and all(a.grad_fn is None and torch.equal(a, b) for a, b in zip(flat(plain), flat(base)))
    core.fine_tune(fusion=True)
    with torch.no_grad():
        off, calls_off = _record(lambda: core(nv, m))            # switched, grad mode off
    assert calls_off == calls and all(torch.equal(a, b) for a, b in zip(flat(off), flat(base)))
    for p in core.parameters():
        p.requires_grad_(False)
    frozen, calls_frozen = _record(lambda: core(nv, m))          # switched, grad mode on, nothing requires grad
    assert calls_frozen == calls and all(a.grad_fn is None and torch.equal(a, b) for a, b in zip(flat(frozen), flat(base)))
    for p in core.parameters():
        p.requires_grad_(True)
    vals, calls_grad = _record(lambda: core(nv, m))              # the grad route: the same head launch per level
    assert calls_grad.count("vfi_phasenet_predict_n") == height - 2 and calls_grad.count("vfi_phasenet_emit_low_n") == 1
    assert vals.low_level.grad_fn is not None
    for a, b in zip(flat(vals), flat(base)):
        assert _rel(a.detach(), b) <= 2e-4
    core.fine_tune(False)
    again, calls_again = _record(lambda: core(nv, m))
    assert calls_again == calls and all(a.grad_fn is None and torch.equal(a, b) for a, b in zip(flat(again), flat(base)))


def test_two_image_fine_tuning_issues_the_calls_it_always_did(device):
    h, w, height = 65, 77, 9
    core = PhaseNetCore(height, device).fine_tune()
    core.load_state_dict(W.net_state(31))
    a0, _, a2 = (torch.from_numpy(x) for x in synth.translating_pair(3, h, w))
    pyr = Pyramid(height=height, nbands=4, scale_factor=W.S2, device=device)
    vals, bufs = pyr.filter(torch.cat((a0, a2), 0).to(device), concat_frames=2, phase_scale=1.0 / math.pi)
    nv = core.normalize_vals(vals, concat=bufs)
    out, fwd = _record(lambda: core(nv, None))
    loss = out.low_level.abs().mean() + sum(p.abs().mean() + a.abs().mean() for p, a in zip(out.phase, out.amplitude))
    _, bwd = _record(loss.backward)
    L = height - 2
    assert fwd.count("vfi_phasenet_predict") == L and fwd.count("vfi_phasenet_emit_low") == 1
    assert bwd.count("vfi_phasenet_predict_backward") == L and bwd.count("vfi_phasenet_emit_low_backward") == 1
    new = {"vfi_phasenet_predict_n", "vfi_phasenet_emit_n", "vfi_phasenet_emit_low_n", "vfi_phasenet_predict_n_backward",
           "vfi_phasenet_emit_n_backward", "vfi_phasenet_emit_low_n_backward"}
    assert not new & set(fwd + bwd)
    assert "vfi_phasenet_emit_backward" not in bwd and "vfi_act_backward" in bwd       # one pass for the head; ELU for the features
    # the fusion keyword changes nothing for two images
    core2 = PhaseNetCore(height, device).fine_tune(fusion=True)
    core2.load_state_dict(W.net_state(31))
    core2.max_amplitudes, core2.max_low_level = core.max_amplitudes, core.max_low_level
    out2, fwd2 = _record(lambda: core2(nv, None))
    assert fwd2 == fwd and torch.equal(out2.low_level.detach(), out.low_level.detach())


# ---- architecture.PhaseNet -----------------------------------------------------------------------------------------------------
def _stand_in_adacof(seed):
    """A seeded stand-in for AdaCoF: (frame 1 warped, frame 2 warped, their blend, a mask) from rolls and a fixed blend."""
    g = torch.Generator().manual_seed(seed)
    a = float(torch.rand(1, generator=g)) * 0.4 + 0.3

    def model(f1, f2):
        assert not torch.is_grad_enabled()
        w1, w2 = torch.roll(f1, (1, -2), (2, 3)) * 0.9 + 0.05, torch.roll(f2, (-1, 1), (2, 3)) * 0.9 + 0.05
        return w1, w2, (a * w1 + (1 - a) * w2).clamp(0, 1), None
    return model


@pytest.mark.parametrize("m", [3, None])
@pytest.mark.parametrize("num_img", [3, 4])
def test_architecture_forward_is_one_training_step(num_img, m, device):
    h, w = 64, 96
    height = calc_pyr_height(torch.empty(3, h, w, device="meta"))
    L = height - 2
    a0, a1, a2 = (torch.from_numpy(x).to(device) for x in synth.translating_pair(5, h, w))
    rgb1, rgb2 = a0.unsqueeze(0), a2.unsqueeze(0)
    lab1, lab2, target = (preprocess(x.unsqueeze(0), device) for x in (a0, a2, a1))
    img_batch = fusion_img_batch(_stand_in_adacof(3), lab1, lab2, rgb1, rgb2, target, num_img)
    assert img_batch.shape == (3 * (num_img + 1), h, w) and torch.equal(img_batch[-3:], target) and torch.equal(img_batch[:3], lab1)
    net = ArchPhaseNet(height, device, num_img=num_img)
    sd = FR.net_state(41, num_img)
    net.core.load_state_dict(sd)
    fed = img_batch if m is not None else img_batch[:-3]            # the fused route takes the inputs alone
    assert net(fed, m=m)[0].grad_fn is None                         # not asked to train: no graph
    with pytest.raises(NotImplementedError, match="training of the fusion variants"):
        net.fine_tune()
    assert net.fine_tune(fusion=True) is net and net.core.fine_tuning
    with torch.no_grad():
        assert net(fed, m=m)[0].grad_fn is None
    prediction, vals_pred, vals_target = net(fed, m=m)
    assert prediction.requires_grad and prediction.grad_fn is not None
    with torch.no_grad():
        vals_list = separate_vals(net.pyr.filter(img_batch), num_img + 1)
        cat = get_concat_layers_inf(net.pyr, vals_list[:-1])
    tgt_v = vals_list[-1]
    if m is None:
        assert vals_target is None
        vals_target = tgt_v
    total = get_loss(vals_pred, vals_target, prediction, target, net.pyr)[0]
    total.backward()

    # float64 restatement of architecture.py:38-71 fed the product's analysis outputs
    d = lambda t: t.detach().cpu().double()
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    m_ = L if m is None else m

    def restated(dtype):
        P = FG.net_params(sd, dtype)
        c = lambda t: d(t).to(dtype)
        inp = FR.normalize({"low": c(cat.low_level), "phase": [c(p) for p in cat.phase], "amp": [c(a) for a in cat.amplitude]})
        low, phases, amps = FG.walk(P, inp, m_, num_img)
        ph, am = [0] * (L - m_) + phases[::-1], [0] * (L - m_) + amps[::-1]        # finest first
        if m is not None:
            for k in range(0, min(height - m, L)):                               # exchange_vals(.., 0, calc_pyr_height - m)
                ph[k], am[k] = c(tgt_v.phase[k]), c(tgt_v.amplitude[k])
        high = torch.zeros((3, 1, h, w), dtype=torch.float64)
        out = PR.reconstruct64(spec, PR.polar_to_coeff(high, [p.double() for p in ph], [a.double() for a in am], low.double()))
        loss = R.get_loss(ph, [c(p) for p in tgt_v.phase], out.to(dtype), c(target), 4)[0]
        loss.backward()
        return loss.detach(), W.named_grads(P)
    l64, g64 = restated(torch.float64)
    _, g32 = restated(torch.float32)
    print(f"architecture step num_img={num_img} m={m}: loss {float(total.detach()):.7f} (float64 {float(l64):.7f})")
    assert abs(float(total.detach()) - float(l64)) <= 1e-4 * abs(float(l64))
    used, worst = 0, (0.0, None)
    for k, p in net.core.named_parameters():
        if g64[k] is None:
            assert p.grad is None, k
            continue
        used += 1
        assert p.grad is not None, k
        err, lost32 = _rel(p.grad, g64[k]), _rel(g32[k], g64[k])
        worst = max(worst, (err, k))
        assert err <= max(2e-4, 4 * lost32), (k, err, lost32)
    assert used >= (8 * 7 if m is None else 8 * 2)
    print(f"architecture step num_img={num_img} m={m}: {used} tensors, worst relative L2 {worst[0]:.3e} ({worst[1]})")


# ---- a short run ---------------------------------------------------------------------------------------------------------------
def test_training_run_of_the_three_image_network_tracks_float64(device):
    h, w, height, num_img = 65, 77, 9, 3
    torch.manual_seed(7)
    sd = {k: v.detach().cpu().clone() for k, v in PhaseNetCore(height, device, num_img=num_img).state_dict().items()}      # a new module's own initialisation
    core = _core(sd, height, num_img, device, batch_stats=True)
    nv, inp = _normalised(core, h, w, height, device, n=1)
    L = height - 2
    P = FG.net_params(sd)
    d64 = W.to_dtype(inp)
    low, phases, amps = FG.bn_walk(FG.net_params(sd), d64, L, num_img)
    tgt = W.walk_targets(19, low, phases, amps)
    t64 = W.to_dtype(tgt)

    def run(params, step_loss, steps=30):
        opt = torch.optim.Adam(params, lr=1e-3)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            val = step_loss()
            val.backward()
            opt.step()
            losses.append(float(val.detach()))
        return losses
    key0 = G.block_packs_raw(core.layers[7])["key"]
    gpu = run(list(core.parameters()), lambda: _hip_walk(core, nv, None, tgt, device)[2])
    assert G.block_packs_raw(core.layers[7])["key"] != key0        # the pack caches follow opt.step()
    cpu = run([P[i][k] for i in range(8) for k in R.BLOCK_KEYS], lambda: W.walk_loss(*FG.bn_walk(P, d64, L, num_img), t64))
    print("Adam run, three images on batch statistics, HIP :", " ".join(f"{v:.5f}" for v in gpu))
    print("Adam run, three images on batch statistics, CPU :", " ".join(f"{v:.5f}" for v in cpu))
    assert gpu[-1] < gpu[0], gpu
    for a, b in zip(gpu, cpu):
        assert abs(a - b) <= 0.02 * abs(b), (gpu, cpu)
    assert all(int(b.feature_map[1].num_batches_tracked) == 30 for b in core.layers)
