"""Fine-tuning the whole PhaseNet on the MI355X, through the public surface: the one-pass head adjoint
(vfi_phasenet_predict_backward) against its float64 model and the five-launch composition, the head node, the differentiable
coarse-to-fine walk of PhaseNetCore against float64 autograd of its restatement (tests/phasenet_walk_ref.py), the unchanged
no-grad route, architecture.PhaseNet's hierarchical form as one training step, and a short Adam run.

Tolerance of parameter gradients: relative L2 2e-4 per tensor; a tensor may exceed it only up to 4 x the error float32
torch-CPU autograd of the same restatement makes against the float64 one (section 14's rule, unchanged)."""
import functools
import itertools
import math

import pytest
import torch

import phasenet_grad_ref as R
import phasenet_walk_ref as W
import pyramid_grad_ref as PR
import trained_stats
from oracle import pyramid_cpu, synth
from vfi_amd import _lib, ops
from vfi_amd.phase_net import grad as G
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
from vfi_amd.phase_net.core import PhaseNetCore
from vfi_amd.phase_net.phase_net import PhaseNetBlock
from vfi_amd.train.loss import get_loss, l1_loss, phase_term
from vfi_amd.train.utils import get_concat_layers_inf, separate_vals

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _maxerr(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


# ---- the head adjoint alone --------------------------------------------------------------------------------------------
HEAD_SHAPES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 1023: (31, 33), 4100: (41, 100)}


def _head_case(n, hw, layout, device, seed=0):
    """f, pred (post-tanh), amp_in, grad_pred_in as dense tensors, as channel slices of 72- / 20-channel buffers, or as slices
    of buffers that start one float off 16-byte alignment; (grad_phase, grad_amp) dense."""
    g = torch.Generator().manual_seed(seed + n * 10000 + hw)
    r = lambda *s: torch.randn(s, generator=g)
    h, w = HEAD_SHAPES[hw]

    def holder(c):
        if layout == "misaligned":
            return torch.empty(n * c * hw + 1, device=device)[1:].view(n, c, h, w)
        return torch.empty((n, c, h, w), device=device)
    f, pred = r(n, 64, h, w), torch.tanh(r(n, 8, h, w))
    amp, gc = torch.rand((n, 8, h, w), generator=g), r(n, 8, h, w)
    host = dict(f=f, pred=pred, amp=amp, gc=gc, gp=r(n * 4, 1, h, w), ga=r(n * 4, 1, h, w), w=r(8, 64, 1, 1) / 8,
                mx=torch.rand(n, generator=g) + 0.5)
    dev = {k: v.to(device) for k, v in host.items()}
    if layout != "dense":
        fp, ab, gb = holder(72), holder(20), holder(72)
        fp[:, :64], fp[:, 64:], ab[:, 11:19], gb[:, 64:] = dev["f"], dev["pred"], dev["amp"], dev["gc"]
        dev.update(f=fp[:, :64], pred=fp[:, 64:], amp=ab[:, 11:19], gc=gb[:, 64:])
        if layout == "misaligned":
            assert dev["f"].data_ptr() % 16 != 0
    return host, dev


def _head_model(host, gp, ga, gc):
    d = lambda t: t.double()
    n, _, h, w = host["f"].shape
    g4 = lambda t: d(t).reshape(n, 4, h, w)
    return W.head_backward(d(host["f"]), d(host["pred"]), d(host["amp"]), d(host["mx"]), d(host["w"]).view(8, 64),
                           g4(host["gp"]) if gp else None, g4(host["ga"]) if ga else None, d(host["gc"]) if gc else None)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_head_adjoint_against_float64_and_the_composition(hw, n, device):
    worst = 0.0
    for layout in ("dense", "slices", "misaligned"):
        host, dev = _head_case(n, hw, layout, device)
        for gp, ga, gc in itertools.product((True, False), repeat=3):
            up = (dev["gp"] if gp else None, dev["ga"] if ga else None, dev["gc"] if gc else None)
            gf, gw, gb = ops.phasenet_predict_backward(dev["f"], dev["pred"], dev["amp"], dev["mx"], dev["w"], *up)
            wf, ww, wb = _head_model(host, gp, ga, gc)
            # elementwise, section 14's bound for the blend adjoints, on sums of eight such terms
            err = _maxerr(gf, wf)
            worst = max(worst, err)
            assert err <= 1e-5 * max(1.0, float(wf.abs().max())), (layout, gp, ga, gc, err)
            if gp or ga or gc:
                assert _rel(gw.view(8, 64), ww) <= 2e-4 and _rel(gb, wb) <= 2e-4, (layout, gp, ga, gc)
                cf, cw, cb = G.head_backward_composed(dev["f"], dev["pred"], dev["amp"], dev["mx"], dev["w"], *up)
                assert _rel(gw, cw) <= 2e-4 and _rel(gb, cb) <= 2e-4 and _maxerr(gf, cf) <= 1e-5 * max(1.0, float(wf.abs().max()))
            else:
                assert not bool(gf.any()) and not bool(gw.any()) and not bool(gb.any())
            again = ops.phasenet_predict_backward(dev["f"], dev["pred"], dev["amp"], dev["mx"], dev["w"], *up)
            assert all(torch.equal(a, b) for a, b in zip((gf, gw, gb), again)), "two runs differ"
    print(f"head adjoint N={n} HW={hw}: worst |grad_f error| {worst:.3e}")


def test_head_adjoint_output_subsets_and_out_slice(device):
    host, dev = _head_case(3, 1023, "slices", device, seed=3)
    args = (dev["f"], dev["pred"], dev["amp"], dev["mx"], dev["w"], dev["gp"], dev["ga"], dev["gc"])
    full = ops.phasenet_predict_backward(*args)
    for nf, nw, nb in itertools.product((True, False), repeat=3):
        if not (nf or nw or nb):
            with pytest.raises(_lib.VfiLibraryError):
                ops.phasenet_predict_backward(*args, need_feat=False, need_weight=False, need_bias=False)
            continue
        got = ops.phasenet_predict_backward(*args, need_feat=nf, need_weight=nw, need_bias=nb)
        for a, b, need in zip(got, full, (nf, nw, nb)):
            assert (a is None) if not need else torch.equal(a, b)
    big = torch.full((3, 70, 31, 33), 7.0, device=device)          # grad_f written into a channel slice, nothing beside it
    ops.phasenet_predict_backward(*args, need_weight=False, need_bias=False, out=big[:, 3:67])
    assert torch.equal(big[:, 3:67], full[0]) and bool((big[:, :3] == 7.0).all()) and bool((big[:, 67:] == 7.0).all())


def test_head_node_forward_is_the_inference_launch_and_its_backward(device):
    sd = R.block_state(4, 88, 8, 3)
    blk = PhaseNetBlock(88, 64, 8, (3, 3)).to(device)
    blk.load_state_dict(sd)
    for h, w in ((9, 13), (40, 104)):               # conv + emit inside the library, and the streaming kernel
        g = torch.Generator().manual_seed(h)
        f, amp = torch.randn((3, 64, h, w), generator=g), torch.rand((3, 8, h, w), generator=g)
        mx = torch.rand(3, generator=g) + 0.5
        gp, ga, gc = (torch.randn(s, generator=g) for s in ((12, 1, h, w), (12, 1, h, w), (3, 8, h, w)))
        pc = ops.PackedConv(blk.prediction_map[0].weight, blk.prediction_map[0].bias)
        want = ops.phasenet_predict(f.to(device), pc, amp.to(device), mx.to(device))
        fd = f.to(device).requires_grad_(True)
        got = G.level_head(blk, fd, amp.to(device), mx.to(device))
        assert all(o.grad_fn is not None for o in got)
        assert all(torch.equal(a.detach(), b) for a, b in zip(got, want))
        with torch.no_grad():
            plain = G.level_head(blk, fd, amp.to(device), mx.to(device))
        assert all(o.grad_fn is None and torch.equal(o, b) for o, b in zip(plain, want))
        ((got[0] * gc.to(device)).sum() + (got[1] * gp.to(device)).sum() + (got[2] * ga.to(device)).sum()).backward()
        wp, bp = sd["prediction_map.0.weight"].double().view(8, 64), sd["prediction_map.0.bias"].double()
        pred64 = W.head_forward(f.double(), wp, bp, amp.double(), mx.double())[0]
        wf, ww, wb = W.head_backward(f.double(), pred64, amp.double(), mx.double(), wp, gp.double().view(3, 4, h, w),
                                     ga.double().view(3, 4, h, w), gc.double())
        assert _rel(fd.grad, wf) <= 2e-4 and _rel(blk.prediction_map[0].weight.grad.view(8, 64), ww) <= 2e-4
        assert _rel(blk.prediction_map[0].bias.grad, wb) <= 2e-4
        assert all(p.grad is None for k, p in blk.named_parameters() if k.startswith("feature_map"))
        blk.zero_grad(set_to_none=True)


# ---- the whole walk ------------------------------------------------------------------------------------------------------
WALKS = {"65x77": (65, 77, 3, 9, None, "seeded"), "128x160": (128, 160, 3, 10, None, "trained"), "128x160-m4": (128, 160, 1, 10, 4, "seeded")}


def _state(kind, seed):
    sd = W.net_state(seed)
    return trained_stats.state_dict_like_trained("phasenet", sd, seed) if kind == "trained" else sd


def _core(sd, height, device):
    core = PhaseNetCore(height, device).fine_tune()
    core.load_state_dict(sd)
    return core


def _normalised(core, h, w, n, height, device):
    """Normalised values of a real analysis, the fused route of architecture.PhaseNet.forward: (values, walk inputs on the host)."""
    from vfi_amd.train.pyramid import Pyramid
    a0, _, a2 = (torch.from_numpy(x) for x in synth.translating_pair(3, h, w))
    imgs = torch.cat((a0[:n], a2[:n]), 0).to(device)
    pyr = Pyramid(height=height, nbands=4, scale_factor=W.S2, device=device)
    vals, bufs = pyr.filter(imgs, concat_frames=2, phase_scale=1.0 / math.pi)
    nv = core.normalize_vals(vals, concat=bufs)
    c = lambda t: t.detach().cpu().clone()
    inp = {"low": c(nv.low_level), "max_low": c(core.max_low_level), "phase": [c(p) for p in nv.phase],
           "amp": [c(a) for a in nv.amplitude], "max_amp": [c(x) for x in core.max_amplitudes]}
    return nv, inp


@functools.lru_cache(maxsize=None)
def _walk_reference(name, dev):
    """float64 and float32 torch-CPU autograd of the restated walk, computed once per configuration and left unchanged."""
    h, w, n, height, m, kind = WALKS[name]
    sd = _state(kind, 31)
    _, inp = _normalised(_core(sd, height, dev), h, w, n, height, dev)
    m_ = height - 2 if m is None else m
    out = {}
    for dtype in (torch.float64, torch.float32):
        P = W.net_params(sd, dtype)
        low, phases, amps = W.walk(P, W.to_dtype(inp, dtype), m_)
        if dtype == torch.float64:
            tgt = W.walk_targets(17, low, phases, amps)
            out["outputs"] = (low.detach(), [p.detach() for p in phases], [a.detach() for a in amps])
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


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_gradients_match_float64_autograd(name, device):
    h, w, n, height, m, kind = WALKS[name]
    sd, tgt, ref = _walk_reference(name, device)
    core = _core(sd, height, device)
    nv, _ = _normalised(core, h, w, n, height, device)
    vals, (low, phases, amps), loss = _hip_walk(core, nv, m, tgt, device)
    assert low.grad_fn is not None and all(p.grad_fn is not None for p in phases + amps)
    L = height - 2
    assert len(vals.phase) == L and all(not torch.is_tensor(p) for p in vals.phase[:L - len(phases)])
    assert vals.high_level.shape[1] == 1 and not bool(vals.high_level.any())
    # the grad route's outputs, within the bound of the float64 walk
    rl, rp, ra = ref["outputs"]
    for got, want in zip([low] + phases + amps, [rl] + rp + ra):
        assert _rel(got.detach(), want) <= 2e-4
    loss.backward()
    worst = (0.0, None)
    for k, p in core.named_parameters():
        want, lost = ref[torch.float64][k], ref[torch.float32][k]
        if want is None:
            assert p.grad is None, f"{k}: a block above level m must get None, not zeros"
            continue
        assert p.grad is not None, k
        err, lost32 = _rel(p.grad, want), _rel(lost, want)
        worst = max(worst, (err, k))
        assert err <= max(2e-4, 4 * lost32), (k, err, lost32)
    print(f"walk {name} ({kind}): worst per-tensor relative L2 {worst[0]:.3e} ({worst[1]})")
    if m is not None:
        assert all(p.grad is None for k, p in core.named_parameters() if int(k.split(".")[1]) > m)


def test_no_grad_route_is_unchanged_and_packs_build_once(device):
    name = "128x160"
    h, w, n, height, m, kind = WALKS[name]
    sd, tgt, ref = _walk_reference(name, device)
    core = _core(sd, height, device)
    nv, _ = _normalised(core, h, w, n, height, device)

    def record(fn):
        _lib.PROFILE = rec = _lib.Recorder()
        try:
            out = fn()
        finally:
            _lib.PROFILE = None
        return out, [row[0] for row in rec.rows]
    with torch.no_grad():
        core(nv, m)                                              # builds the inference packs, once
        base, calls = record(lambda: core(nv, m))
    for p in core.parameters():
        p.requires_grad_(False)
    frozen, calls_frozen = record(lambda: core(nv, m))           # grad mode on, nothing requires grad
    assert calls_frozen == calls and "vfi_phasenet_predict" in calls
    flat = lambda v: [v.low_level, v.high_level] + list(v.phase) + list(v.amplitude)
    assert all(a.grad_fn is None and torch.equal(a, b) for a, b in zip(flat(frozen), flat(base)))
    for p in core.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        off, calls_off = record(lambda: core(nv, m))
    assert calls_off == calls and all(torch.equal(a, b) for a, b in zip(flat(off), flat(base)))
    # a module that was not switched to fine-tuning keeps results without a graph, as callers in grad mode always got them
    assert not PhaseNetCore(height, device).fine_tuning
    plain, calls_plain = record(lambda: core.fine_tune(False)(nv, m))
    assert calls_plain == calls and all(a.grad_fn is None and torch.equal(a, b) for a, b in zip(flat(plain), flat(base)))
    core.fine_tune()
    # the grad route: same values within the bound, the same head launch per level, packs built once per step
    (vals, calls_grad) = record(lambda: core(nv, m))
    assert calls_grad.count("vfi_phasenet_predict") == calls.count("vfi_phasenet_predict") == height - 2
    assert calls_grad.count("vfi_conv2d_pack") == 3 * 8         # eight blocks, although the last one serves two levels
    for a, b in zip(flat(vals), flat(base)):
        assert _rel(a.detach(), b) <= 2e-4
    _, calls_again = record(lambda: core(nv, m))
    assert calls_again.count("vfi_conv2d_pack") == 0


def test_architecture_forward_is_one_training_step(device):
    h, w, height, m = 128, 160, 10, 6
    a0, a1, a2 = (torch.from_numpy(x) for x in synth.translating_pair(5, h, w))
    img_batch = torch.cat((a0, a2, a1), 0).to(device)            # two inputs, target frame last
    net = ArchPhaseNet(height, device)
    sd = W.net_state(41)
    net.core.load_state_dict(sd)
    with pytest.raises(NotImplementedError):
        net.train(True)
    with pytest.raises(NotImplementedError):
        net.core.train(True)
    assert net(img_batch, m=m)[0].grad_fn is None                # not asked to fine-tune: no graph, as before
    assert net.fine_tune() is net and net.core.fine_tuning
    with torch.no_grad():
        assert net(img_batch, m=m)[0].grad_fn is None
    prediction, vals_pred, vals_target = net(img_batch, m=m)
    assert prediction.requires_grad and prediction.grad_fn is not None
    target = img_batch[-3:]
    total = get_loss(vals_pred, vals_target, prediction, target, net.pyr)[0]
    total.backward()

    # float64 restatement of architecture.py:38-71 fed the product's analysis outputs
    with torch.no_grad():
        vals_list = separate_vals(net.pyr.filter(img_batch), 3)
        cat = get_concat_layers_inf(net.pyr, vals_list[:2])
    d = lambda t: t.detach().cpu().double()
    tgt_v = vals_list[-1]
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    L = height - 2

    def restated(dtype):
        P = W.net_params(sd, dtype)
        c = lambda t: d(t).to(dtype)
        inp = W.normalize({"low": c(cat.low_level), "phase": [c(p) for p in cat.phase], "amp": [c(a) for a in cat.amplitude]})
        low, phases, amps = W.walk(P, inp, m)
        ph, am = [0] * (L - m) + phases[::-1], [0] * (L - m) + amps[::-1]        # finest first
        for k in range(0, height - m):                                          # exchange_vals(.., 0, calc_pyr_height - m)
            ph[k], am[k] = c(tgt_v.phase[k]), c(tgt_v.amplitude[k])
        high = torch.zeros((3, 1, h, w), dtype=torch.float64)
        out = PR.reconstruct64(spec, PR.polar_to_coeff(high, [p.double() for p in ph], [a.double() for a in am], low.double()))
        loss = R.get_loss(ph, [c(p) for p in tgt_v.phase], out.to(dtype), c(target), 4)[0]
        loss.backward()
        return loss.detach(), W.named_grads(P)
    l64, g64 = restated(torch.float64)
    _, g32 = restated(torch.float32)
    print(f"architecture step loss {float(total.detach()):.7f} (float64 {float(l64):.7f})")
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
    assert used >= 8 * 3
    print(f"architecture step: {used} tensors, worst relative L2 {worst[0]:.3e} ({worst[1]})")


def test_fine_tuning_run_tracks_float64(device):
    h, w, n, height = 65, 77, 1, 9
    sd = W.net_state(51)
    core = _core(sd, height, device)
    nv, inp = _normalised(core, h, w, n, height, device)
    L = height - 2
    P = W.net_params(sd)
    d64 = W.to_dtype(inp)
    low, phases, amps = W.walk(P, d64, L)
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
    key0 = G.block_packs(core.layers[7])["key"]
    gpu = run(list(core.parameters()), lambda: _hip_walk(core, nv, None, tgt, device)[2])
    assert G.block_packs(core.layers[7])["key"] != key0           # the pack caches follow opt.step()
    cpu = run([P[i][k] for i in range(8) for k in R.BLOCK_KEYS], lambda: W.walk_loss(*W.walk(P, d64, L), t64))
    print("Adam run, HIP :", " ".join(f"{v:.5f}" for v in gpu))
    print("Adam run, CPU :", " ".join(f"{v:.5f}" for v in cpu))
    assert gpu[-1] < gpu[0], gpu
    for a, b in zip(gpu, cpu):
        assert abs(a - b) <= 0.02 * abs(b), (gpu, cpu)
