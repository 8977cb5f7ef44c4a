"""CPU checks of training PhaseNet with three and four input images: the float64 restatement of the
walk under autograd (tests/phasenet_fusion_grad_ref.py), on the running statistics and on the batch's, against loss, gradients
and running statistics the reference's own `PhaseNet(num_img = 3 | 4).forward` produced (tests/golden/phasenet_fusion_grad.npz);
the closed forms of the three adjoints against float64 autograd of their forwards; the three new entry points' argument
validation; the `fine_tune(fusion=True)` switch; and the ordering of `fusion_img_batch`."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

import phasenet_bn_ref as B
import phasenet_fusion_grad_ref as FG
import phasenet_fusion_ref as FR
import phasenet_grad_ref as R
import phasenet_walk_ref as W


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "phasenet_fusion_grad.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("num_img", [3, 4])
def test_walk_restatement_matches_the_reference_fixture(num_img, mode, golden_dir):
    z = _fixture(golden_dir)
    n, h, w, height = (int(v) for v in z["shape"])
    seed, L = int(z["seed"]), height - 2
    assert n == 2 and L == 8                                    # statistics span the batch; the last block serves two levels
    pre = f"n{num_img}_"
    p = f"{pre}{mode}_"
    t = lambda k: torch.from_numpy(z[k])
    inp = FG.seeded_inputs(seed + num_img, n, h, w, height, num_img)      # the generator the fixture script used, restated
    assert torch.equal(inp["low"], t(pre + "low")) and all(torch.equal(a, t(f"{pre}amp{i}")) for i, a in enumerate(inp["amp"]))
    assert all(torch.equal(a, t(f"{pre}phase{i}")) for i, a in enumerate(inp["phase"]))
    assert inp["low"].shape[1] == num_img and inp["amp"][0].shape[1] == 4 * num_img
    tgt = {"low": t(p + "tgt_low"), "phase": [t(f"{p}tgt_phase{i}") for i in range(L)], "amp": [t(f"{p}tgt_amp{i}") for i in range(L)]}
    state = FR.net_state(seed, num_img)
    walk = FG.bn_walk if mode == "train" else FG.walk
    P = FG.net_params(state)
    d, t64 = W.to_dtype(inp), W.to_dtype(tgt)
    low, phases, amps = walk(P, d, L, num_img)
    for ph, pt in zip(phases, t64["phase"]):                    # the targets keep the cut and the kink out of reach
        dist = R.wrap(pt - ph.detach()).abs()
        assert 0.04 <= float(dist.min()) and float(dist.max()) <= np.pi - 0.04
    loss = W.walk_loss(low, phases, amps, t64)
    assert abs(float(loss.detach()) - float(z[p + "loss"])) <= 1e-10
    loss.backward()
    grads = W.named_grads(P)
    g = torch.Generator().manual_seed(seed + 2)
    checked = 0
    for k, got in grads.items():
        if got.dim() == 4 and "prediction_map" not in k:
            probe = torch.randn(got.shape, generator=g, dtype=torch.float64)
            assert abs(float(got.norm()) - float(z[p + "norm:" + k])) <= 1e-10 * max(1.0, float(z[p + "norm:" + k])), k
            assert abs(float((got * probe).sum()) - float(z[p + "dot:" + k])) <= 1e-10 * max(1.0, abs(float(z[p + "dot:" + k]))), k
        else:
            want = torch.from_numpy(z[p + "grad:" + k])
            assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())), k
        checked += 1
    assert checked == 8 * 8
    assert grads["layers.3.prediction_map.0.weight"].shape[0] == (12 if num_img == 3 else 8)
    for k, got in B.named_buffers(P).items():
        want = torch.from_numpy(z[p + "buffer:" + k])
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(want) == (0 if mode == "eval" else 2 if k.startswith("layers.7.") else 1), k
        else:
            assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())), k
            assert torch.allclose(got, state[k].double()) == (mode == "eval"), k
    # hierarchical form: m = 3 runs blocks 0-3 only
    P3 = FG.net_params(state)
    low3, ph3, am3 = walk(P3, d, 3, num_img)
    loss3 = W.walk_loss(low3, ph3, am3, {"low": t64["low"], "phase": t64["phase"][:3], "amp": t64["amp"][:3]})
    assert abs(float(loss3.detach()) - float(z[p + "loss_m3"])) <= 1e-10
    loss3.backward()
    assert all((P3[i]["feature_map.0.weight"].grad is None) == (i > 3) for i in range(8))
    if mode == "train":
        assert [int(P3[i]["feature_map.1.num_batches_tracked"]) for i in range(8)] == [1, 1, 1, 1, 0, 0, 0, 0]
        # the two modes differ: batch statistics were really in use
        assert abs(float(z[p + "loss"]) - float(W.walk_loss(*FG.walk(FG.net_params(state), d, L, num_img), t64).detach())) > 1e-3


# ---- the closed forms against autograd ------------------------------------------------------------------------------------------
def _case(num_img, seed=0, n=2, h=3, w=5):
    g = torch.Generator().manual_seed(seed + num_img)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)
    pl, pb = FR.pred_channels(num_img)
    case = dict(f=r(n, 64, h, w), w=r(pb, 64) / 8, b=r(pb) / 8, amp=u(n, 4 * num_img, h, w), mx=u(n) + 0.5,
                low=u(n, num_img, h, w) * 2 - 1, mxl=u(n) + 0.5, pred=torch.tanh(r(n, pb, h, w)), pred_low=torch.tanh(r(n, pl, h, w)),
                gp=r(n, 4, h, w), ga=r(n, 4, h, w), gc=r(n, pb, h, w), gl=r(n, 1, h, w))
    if num_img == 4:                # the planes that are never read
        case["amp"][:, 8:] = float("nan")
        case["low"][:, 2:] = float("nan")
    return case


@pytest.mark.parametrize("num_img", [2, 3, 4])
def test_emit_adjoints_closed_form_match_autograd(num_img):
    c = _case(num_img)
    for gp, ga in ((True, True), (True, False), (False, True)):
        pred = c["pred"].clone().requires_grad_(True)
        phase, amp = FR.emit_n(pred, c["amp"], c["mx"], num_img)
        ((phase * c["gp"]).sum() * gp + (amp * c["ga"]).sum() * ga).backward()
        got = FG.emit_n_backward(c["gp"] if gp else None, c["ga"] if ga else None, c["pred"], c["amp"], c["mx"], num_img)
        assert bool(torch.isfinite(got).all()) and float((got - pred.grad).abs().max()) <= 1e-12 * max(1.0, float(pred.grad.abs().max()))
    if num_img == 2:
        want = R.emit_backward(c["gp"].numpy(), c["ga"].numpy(), c["amp"].numpy(), c["mx"].numpy())
        assert float(np.abs(FG.emit_n_backward(c["gp"], c["ga"], c["pred"], c["amp"], c["mx"], 2).numpy() - want).max()) <= 1e-12
    pl = c["pred_low"].clone().requires_grad_(True)
    (FR.emit_low_n(pl, c["low"], c["mxl"], num_img) * c["gl"]).sum().backward()
    got = FG.emit_low_n_backward(c["gl"], c["pred_low"], c["low"], c["mxl"], num_img)
    assert got.shape == pl.grad.shape and bool(torch.isfinite(got).all())
    assert float((got - pl.grad).abs().max()) <= 1e-12 * max(1.0, float(pl.grad.abs().max()))


@pytest.mark.parametrize("num_img", [2, 3, 4])
def test_head_adjoint_closed_form_matches_autograd(num_img):
    c = _case(num_img, seed=5)
    for gp, ga, gc in itertools.product((True, False), repeat=3):
        f, w, b = (c[k].clone().requires_grad_(True) for k in ("f", "w", "b"))
        pred, phase, amp = FG.head_forward(f, w, b, c["amp"], c["mx"], num_img)
        total = (phase * c["gp"]).sum() * gp + (amp * c["ga"]).sum() * ga + (pred * c["gc"]).sum() * gc
        got = FG.head_backward(c["f"], pred.detach(), c["amp"], c["mx"], c["w"], num_img, c["gp"] if gp else None,
                               c["ga"] if ga else None, c["gc"] if gc else None)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        if not (gp or ga or gc):
            assert not any(bool(t.any()) for t in got)
            continue
        total.backward()
        for a, want in zip(got, (f.grad, w.grad, b.grad)):
            assert a.shape == want.shape and float((a - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (gp, ga, gc)
    if num_img == 2:
        pred = c["pred"]
        for a, want in zip(FG.head_backward(c["f"], pred, c["amp"], c["mx"], c["w"], 2, c["gp"], c["ga"], c["gc"]),
                           W.head_backward(c["f"], pred, c["amp"], c["mx"], c["w"], c["gp"], c["ga"], c["gc"])):
            assert float((a - want).abs().max()) <= 1e-12


# ---- the library's argument checks ----------------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_before_any_device_call():
    import vfi_amd
    from vfi_amd import _lib
    h = vfi_amd.lib()
    one = 16
    assert _lib.PHASENET_HEAD_N_WORKSPACE_FLOATS == 1024 * 780
    emit = h.vfi_phasenet_emit_n_backward
    assert emit(None, None, one, 12, one, 12, one, one, 12, 1, 1, 3, None) == -1              # no upstream gradient
    assert emit(one, one, one, 12, one, 12, one, None, 12, 1, 1, 3, None) == -1               # no output
    assert emit(one, one, one, 12, None, 12, one, one, 12, 1, 1, 3, None) == -1               # grad_amp without amplitudes
    assert emit(one, one, None, 12, one, 12, one, one, 12, 1, 1, 3, None) == -1               # ... or, for three images, pred
    assert emit(one, one, one, 12, one, 12, one, one, 12, 0, 1, 3, None) == -1
    assert emit(one, one, one, 12, one, 12, one, one, 12, 1, -1, 3, None) == -1
    for bad in (1, 5):
        assert emit(one, one, one, 12, one, 12, one, one, 12, 1, 1, bad, None) == -4 and f"num_img {bad}".encode() in h.vfi_last_error()
    low = h.vfi_phasenet_emit_low_n_backward
    assert low(None, one, 2, one, 3, one, one, 2, 1, 1, 3, None) == -1
    assert low(one, one, 2, None, 3, one, one, 2, 1, 1, 3, None) == -1
    assert low(one, one, 2, one, 3, None, one, 2, 1, 1, 3, None) == -1
    assert low(one, one, 2, one, 3, one, None, 2, 1, 1, 3, None) == -1
    assert low(one, None, 2, one, 3, one, one, 2, 1, 1, 3, None) == -1
    assert low(one, one, 2, one, 3, one, one, 2, 1, 0, 3, None) == -1
    for bad in (1, 5):
        assert low(one, one, 2, one, 3, one, one, 2, 1, 1, bad, None) == -4 and f"num_img {bad}".encode() in h.vfi_last_error()
    head = h.vfi_phasenet_predict_n_backward
    args = lambda **kw: [kw.get(k, d) for k, d in (("feat", one), ("fs", 64), ("pred", one), ("ps", 12), ("amp", one), ("as_", 12),
                                                  ("mx", one), ("w", one), ("gp", one), ("ga", one), ("gi", one), ("gis", 12),
                                                  ("gf", one), ("gfs", 64), ("gw", one), ("gb", one), ("ws", one), ("n", 1), ("hw", 1),
                                                  ("num_img", 3), ("stream", None))]
    assert head(*args(pred=None)) == -1
    assert head(*args(gf=None, gw=None, gb=None)) == -1 and b"null pointer" in h.vfi_last_error()         # no output asked for
    assert head(*args(w=None)) == -1
    assert head(*args(feat=None)) == -1 and head(*args(ws=None)) == -1
    assert head(*args(amp=None)) == -1 and head(*args(mx=None)) == -1
    assert head(*args(n=0)) == -1 and head(*args(hw=0)) == -1
    for bad in (1, 5):
        assert head(*args(num_img=bad)) == -4 and f"num_img {bad}".encode() in h.vfi_last_error()
    assert head(*args(hw=1 << 25)) == -4                                                                 # 64 HW beyond 32-bit pixel indices


# ---- the switch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [3, 4])
def test_fusion_switch_semantics_on_cpu_modules(num_img):
    from vfi_amd.phase_net.core import PhaseNetCore
    from vfi_amd.phase_net.phase_net import PhaseNet
    for net in (PhaseNetCore(4, "cpu", num_img=num_img), PhaseNet(types.SimpleNamespace(height=4, nbands=4), "cpu", num_img=num_img)):
        for kw in ({}, {"batch_stats": True}):
            with pytest.raises(NotImplementedError, match="training of the fusion variants"):
                net.fine_tune(**kw)
            assert not net.fine_tuning and not net.batch_stats
        assert net.fine_tune(fusion=True) is net and net.fine_tuning and not net.batch_stats
        assert not any(b.batch_stats for b in net.layers)
        assert net.fine_tune(fusion=True, batch_stats=True) is net and net.fine_tuning and net.batch_stats
        assert all(b.batch_stats for b in net.layers)
        assert not net.training and not any(mod.training for mod in net.modules())
        with pytest.raises(NotImplementedError):
            net.train(True)
        net.fine_tune(False)
        assert not net.fine_tuning and not net.batch_stats and not any(b.batch_stats for b in net.layers)
        net.fine_tune(False, batch_stats=True, fusion=True)         # nothing to train: the flags stay off
        assert not net.fine_tuning and not net.batch_stats and not any(b.batch_stats for b in net.layers)


def test_fusion_keyword_changes_nothing_for_two_images():
    from vfi_amd.phase_net.core import PhaseNetCore
    net = PhaseNetCore(4, "cpu")
    assert net.fine_tune(fusion=True).fine_tuning and not net.batch_stats
    assert net.fine_tune(batch_stats=True, fusion=True).batch_stats and net.fine_tune(False).fine_tuning is False
    assert "fusion" in PhaseNetCore.fine_tune.__doc__


def test_architecture_passes_the_switch_down():
    from vfi_amd.phase_net import architecture
    calls = []
    net = architecture.PhaseNet.__new__(architecture.PhaseNet)
    torch.nn.Module.__init__(net)
    net.core = types.SimpleNamespace(fine_tune=lambda mode=True, **kw: calls.append((mode, kw)))
    assert net.fine_tune(fusion=True, batch_stats=True) is net and net.fine_tune(False) is net
    assert calls == [(True, {"batch_stats": True, "fusion": True}), (False, {"batch_stats": False, "fusion": False})]


# ---- the reference's batch assembly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [3, 4])
def test_fusion_img_batch_order_and_shapes(num_img, monkeypatch):
    from vfi_amd import ops
    from vfi_amd.train.fusion import fusion_img_batch
    b, h, w = 2, 4, 6
    monkeypatch.setattr(ops, "rgb2lab", lambda x: x + 1000.0)              # a stand-in that leaves a mark and keeps the layout
    code = lambda base: base + torch.arange(b * 3 * h * w, dtype=torch.float32).reshape(b, 3, h, w)
    rgb1, rgb2 = code(1e4).requires_grad_(True), code(2e4)
    lab = lambda base: code(base).reshape(-1, h, w)
    lab1, lab2, target = lab(1e5), lab(2e5), lab(3e5)
    seen = []

    def adacof(f1, f2):
        seen.append((f1, f2, torch.is_grad_enabled()))
        return f1 * 2, f2 * 2, f1 + f2, "mask"
    out = fusion_img_batch(adacof, lab1, lab2, rgb1, rgb2, target, num_img)
    assert seen[0][0] is rgb1 and seen[0][1] is rgb2 and seen[0][2] is False          # AdaCoF ran under no_grad
    assert out.shape == ((num_img + 1) * b * 3, h, w) and not out.requires_grad
    parts = out.reshape(num_img + 1, b * 3, h, w)
    ch = lambda x: (x.detach() + 1000.0).reshape(-1, h, w)
    want = [lab1, lab2] + ([ch(rgb1 * 2), ch(rgb2 * 2)] if num_img == 4 else [ch(rgb1 + rgb2)]) + [target]
    assert len(want) == (5 if num_img == 4 else 4)
    assert all(torch.equal(a, x) for a, x in zip(parts, want))
    with pytest.raises(ValueError):
        fusion_img_batch(adacof, lab1, lab2, rgb1, rgb2, target, 2)
