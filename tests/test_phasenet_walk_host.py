"""CPU checks of the whole PhaseNet's backward: the float64 restatement of the coarse-to-fine walk
(tests/phasenet_walk_ref.py) against loss and gradients the reference's own `PhaseNet.forward` produced
(tests/golden/phasenet_walk_grad.npz), and the head adjoint's formulas against float64 autograd."""
import itertools
import os

import numpy as np
import pytest
import torch

import phasenet_grad_ref as R
import phasenet_walk_ref as W


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "phasenet_walk_grad.npz"))
    return {k: z[k] for k in z.files}


def _fixture_inputs(z, L):
    t = lambda k: torch.from_numpy(z[k])
    inp = {"low": t("low"), "max_low": t("max_low"), "phase": [t(f"phase{i}") for i in range(L)],
           "amp": [t(f"amp{i}") for i in range(L)], "max_amp": [t(f"max_amp{i}") for i in range(L)]}
    tgt = {"low": t("tgt_low"), "phase": [t(f"tgt_phase{i}") for i in range(L)], "amp": [t(f"tgt_amp{i}") for i in range(L)]}
    return inp, tgt


def test_walk_restatement_matches_the_reference_fixture(golden_dir):
    z = _fixture(golden_dir)
    n, h, w, height = (int(v) for v in z["shape"])
    seed, L = int(z["seed"]), height - 2
    assert L == 8 and len(W.BLOCKS) == 8            # the last block serves levels 6 and 7
    inp, tgt = _fixture_inputs(z, L)
    again = W.seeded_inputs(seed, n, h, w, height)  # the generator the fixture script used, restated
    assert torch.equal(again["low"], inp["low"]) and all(torch.equal(a, b) for a, b in zip(again["amp"], inp["amp"]))
    assert inp["phase"][0].shape[2:] == (3, 3) and inp["phase"][-1].shape[2:] == (h, w)
    P = W.net_params(W.net_state(seed))
    d, t64 = W.to_dtype(inp), W.to_dtype(tgt)
    low, phases, amps = W.walk(P, d, L)
    # the targets keep the cut and the kink out of reach
    for p, pt in zip(phases, t64["phase"]):
        dist = R.wrap(pt - p.detach()).abs()
        assert 0.04 <= float(dist.min()) and float(dist.max()) <= np.pi - 0.04
    loss = W.walk_loss(low, phases, amps, t64)
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-10
    loss.backward()
    grads = W.named_grads(P)
    g = torch.Generator().manual_seed(seed + 2)
    checked = 0
    for k, got in grads.items():
        if got.dim() == 4 and "prediction_map" not in k:
            probe = torch.randn(got.shape, generator=g, dtype=torch.float64)
            assert abs(float(got.norm()) - float(z["norm:" + k])) <= 1e-10 * max(1.0, float(z["norm:" + k])), k
            assert abs(float((got * probe).sum()) - float(z["dot:" + k])) <= 1e-10 * max(1.0, abs(float(z["dot:" + k]))), k
        else:
            want = torch.from_numpy(z["grad:" + k])
            assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())), k
        checked += 1
    assert checked == 8 * 8
    assert float(grads["layers.7.feature_map.3.weight"].norm()) > 0      # the shared block collects two levels
    # hierarchical form: m = 3 runs blocks 0-3 only
    P3 = W.net_params(W.net_state(seed))
    low3, ph3, am3 = W.walk(P3, d, 3)
    loss3 = W.walk_loss(low3, ph3, am3, {"low": t64["low"], "phase": t64["phase"][:3], "amp": t64["amp"][:3]})
    assert abs(float(loss3.detach()) - float(z["loss_m3"])) <= 1e-10
    loss3.backward()
    assert all(P3[i][k].grad is None for i in range(4, 8) for k in R.BLOCK_KEYS)
    assert all(P3[i][k].grad is not None for i in range(0, 4) for k in R.BLOCK_KEYS)


@pytest.mark.parametrize("nulls", list(itertools.product((False, True), repeat=3)))
def test_head_adjoint_formulas_match_autograd(nulls):
    """vfi_phasenet_predict_backward's formulas, every NULL combination of (grad_phase, grad_amp, grad_pred_in)."""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    n, h, w = 3, 5, 7
    f, wp, bp = r(n, 64, h, w).requires_grad_(True), (r(8, 64) / 8).requires_grad_(True), r(8).requires_grad_(True)
    amp_in = torch.rand((n, 8, h, w), generator=g, dtype=torch.float64)
    max_amp = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
    gp, ga, gc = (None if nulls[0] else r(n, 4, h, w)), (None if nulls[1] else r(n, 4, h, w)), (None if nulls[2] else r(n, 8, h, w))
    pred, phase, amp = W.head_forward(f, wp, bp, amp_in, max_amp)
    total = (pred * 0).sum()
    if gp is not None:
        total = total + (phase * gp).sum()
    if ga is not None:
        total = total + (amp * ga).sum()
    if gc is not None:
        total = total + (pred * gc).sum()
    total.backward()
    got = W.head_backward(f.detach(), pred.detach(), amp_in, max_amp, wp.detach(), gp, ga, gc)
    for a, b in zip(got, (f.grad, wp.grad, bp.grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_parents_still_refuse_training_mode():
    from vfi_amd.nn_util import PackedModule
    from vfi_amd.phase_net.core import PhaseNetCore
    from vfi_amd.phase_net.phase_net import PhaseNet
    import types
    for net in (PhaseNetCore(4, "cpu"), PhaseNet(types.SimpleNamespace(height=4, nbands=4), "cpu"), PackedModule()):
        with pytest.raises(NotImplementedError):
            net.train(True)

