"""CPU checks of PhaseNet with three and four input images: the float64 restatement the GPU tests compare
against (tests/phasenet_fusion_ref.py) is itself held against the reference's own outputs (tests/golden/phasenet_fusion_walk.npz,
made by tests/golden/make_golden_phasenet_fusion.py) and, at two images, against the oracle; the module's parameters carry the
reference's names and shapes; separate_vals splits lists of three and four as the reference does.

(get_concat_layers_inf copies with a device kernel, so its check at three and four values is in test_phasenet_fusion_gpu.py.)
"""
import os

import numpy as np
import pytest
import torch

import phasenet_fusion_ref as FR
from conftest import GOLDEN
from oracle import layout_cpu, nets_cpu, synth

FIX = os.path.join(GOLDEN, "phasenet_fusion_walk.npz")


def fixture_inputs(g, num_img):
    """The fixture's raw inputs as FR.raw_inputs returns them (float32 tensors, coarsest first)."""
    t = f"n{num_img}_"
    n, h, w, height = (int(v) for v in g["shape"])
    L = height - 2
    f = lambda k: torch.from_numpy(g[t + k])
    return {"low": f("low"), "high_shape": (n, num_img, h, w), "phase": [f(f"phase{i}") for i in range(L)],
            "amp": [f(f"amp{i}") for i in range(L)]}, L


@pytest.mark.parametrize("num_img", [3, 4])
def test_restatement_matches_the_reference_outputs(num_img):
    g = np.load(FIX)
    t = f"n{num_img}_"
    inp, L = fixture_inputs(g, num_img)
    regenerated = FR.raw_inputs(int(g["seed"]) + num_img, *(int(v) for v in g["shape"]), num_img)
    assert all(torch.equal(a, b) for a, b in zip(inp["phase"] + inp["amp"] + [inp["low"]],
                                                regenerated["phase"] + regenerated["amp"] + [regenerated["low"]]))
    normed = FR.normalize(FR.to_dtype(inp))
    close = lambda a, k: float(np.abs(a.numpy() - g[t + k]).max()) <= 1e-10 * max(1.0, float(np.abs(g[t + k]).max()))
    assert close(normed["max_low"], "max_low") and close(normed["low"], "norm_low")
    assert close(normed["phase"][0], "norm_phase0") and close(normed["amp"][0], "norm_amp0")
    for i in range(L):
        assert close(normed["max_amp"][i], f"max_amp{i}")
    P = FR.params(FR.net_state(int(g["seed"]), num_img))
    with torch.no_grad():
        low, phases, amps = FR.walk(P, normed, L, num_img)
        low3, ph3, am3 = FR.walk(P, normed, 3, num_img)
    assert close(low, "out_low") and close(low3, "m3_low")
    for i in range(L):                       # the fixture's outputs are finest first
        assert close(phases[L - 1 - i], f"out_phase{i}") and close(amps[L - 1 - i], f"out_amp{i}"), i
    for i in range(L):
        if i < L - 3:
            assert f"{t}m3_phase{i}" not in g.files          # the reference's scalar zeros
        else:
            assert close(ph3[L - 1 - i], f"m3_phase{i}") and close(am3[L - 1 - i], f"m3_amp{i}"), i
    assert not g[t + "out_high"].any() and g[t + "out_high"].shape == (2, 1, 12, 16)


def test_restatement_at_two_images_matches_the_oracle():
    h, w, height = 32, 48, 6
    vin = layout_cpu.get_concat_layers_inf(layout_cpu.separate_vals(synth.synthetic_vals(5, 6, h, w, height), 2))
    sd = nets_cpu.phasenet_random_state_dict(3)
    normed_o, state = nets_cpu.phasenet_normalize(vin)
    with torch.no_grad():
        want = nets_cpu.phasenet_forward(sd, normed_o, state, height)
        inp = {"low": vin.low_level, "phase": list(vin.phase), "amp": list(vin.amplitude)}
        low, phases, amps = FR.walk(FR.params(sd, torch.float32), FR.normalize(inp), height - 2, 2)
    L = height - 2
    assert (low - want.low_level).abs().max().item() <= 1e-6 * max(1.0, want.low_level.abs().max().item())
    for i in range(L):
        for got, ref in ((phases[L - 1 - i], want.phase[i]), (amps[L - 1 - i], want.amplitude[i])):
            assert got.shape == ref.shape and (got - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("num_img", [3, 4])
def test_module_has_the_reference_keys_and_shapes(num_img):
    from types import SimpleNamespace
    from vfi_amd.phase_net.phase_net import PhaseNet
    g = np.load(FIX)
    net = PhaseNet(SimpleNamespace(height=10, nbands=4), "meta", num_img=num_img)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"n{num_img}_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g[f"n{num_img}_shapes"]]
    assert net.pred_channels == ((2, 12) if num_img == 3 else (1, 8))
    assert {k: tuple(v.shape) for k, v in FR.net_state(0, num_img).items()} == {k: tuple(v.shape) for k, v in sd.items()}
    with pytest.raises(NotImplementedError, match="training of the fusion variants"):
        net.fine_tune()


def test_other_image_counts_are_refused():
    from types import SimpleNamespace
    from vfi_amd.phase_net.phase_net import PhaseNet
    for num_img in (1, 5):
        with pytest.raises(NotImplementedError):
            PhaseNet(SimpleNamespace(height=6, nbands=4), "meta", num_img=num_img)


def layout_vals(g, prefix, device="cpu"):
    from vfi_amd.values import DecompValues
    n = len([k for k in g.files if k.startswith(prefix + "phase")])
    f = lambda k: torch.from_numpy(g[prefix + k]).to(device)
    return DecompValues(f("high"), [f(f"phase{i}") for i in range(n)], [f(f"amp{i}") for i in range(n)], f("low"))


def same_vals(got, want):
    pairs = [(got.high_level, want.high_level), (got.low_level, want.low_level)] + list(zip(got.phase, want.phase)) + \
        list(zip(got.amplitude, want.amplitude))
    assert len(got.phase) == len(want.phase)
    for a, b in pairs:
        assert a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("num", [3, 4])
def test_separate_vals_splits_three_and_four(num):
    from vfi_amd.train import utils
    g = np.load(FIX)
    sep = utils.separate_vals(layout_vals(g, f"layout{num}_vals_"), num)
    assert len(sep) == num
    for i, s in enumerate(sep):
        same_vals(s, layout_vals(g, f"layout{num}_sep{i}_"))


def test_n_entry_points_validate_without_a_gpu():
    """Null pointers and a bad num_img are refused before any device call (as tests/test_abi.py checks for the others)."""
    import ctypes
    from vfi_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(16)
    assert h.vfi_phasenet_emit_n(None, 8, one, 8, one, one, one, 1, 1, 3, None) == -1
    assert h.vfi_phasenet_emit_n(one, 8, one, 8, one, one, one, 1, 1, 5, None) == -4 and b"num_img 5" in h.vfi_last_error()
    assert h.vfi_phasenet_emit_low_n(one, 1, one, 2, one, None, 1, 1, 2, None) == -1
    assert h.vfi_phasenet_emit_low_n(one, 1, one, 2, one, one, 1, 0, 2, None) == -1
    assert h.vfi_phasenet_emit_low_n(one, 1, one, 2, one, one, 1, 1, 1, None) == -4
    assert h.vfi_phasenet_predict_n(one, 64, one, one, None, 8, one, one, 8, one, one, 1, 64, 1, 1, 3, None) == -1
    assert h.vfi_phasenet_predict_n(one, 64, one, one, one, 8, one, one, 8, one, one, 1, 64, 1, 1, 6, None) == -4
    assert h.vfi_phasenet_predict_n(one, 64, one, one, one, 8, one, one, 8, one, one, 1, 64, 0, 1, 3, None) == -1
