"""FusionNet's training batch (vfi_amd/fusion_net/train_batch.py; reference src/fusion_net/trainer.py:65-259).

B = 3 at 64x96 is the smallest batch at which both analyses of `fusion_net_inputs` (6B = 18 images) pass a slice of the
pyramid plan (16 images).  Per sample, every input it produces is held against `FusionInterpolator`
on that pair alone at the project's bar, >= 60 dB on [0, 1] images.  `ada_uncertainty` amplifies
differences of its input images by 50-57 dB (tests/test_oracle_conditioning.py), so it is held the way
tests/test_pipeline_gpu.py holds it: the oracle's uncertainty_maps applied to the batch function's OWN ada_pred[b],
phase_pred[b] must reproduce its map at >= 60 dB.  Then one training step of the reference (trainer.py:246-259)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from oracle import layout_cpu, pipeline_cpu, pyramid_cpu, synth, uncertainty_cpu
from vfi_amd.adacof.models import Model
from vfi_amd.fusion_net.fusion_net import FusionNet
from vfi_amd.fusion_net.interpolate_twoframe import FusionInterpolator
from vfi_amd.fusion_net.train_batch import fusion_net_inputs
from vfi_amd.phase_net.phase_net import PhaseNet
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.train.utils import calc_pyr_height, preprocess

pytestmark = pytest.mark.gpu
B, H, W_ = 3, 64, 96


def _psnr(a, b):
    return 10 * math.log10(1.0 / max(float(((a.double().cpu() - b.double().cpu()) ** 2).mean()), 1e-30))


def _models(device, fusion_training=False):
    weights = pipeline_cpu.seeded_weights(0)
    adacof = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    adacof.load(weights["adacof"])
    adacof.eval()
    fusion = FusionNet().to(device)
    fusion.load_state_dict(weights["fusionnet"])
    fusion.train(fusion_training)
    height = calc_pyr_height(torch.empty(3, H, W_, device="meta"))
    pyr = Pyramid(height=height, nbands=4, scale_factor=np.sqrt(2), device=device)
    phase_net = PhaseNet(pyr, device, num_img=2)
    phase_net.load_state_dict(weights["phasenet"])
    return weights, adacof, fusion, pyr, phase_net


def _frames(device):
    """(B, 3, H, W) rgb frames 1, 2 and the target: a different texture and motion per sample"""
    trips = [synth.translating_pair(7 + 5 * i, H, W_, shift=(3.5 - i, -2.25 + 1.5 * i)) for i in range(B)]
    return [torch.stack([torch.from_numpy(t[j]) for t in trips], 0).to(device) for j in (0, 2, 1)]


@functools.lru_cache(maxsize=None)
def _batch(device):
    weights, adacof, fusion, pyr, phase_net = _models(device, fusion_training=True)
    rgb1, rgb2, target = _frames(device)
    lab1, lab2 = preprocess(rgb1, device), preprocess(rgb2, device)
    out = fusion_net_inputs(adacof, phase_net, pyr, lab1, lab2, rgb1, rgb2)
    return weights, adacof, fusion, phase_net, (rgb1, rgb2, target, lab1, lab2), out


def test_inputs_match_the_interpolator_per_sample(device):
    weights, adacof, _, _, (rgb1, rgb2, _, lab1, lab2), (base, ada_pred, phase_pred, other, maps) = _batch(device)
    for t, c in ((base, 3), (ada_pred, 3), (phase_pred, 3), (other, 6), (maps, 3)):
        assert tuple(t.shape) == (B, c, H, W_) and t.dtype == torch.float32 and t.is_contiguous()
        assert not t.requires_grad and t.grad_fn is None and bool(torch.isfinite(t).all())
    assert torch.equal(other[:, :3], lab1.reshape(B, 3, H, W_)) and torch.equal(other[:, 3:], lab2.reshape(B, 3, H, W_))
    fusion = FusionNet().to(device)
    fusion.load_state_dict(weights["fusionnet"])
    fusion.eval()
    run = FusionInterpolator(adacof, fusion, weights["phasenet"], device)
    opyr = pyramid_cpu.Pyramid(layout_cpu.calc_pyr_height(H, W_), 4, np.sqrt(2))
    for b in range(B):
        one = run(rgb1[b], rgb2[b])
        report = {"phase_pred": _psnr(phase_pred[b], one["phase_pred"][0]), "ada_pred": _psnr(ada_pred[b], one["ada_pred"][0]),
                  "base": _psnr(base[b], one["base"][0]), "flow_var_map": _psnr(maps[b, 2], one["flow_var_map"][0, 0]),
                  "phase_uncertainty": _psnr(maps[b, 1], one["phase_uncertainty"][0])}
        pu, au = uncertainty_cpu.uncertainty_maps(opyr, ada_pred[b].cpu(), phase_pred[b].cpu())
        report["ada_uncertainty | own inputs"] = _psnr(maps[b, 0], au[0])
        report["phase_uncertainty | own inputs"] = _psnr(maps[b, 1], pu[0])
        print(f"sample {b}:", {k: round(v, 1) for k, v in report.items()},
              "ada_uncertainty vs the interpolator (not asserted):", round(_psnr(maps[b, 0], one["ada_uncertainty"][0]), 1))
        for k, v in report.items():
            assert v >= 60.0, (b, k, report)
        # the trainable forward on these inputs is the interpolator's frame
        with torch.no_grad():
            final = fusion(base[b:b + 1], ada_pred[b:b + 1], phase_pred[b:b + 1], other[b:b + 1], maps[b:b + 1], variant=0)
        assert _psnr(final, one["final"]) >= 60.0, b
    # the samples are different pairs: a slice mix-up would not pass the above by accident
    assert _psnr(phase_pred[0], phase_pred[1]) < 40.0 and _psnr(phase_pred[1], phase_pred[2]) < 40.0


def test_one_training_step(device):
    _, adacof, fusion, phase_net, (_, _, target, _, _), (base, ada_pred, phase_pred, other, maps) = _batch(device)
    for p in list(adacof.parameters()) + list(phase_net.parameters()) + list(fusion.parameters()):
        p.grad = None
    assert fusion.training and any(p.requires_grad for p in adacof.parameters()) and any(p.requires_grad for p in phase_net.parameters())
    final = fusion(base, ada_pred, phase_pred, other, maps, variant=0)
    assert final.grad_fn is not None and tuple(final.shape) == (B, 3, H, W_)
    loss = torch.nn.L1Loss()(target, torch.clip(final, 0, 1))                        # trainer.py:246-254
    loss.backward()
    assert math.isfinite(float(loss.detach()))
    live = [(k, p) for k, p in fusion.named_parameters() if not k.startswith("net.")]   # (`net.` is the variant this call does not run)
    assert live and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in live)
    assert any(float(p.grad.abs().max()) > 0 for _, p in live)
    assert all(p.grad is None for p in adacof.parameters()) and all(p.grad is None for p in phase_net.parameters())


def test_channel_order_of_other_and_maps_with_integer_coded_inputs(device):
    """other = Lab frame 1 | Lab frame 2 per sample; maps = [ada_uncertainty, phase_uncertainty, flow_var_map]
    (trainer.py:208-211): Lab planes that hold their own index, and a stand-in AdaCoF whose mask holds the sample's."""
    _, _, _, pyr, phase_net = _models(device)
    rgb1, rgb2, _ = _frames(device)
    # plane j of frame 1 holds j / 128, of frame 2 (64 + j) / 128: exact in float32, and inside the range of scaled Lab values
    code = lambda first: ((first + torch.arange(3 * B, device=device, dtype=torch.float32)) / 128).view(-1, 1, 1).expand(3 * B, H, W_).contiguous()
    lab1, lab2 = code(0.0), code(64.0)
    seen = []

    def adacof(f1, f2):
        assert not torch.is_grad_enabled()
        seen.append(f1.shape[0])
        n = f1.shape[0]
        mask = (1000.0 + torch.arange(n, device=device, dtype=torch.float32)).view(n, 1, 1, 1).expand(n, 1, H, W_).contiguous()
        return f1, f2, (0.5 * (f1 + f2)).contiguous(), mask
    base, ada_pred, phase_pred, other, maps = fusion_net_inputs(adacof, phase_net, pyr, lab1, lab2, rgb1, rgb2)
    assert seen == [3 * B, B]                                        # AdaCoF #1-#3 as one batch, then #4
    for b in range(B):
        for c in range(3):
            assert bool((other[b, c] * 128 == 3 * b + c).all()) and bool((other[b, 3 + c] * 128 == 64 + 3 * b + c).all()), (b, c)
        assert bool((maps[b, 2] == 1000 + b).all()), b              # the mask of AdaCoF #1, sample b
        assert float(maps[b, :2].min()) >= 0.0 and float(maps[b, :2].max()) <= 1.0       # the two clamped uncertainty maps
    assert torch.equal(ada_pred, 0.5 * (rgb1 + rgb2))
    # phase_uncertainty is a Gaussian blur (sigma 5) of a clamped map, ada_uncertainty a distance from a median: only the
    # former is smooth
    rough = lambda t: float((t[:, 1:] - t[:, :-1]).abs().max())
    assert rough(maps[:, 1]) <= 0.1
