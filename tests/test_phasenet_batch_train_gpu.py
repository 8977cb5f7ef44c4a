"""architecture.PhaseNet on a batch of B samples as one training step: img_batch holds
(num_img + 1) * 3 * B channel-images, frame-major as reference src/train/trainer.py's `Trainer.predict` builds it, and goes
through ONE `Pyramid.filter` call -- 18 to 72 images, past the 16 a pyramid plan holds.

The step is tests/test_phasenet_walk_backward_gpu.py::test_architecture_forward_is_one_training_step's: forward, get_loss,
backward, against float64 autograd of the restatement of architecture.py:38-71 (phasenet_walk_ref / phasenet_fusion_ref,
pyramid_grad_ref, phasenet_grad_ref) fed the product's analysis outputs.  Its rule, unchanged: the loss agrees to 1e-4
relative; parameter gradients to relative L2 2e-4 per tensor, or 4 x what float32 torch-CPU autograd of the same restatement
loses against the float64 one.  On batch statistics the running statistics are held to tests/test_phasenet_bn_gpu.py's 2e-4.

Every sample of a batch is a different synthetic pair, so images that land in the wrong slice change the loss."""
import pytest
import torch

import phasenet_bn_ref as B
import phasenet_fusion_grad_ref as FG
import phasenet_fusion_ref as FR
import phasenet_grad_ref as R
import phasenet_walk_ref as W
import pyramid_grad_ref as PR
from oracle import pyramid_cpu, synth
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
from vfi_amd.train.fusion import fusion_img_batch
from vfi_amd.train.loss import get_loss
from vfi_amd.train.utils import calc_pyr_height, get_concat_layers_inf, preprocess, separate_vals

pytestmark = pytest.mark.gpu
ZERO_GRADIENT = "feature_map.0.bias"            # on batch statistics only (its gradient is exactly zero)

# name: (num_img, B, h, w, m, batch statistics)
STEPS = {
    "two-images-B2-64x80": (2, 2, 64, 80, 5, False),              # 18 images
    "two-images-B8-32x48": (2, 8, 32, 48, 3, False),              # 72 images: the reference's default batch, m below full height
    "four-images-B2-48x64": (4, 2, 48, 64, 4, False),             # 30 images, fine_tune(fusion=True)
    "two-images-B3-32x48-batch-statistics": (2, 3, 32, 48, 3, True),      # 27 images
}


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _stand_in_adacof(seed):
    """A seeded stand-in for AdaCoF: (frame 1 warped, frame 2 warped, their blend, a mask) from rolls and a fixed blend."""
    g = torch.Generator().manual_seed(seed)
    a = float(torch.rand(1, generator=g)) * 0.4 + 0.3

    def model(f1, f2):
        assert not torch.is_grad_enabled()
        w1, w2 = torch.roll(f1, (1, -2), (2, 3)) * 0.9 + 0.05, torch.roll(f2, (-1, 1), (2, 3)) * 0.9 + 0.05
        return w1, w2, (a * w1 + (1 - a) * w2).clamp(0, 1), None
    return model


def _samples(b, h, w, device):
    """rgb frames 1, 2 and the target, each (B, 3, H, W): a different texture and motion per sample"""
    trips = [synth.translating_pair(11 + 7 * i, h, w, shift=(1.5 + i, -2.25 + 0.5 * i)) for i in range(b)]
    return [torch.stack([torch.from_numpy(t[j]) for t in trips], 0).to(device) for j in (0, 2, 1)]


@pytest.mark.parametrize("name", list(STEPS))
def test_architecture_forward_on_a_batch_is_one_training_step(name, device):
    num_img, b, h, w, m, bn = STEPS[name]
    height = calc_pyr_height(torch.empty(3, h, w, device="meta"))
    L = height - 2
    assert m < L
    rgb1, rgb2, rgb_t = _samples(b, h, w, device)
    lab1, lab2, target = (preprocess(x, device) for x in (rgb1, rgb2, rgb_t))
    assert target.shape == (3 * b, h, w)
    if num_img == 2:
        img_batch = torch.cat((lab1, lab2, target), 0)                            # trainer.py:72
    else:
        img_batch = fusion_img_batch(_stand_in_adacof(3), lab1, lab2, rgb1, rgb2, target, num_img)
    n_all = (num_img + 1) * 3 * b
    assert img_batch.shape == (n_all, h, w) and n_all > 16
    assert torch.equal(img_batch[-3 * b:], target) and torch.equal(img_batch[:3 * b], lab1) and torch.equal(img_batch[3 * b:6 * b], lab2)
    net = ArchPhaseNet(height, device, num_img=num_img)
    sd = FR.net_state(41, num_img)
    net.core.load_state_dict(sd)
    if not bn:                                       # (on batch statistics every forward moves the running ones)
        assert net(img_batch, m=m)[0].grad_fn is None                              # not asked to train: no graph
    assert net.fine_tune(fusion=num_img != 2, batch_stats=bn) is net and net.core.fine_tuning and net.core.batch_stats == bn
    prediction, vals_pred, vals_target = net(img_batch, m=m)
    assert prediction.shape == (3 * b, h, w) and prediction.grad_fn is not None
    assert vals_target.high_level.shape == (3 * b, 1, h, w) and vals_pred.low_level.shape[0] == 3 * b
    total = get_loss(vals_pred, vals_target, prediction, target, net.pyr)[0]
    total.backward()

    # float64 restatement of architecture.py:38-71 fed the product's analysis outputs
    with torch.no_grad():
        vals_list = separate_vals(net.pyr.filter(img_batch), num_img + 1)
        cat = get_concat_layers_inf(net.pyr, vals_list[:-1])
    tgt_v = vals_list[-1]
    assert cat.low_level.shape[:2] == (3 * b, num_img) and cat.phase[0].shape[:2] == (3 * b, 4 * num_img)
    for k in range(L):
        assert torch.equal(tgt_v.phase[k], vals_target.phase[k]) and torch.equal(tgt_v.amplitude[k], vals_target.amplitude[k]), k
    d = lambda t: t.detach().cpu().double()
    spec = pyramid_cpu.PyramidSpec(h, w, height)

    def restated(dtype):
        P = FG.net_params(sd, dtype)
        c = lambda t: d(t).to(dtype)
        inp = FR.normalize({"low": c(cat.low_level), "phase": [c(p) for p in cat.phase], "amp": [c(a) for a in cat.amplitude]})
        low, phases, amps = (FG.bn_walk if bn else FG.walk)(P, inp, m, num_img)
        ph, am = [0] * (L - m) + phases[::-1], [0] * (L - m) + amps[::-1]         # finest first
        for k in range(0, min(height - m, L)):                                    # exchange_vals(.., 0, calc_pyr_height - m)
            ph[k], am[k] = c(tgt_v.phase[k]), c(tgt_v.amplitude[k])
        high = torch.zeros((3 * b, 1, h, w), dtype=torch.float64)
        out = PR.reconstruct64(spec, PR.polar_to_coeff(high, [p.double() for p in ph], [a.double() for a in am], low.double()))
        loss = R.get_loss(ph, [c(p) for p in tgt_v.phase], out.to(dtype), c(target), 4)[0]
        loss.backward()
        return loss.detach(), W.named_grads(P), B.named_buffers(P)
    l64, g64, buf64 = restated(torch.float64)
    _, g32, _ = restated(torch.float32)
    print(f"batch step {name}: loss {float(total.detach()):.7f} (float64 {float(l64):.7f})")
    assert abs(float(total.detach()) - float(l64)) <= 1e-4 * abs(float(l64))
    used, worst = 0, (0.0, None)
    for k, p in net.core.named_parameters():
        if g64[k] is None:
            assert p.grad is None, k
            continue
        used += 1
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        err, lost32 = _rel(p.grad, g64[k]), _rel(g32[k], g64[k])
        if not (bn and k.endswith(ZERO_GRADIENT)):
            worst = max(worst, (err, k))
        print(f"  {k}: relative L2 {err:.3e} (float32 torch-CPU {lost32:.3e})")
        assert err <= max(2e-4, 4 * lost32), (k, err, lost32)
    # exchange_vals hands levels 0 .. height - m - 1 to the target, so the loss sees the walk's levels 0 .. m - 3 (coarsest
    # first) and the low level: blocks 0 .. m - 2, eight tensors each; the blocks above get None, as float64 autograd gives
    assert used == 8 * (m - 1)
    print(f"batch step {name}: {used} tensors, worst relative L2 {worst[0]:.3e} ({worst[1]})")
    buffers = dict(net.core.named_buffers())
    for k, want in buf64.items():
        i = int(k.split(".")[1])
        if k.endswith("num_batches_tracked"):
            assert int(buffers[k]) == int(want) == (1 if bn and i <= m else 0), k
        elif not bn or i > m:
            assert torch.equal(buffers[k].cpu(), sd[k]), k
        else:
            err = _rel(buffers[k], want)
            print(f"  {k}: relative L2 {err:.3e}")
            assert err <= 2e-4, (k, err)
