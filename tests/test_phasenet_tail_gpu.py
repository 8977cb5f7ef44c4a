"""vfi_phasenet_level_tail (a two-image band level's head and the next level's resize in one pass over the 64 feature planes)
against the two launches it replaces, vfi_phasenet_predict followed by vfi_resize_bilinear of [feature | prediction].

The level's outputs must be the old path's bits: the FMA chain over the channels and the emit arithmetic are the same source.
The resized planes are held to the same bits too; were the compiler to contract the bilinear expression differently in the new
kernel, the rule is: against a float64 evaluation of the same formula, the new path's worst absolute error may exceed the old
path's by at most one float32 ulp of the largest input magnitude.

Measured: the outputs are bit-identical at all six shapes; so are the resized planes of the four small shapes (the entry point
runs the old launches there).  At 96x170 -> 135x240 and 270x480 -> 382x679 the one-pass kernel's resized planes differ in last
bits and the float64 rule holds with equal errors: 6.084e-05 and 1.383e-04 for both paths (ulp 4.8e-07).  In the walk, phase
and amplitude of the finest level differ: 5.06e-07 against 5.29e-07 and 3.885e-07 against 3.885e-07 (ulp 1.9e-06)."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _resize_f64(src, ho, wo):
    """torch's bilinear resize, align_corners=False, of (..., h, w) float32 planes, evaluated in float64."""
    src = src.astype(np.float64)
    h, w = src.shape[-2:]

    def taps(n_in, n_out):
        f = np.maximum(n_in / n_out * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(f.astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), f - i0

    y0, y1, ly = taps(h, ho)
    x0, x1, lx = taps(w, wo)
    ly = ly[:, None]
    top = (1.0 - lx) * src[..., y0, :][..., x0] + lx * src[..., y0, :][..., x1]
    bot = (1.0 - lx) * src[..., y1, :][..., x0] + lx * src[..., y1, :][..., x1]
    return (1.0 - ly) * top + ly * bot


def _same_or_within_one_ulp(new, old, src, ho, wo, what):
    """Bit identity; else the float64 rule of the module docstring.  -> True when the bits were identical."""
    if torch.equal(new, old):
        return True
    src = src.cpu().numpy()
    ref = _resize_f64(src, ho, wo)
    e_new = float(np.abs(new.cpu().numpy() - ref).max())
    e_old = float(np.abs(old.cpu().numpy() - ref).max())
    ulp = float(np.spacing(np.float32(np.abs(src).max())))
    print(f"{what}: not bit-identical; max error against float64: new {e_new:.3e}, old {e_old:.3e}, ulp {ulp:.3e}")
    assert e_new <= e_old + ulp, (what, e_new, e_old, ulp)
    return False


@pytest.mark.parametrize("n,h,w,ho,wo", [(3, 6, 11, 9, 15),           # smaller than a tile; every clamp
                                         (3, 17, 30, 24, 43),         # width = 3 mod 4
                                         (3, 34, 60, 48, 85),         # width = 1 mod 4
                                         (3, 48, 85, 68, 120),        # odd source width
                                         (2, 96, 170, 135, 240),      # several tiles both ways; last tile row partial
                                         (1, 270, 480, 382, 679)])    # odd width above one tile
def test_level_tail_equals_predict_then_resize(n, h, w, ho, wo, device):
    from vfi_amd import _lib, ops
    g = torch.Generator().manual_seed(h * w + n)
    fp = torch.randn((n, 80, h, w), generator=g).to(device)            # features = fp[:, :64]: a batch stride of 80 planes
    x = torch.rand((n, 88, h, w), generator=g).to(device)
    mx = (torch.rand((n,), generator=g) + 0.5).to(device)
    pc = ops.PackedConv(torch.randn((8, 64, 1, 1), generator=g) / 8.0, torch.randn((8,), generator=g) * 0.1, device=device)
    amp_in = x[:, 80:]
    feat0 = fp[:, :64].clone()

    # the two launches: the prediction planes go to fp[:, 64:72], the 72 planes are resized into x_next[:, :72]
    p_ref, a_ref = torch.empty((n * 4, 1, h, w), device=device), torch.empty((n * 4, 1, h, w), device=device)
    _lib.call("vfi_phasenet_predict", fp.data_ptr(), fp.stride(0), pc.packed.data_ptr(), pc.bias.data_ptr(), amp_in.data_ptr(), x.stride(0),
              mx.data_ptr(), fp[:, 64:].data_ptr(), fp.stride(0), p_ref.data_ptr(), a_ref.data_ptr(), n, 64, h, w, _lib.stream_ptr())
    ref_next = torch.full((n, 88, ho, wo), SENTINEL, device=device)
    ops.resize_bilinear(fp[:, :72], (ho, wo), align_corners=False, out=ref_next[:, :72])

    x_next = torch.full((n, 88, ho, wo), SENTINEL, device=device)
    p_out, a_out = ops.phasenet_level_tail(fp, pc, amp_in, mx, x_next[:, :72])
    torch.cuda.synchronize()

    assert torch.equal(fp[:, :64], feat0)                                # the features are only read
    assert bool((x_next[:, 72:] == SENTINEL).all())                      # channels 72..87 are not touched
    assert torch.equal(p_out, p_ref) and torch.equal(a_out, a_ref)
    _same_or_within_one_ulp(x_next[:, :72], ref_next[:, :72], fp[:, :72], ho, wo, f"resized prefix {h}x{w} -> {ho}x{wo}")


def test_fused_walk_equals_the_two_launch_walk(device, monkeypatch):
    """PhaseNet.forward on the levels of a 96x128 pair: the walk with the one-launch tails against VFI_PHASENET_TAIL=0, every
    output by the rule of the module docstring (the float64 evaluation: the oracle's walk on float64 tensors).  The levels of
    this size lie below ops.PHASENET_TAIL_MIN_PIXELS, so the default walk is the old one; VFI_PHASENET_TAIL=1 takes the
    tail at every level that can."""
    from oracle import layout_cpu, nets_cpu, synth
    from vfi_amd import ops
    from vfi_amd.phase_net.phase_net import PhaseNet
    from vfi_amd.values import DecompValues
    h, w = 96, 128
    assert h * w < ops.PHASENET_TAIL_MIN_PIXELS
    height = layout_cpu.calc_pyr_height(h, w)
    sd = nets_cpu.phasenet_random_state_dict(3)
    net = PhaseNet(types.SimpleNamespace(height=height, nbands=4), device)
    net.load_state_dict(sd)
    net.eval()
    vin = layout_cpu.get_concat_layers_inf(layout_cpu.separate_vals(synth.synthetic_vals(11, 6, h, w, height), 2))
    dv = DecompValues(vin.high_level.to(device), [p.to(device) for p in vin.phase], [a.to(device) for a in vin.amplitude],
                      vin.low_level.to(device))
    normed = net.normalize_vals(dv)
    calls = []
    tail = ops.phasenet_level_tail
    monkeypatch.setattr(ops, "phasenet_level_tail", lambda *a: (calls.append(a[0].shape), tail(*a))[1])
    monkeypatch.delenv("VFI_PHASENET_TAIL", raising=False)
    default = net(normed)
    assert not calls
    monkeypatch.setenv("VFI_PHASENET_TAIL", "1")
    new = net(normed)
    assert len(calls) >= 3 and calls[-1][2:] == (68, 91)        # ... the last one in the one-pass kernel (>= 4096 pixels, even)
    monkeypatch.setenv("VFI_PHASENET_TAIL", "0")
    old = net(normed)
    torch.cuda.synchronize()
    assert len(calls) == len(new.phase) - 2               # none with the switch at 0

    to64 = lambda v: DecompValues(v.high_level.double(), [p.double() for p in v.phase], [a.double() for a in v.amplitude], v.low_level.double())
    normed64, state64 = nets_cpu.phasenet_normalize(to64(vin))
    with torch.no_grad():
        ref = nets_cpu.phasenet_forward({k: v.double() for k, v in sd.items()}, normed64, state64, height)
    big = max(float(t.abs().max()) for t in vin.phase + vin.amplitude + [vin.low_level])
    ulp = float(np.spacing(np.float32(big)))
    names = ["low"] + [f"phase{k}" for k in range(len(new.phase))] + [f"amp{k}" for k in range(len(new.amplitude))]
    for name, a, b, d, r in zip(names, [new.low_level] + new.phase + new.amplitude, [old.low_level] + old.phase + old.amplitude,
                                [default.low_level] + default.phase + default.amplitude, [ref.low_level] + ref.phase + ref.amplitude):
        assert torch.equal(d, b), name                          # the default walk at this size IS the two-launch walk
        if torch.equal(a, b):
            continue
        e_new, e_old = float((a.cpu().double() - r).abs().max()), float((b.cpu().double() - r).abs().max())
        print(f"{name}: not bit-identical; max error against float64: new {e_new:.3e}, old {e_old:.3e}, ulp {ulp:.3e}")
        assert e_new <= e_old + ulp, (name, e_new, e_old, ulp)
