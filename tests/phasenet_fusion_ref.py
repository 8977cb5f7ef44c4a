"""Torch restatement (any dtype) of the reference's PhaseNet with two, three and four input images
(src/phase_net/phase_net.py:21-35, 42-78, 80-105, 107-177), shared by tests/test_phasenet_fusion_host.py (CPU),
tests/test_phasenet_fusion_gpu.py and tests/golden/make_golden_phasenet_fusion.py:

  * the blocks' shapes, seeded weights (and weights with the trained two-frame checkpoint's per-tensor statistics), seeded raw
    inputs in the concatenated layout;
  * normalize_vals, the coarse-to-fine walk with both blends, reverse_normalize;
  * the head's formulas (vfi_phasenet_emit_n, vfi_phasenet_emit_low_n) on their own.

oracle/nets_cpu.py states the two-image network only; test_phasenet_fusion_host.py holds this file against it at num_img = 2 and
against the reference's own outputs (tests/golden/phasenet_fusion_walk.npz) at 3 and 4.
"""
import json
import math
import os

import torch

import phasenet_grad_ref as R
import phasenet_walk_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pred_channels(num_img):
    return (2, 12) if num_img == 3 else (1, 8)                     # phase_net.py:25-34


def blocks(num_img):
    """(c_in, pred_out, kernel) of the eight blocks, phase_net.py:23-35."""
    pl, pb = pred_channels(num_img)
    return [(num_img, pl, 1), (64 + pl + 8 * num_img, pb, 1), (64 + pb + 8 * num_img, pb, 1)] + [(64 + pb + 8 * num_img, pb, 3)] * 5


def net_state(seed, num_img):
    """Seeded state dict of PhaseNet(num_img).layers, each block drawn by phasenet_grad_ref.block_state."""
    return {f"layers.{i}.{k}": v for i, (cin, pred, ks) in enumerate(blocks(num_img))
            for k, v in R.block_state(seed * 100 + 10 * num_img + i, cin, pred, ks).items()}


def trained_like_state(seed, num_img):
    """net_state's keys and shapes with every floating-point tensor redrawn to the mean / std / range that the same key has in
    the reference's trained two-frame phase_net.pt (tests/golden/trained_weight_stats.json; the fusion checkpoints are not in
    the reference's snapshot).  Shapes differ from that table's where num_img enters, the statistics carry over."""
    with open(os.path.join(GOLDEN, "trained_weight_stats.json")) as f:
        table = json.load(f)["phasenet"]
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in net_state(seed, num_img).items():
        st = table.get(k)
        if st is None or not v.dtype.is_floating_point:
            out[k] = v.clone()
            continue
        t = torch.randn(v.shape, generator=g, dtype=torch.float64) * st["std"] + st["mean"]
        out[k] = t.clamp_(st["min"], st["max"]).to(v.dtype)
    return out


def params(sd, dtype=torch.float64, device=None):
    """List of per-block dicts (phasenet_grad_ref.block's argument) of a state dict, floating tensors as `dtype`."""
    out = []
    for i in range(8):
        pre = f"layers.{i}."
        out.append({k[len(pre):]: (v.to(dtype=dtype, device=device) if v.dtype.is_floating_point else v)
                    for k, v in sd.items() if k.startswith(pre)})
    return out


def raw_inputs(seed, n, h, w, height, num_img):
    """Concatenated raw values as get_concat_layers_inf returns them, lists COARSEST first: phase in [-pi, pi], amplitudes
    in [0, 1 + level], low level in [0.1, 2]; n = batch (colours), float32."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    sizes = W.level_sizes(h, w, height - 2)
    bands = sizes[:-1][::-1]
    return {"low": u((n, num_img, *sizes[-1]), 0.1, 2.0), "high_shape": (n, num_img, h, w),
            "phase": [u((n, 4 * num_img, *s), -math.pi, math.pi) for s in bands],
            "amp": [u((n, 4 * num_img, *s), 0.0, 1.0 + k) for k, s in enumerate(bands)]}


normalize = W.normalize         # phase_net.py:42-78 (any number of images: the maxima run over a sample's whole block)
to_dtype = W.to_dtype


def emit_n(pred, amp_in, max_amp, num_img):
    """phase_net.py:155-168 + :83,89: pred (N,8|12,H,W), amp_in (N,4*num_img,H,W) -> phase, amp (N,4,H,W)."""
    beta = (pred[:, 4:8] + 1) / 2
    amp = beta * amp_in[:, 4:8] + (1 - beta) * amp_in[:, :4]
    if num_img == 3:
        fb = (pred[:, 8:12] + 1) / 2
        amp = fb * amp + (1 - fb) * amp_in[:, 8:12]
    return pred[:, :4] * math.pi, amp * max_amp.reshape(-1, 1, 1, 1)


def emit_low_n(pred, low_in, max_low, num_img):
    """phase_net.py:115-124 + :98 -> (N,1,H,W)."""
    alpha = (pred[:, 0] + 1) / 2
    low = alpha * low_in[:, 0] + (1 - alpha) * low_in[:, 1]
    if num_img == 3:
        fa = (pred[:, 1] + 1) / 2
        low = fa * low + (1 - fa) * low_in[:, 2]
    return (low * max_low.reshape(-1, 1, 1)).unsqueeze(1)


def walk(P, inp, m, num_img, resize=R.torch_resize):
    """phase_net.py:107-177 with reverse_normalize (:80-105) on normalised inputs (`normalize`'s result) -> (low (N,1,hL,wL),
    [phase_out], [amp_out]) of the m coarsest levels, COARSEST first, each (N*4,1,h,w)."""
    f, c = R.block(P[0], inp["low"])
    low = emit_low_n(c, inp["low"], inp["max_low"], num_img)
    phases, amps = [], []
    for idx in range(m):
        size = tuple(inp["phase"][idx].shape[2:])
        x = torch.cat((resize(f, size), inp["phase"][idx], inp["amp"][idx], resize(c, size)), 1)
        i = idx + 1 if idx + 1 < len(P) - 1 else len(P) - 1
        f, c = R.block(P[i], x)
        ph, am = emit_n(c, inp["amp"][idx], inp["max_amp"][idx], num_img)
        phases.append(ph.reshape(-1, 1, *size))
        amps.append(am.reshape(-1, 1, *size))
    return low, phases, amps
