"""Float64 restatements for the backward of PhaseNet with three and four input images, shared by
tests/test_phasenet_fusion_grad_host.py (CPU), tests/test_phasenet_fusion_grad_gpu.py and
tests/golden/make_golden_phasenet_fusion_grad.py:

  * the coarse-to-fine walk of tests/phasenet_fusion_ref.py with leaves that require grad, on the running statistics and on
    the batch's (tests/phasenet_bn_ref.py's block);
  * seeded normalised inputs of a small pyramid with num_img images;
  * the closed forms of the three adjoints: vfi_phasenet_emit_n_backward, vfi_phasenet_emit_low_n_backward and
    vfi_phasenet_predict_n_backward.
"""
import math

import torch

import phasenet_bn_ref as B
import phasenet_fusion_ref as FR
import phasenet_grad_ref as R
import phasenet_walk_ref as W


def net_params(sd, dtype=torch.float64):
    """Leaves that require grad (the BatchNorm buffers do not) of a PhaseNet(num_img) state dict, one dict per block."""
    return [W.block_params(sd, i, dtype) for i in range(8)]


def seeded_inputs(seed, n, h, w, height, num_img):
    """phasenet_walk_ref.seeded_inputs with num_img images: normalised values, lists COARSEST first."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    sizes = W.level_sizes(h, w, height - 2)
    bands = sizes[:-1][::-1]
    return {"low": u((n, num_img, *sizes[-1]), -1, 1), "max_low": u((n,), 0.5, 1.5), "high_shape": (n, num_img, h, w),
            "phase": [u((n, 4 * num_img, *s), -1, 1) for s in bands], "amp": [u((n, 4 * num_img, *s), 0, 1) for s in bands],
            "max_amp": [u((n,), 0.5, 1.5) for _ in bands]}


walk = FR.walk              # running statistics: (P, inp, m, num_img) -> (low, [phase], [amp]) coarsest first


def bn_walk(P, inp, m, num_img, resize=R.torch_resize):
    """FR.walk with every block on batch statistics (phasenet_bn_ref.block): the running statistics in P move."""
    f, c = B.block(P[0], inp["low"])
    low = FR.emit_low_n(c, inp["low"], inp["max_low"], num_img)
    phases, amps = [], []
    for idx in range(m):
        size = tuple(inp["phase"][idx].shape[2:])
        x = torch.cat((resize(f, size), inp["phase"][idx], inp["amp"][idx], resize(c, size)), 1)
        i = idx + 1 if idx + 1 < len(P) - 1 else len(P) - 1
        f, c = B.block(P[i], x)
        ph, am = FR.emit_n(c, inp["amp"][idx], inp["max_amp"][idx], num_img)
        phases.append(ph.reshape(-1, 1, *size))
        amps.append(am.reshape(-1, 1, *size))
    return low, phases, amps


# ---- closed forms of the three adjoints -------------------------------------------------------------------------------------
def emit_n_backward(g_phase, g_amp, pred, amp_in, max_amp, num_img):
    """vfi_phasenet_emit_n_backward: g_phase, g_amp (N,4,H,W) or None (= zero) -> grad_pred (N,8|12,H,W).  Planes 8.. of
    amp_in are read for three images only."""
    g = torch.zeros_like(pred)
    if g_phase is not None:
        g[:, 0:4] = math.pi * g_phase
    if g_amp is not None:
        gm = g_amp * max_amp.view(-1, 1, 1, 1)
        d = (amp_in[:, 4:8] - amp_in[:, 0:4]) / 2
        if num_img == 3:
            b, fb = (pred[:, 4:8] + 1) / 2, (pred[:, 8:12] + 1) / 2
            amp1 = b * amp_in[:, 4:8] + (1 - b) * amp_in[:, 0:4]
            g[:, 4:8] = gm * fb * d
            g[:, 8:12] = gm * (amp1 - amp_in[:, 8:12]) / 2
        else:
            g[:, 4:8] = gm * d
    return g


def emit_low_n_backward(g_low, pred, low_in, max_low, num_img):
    """vfi_phasenet_emit_low_n_backward: g_low (N,1,H,W) -> grad_pred (N,1|2,H,W)."""
    gm = g_low * max_low.view(-1, 1, 1, 1)
    d = (low_in[:, 0:1] - low_in[:, 1:2]) / 2
    if num_img != 3:
        return gm * d
    a, fa = (pred[:, 0:1] + 1) / 2, (pred[:, 1:2] + 1) / 2
    low1 = a * low_in[:, 0:1] + (1 - a) * low_in[:, 1:2]
    return torch.cat((gm * fa * d, gm * (low1 - low_in[:, 2:3]) / 2), 1)


def head_forward(f, w, b, amp_in, max_amp, num_img):
    """vfi_phasenet_predict_n: f (N,64,H,W), w (P,64), b (P,) -> (pred, phase (N,4,H,W), amp (N,4,H,W))."""
    pred = torch.tanh(torch.einsum("jk,nkhw->njhw", w, f) + b.view(1, -1, 1, 1))
    return (pred, *FR.emit_n(pred, amp_in, max_amp, num_img))


def head_backward(f, pred, amp_in, max_amp, w, num_img, g_phase=None, g_amp=None, g_pred_in=None):
    """vfi_phasenet_predict_n_backward's formulas -> (grad_f, grad_w (P,64), grad_b (P,)); None = zero."""
    if g_phase is None and g_amp is None:
        g = torch.zeros_like(pred)
    else:
        g = emit_n_backward(g_phase, g_amp, pred, amp_in, max_amp, num_img)
    if g_pred_in is not None:
        g = g + g_pred_in
    gz = g * (1 - pred * pred)
    return torch.einsum("jk,njhw->nkhw", w, gz), torch.einsum("njhw,nkhw->jk", gz, f), gz.sum((0, 2, 3))
