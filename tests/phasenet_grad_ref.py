"""Host models and float64 restatements for the PhaseNet block backward, shared by
tests/test_phasenet_grad_host.py (CPU) and tests/test_phasenet_block_backward_gpu.py.

  * the arbitrary-size bilinear resize (align_corners=False) and its adjoint, with the index and weight arithmetic in
    float32 exactly as resize_bilinear_kernel / resize_adjoint_kernel do it and the sums in float64;
  * the activation, blend and BatchNorm-unfold formulas of the backward as numpy / torch expressions;
  * a torch restatement of one PhaseNetBlock (reflect-padded convolutions, eval-mode BatchNorm, ELU, tanh), of the level
    step built from it, and of the reference's loss (src/train/loss.py:5-26).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


# ---- resize ----------------------------------------------------------------------------------------------------------
def resize_taps(o, n_in, n_out):
    """(i0, i1, l) of output o of an axis resized n_in -> n_out: the kernels' fp32 arithmetic, operation by operation."""
    s = f32(n_in) / f32(n_out)
    f = max(f32(f32(s * f32(f32(o) + f32(0.5))) - f32(0.5)), f32(0.0))
    i0 = min(int(f), n_in - 1)
    i1 = min(i0 + 1, n_in - 1)
    return i0, i1, f32(f - f32(i0))


def resize_matrix(n_in, n_out):
    """R (n_out, n_in) float64 holding the fp32 weights (1 - l at i0, l at i1; both on one source at the clamped edge)."""
    r = np.zeros((n_out, n_in))
    for o in range(n_out):
        i0, i1, l = resize_taps(o, n_in, n_out)
        r[o, i0] += float(f32(1.0) - l)
        r[o, i1] += float(l)
    return r


def resize_forward(x, size):
    """x (..., h, w) float64 -> (..., H, W)."""
    ry, rx = resize_matrix(x.shape[-2], size[0]), resize_matrix(x.shape[-1], size[1])
    return ry @ x @ rx.T


def resize_adjoint(g, size):
    """g (..., H, W) float64 -> (..., h, w): the transpose of resize_forward."""
    ry, rx = resize_matrix(size[0], g.shape[-2]), resize_matrix(size[1], g.shape[-1])
    return ry.T @ g @ rx


def resize_candidates(s, n_in, n_out):
    """[lo, hi] of resize_candidates in csrc/vfi_phasenet_grad.hip (integer arithmetic; python's // is a floor)."""
    a, b, d = (2 * s - 1) * n_out - n_in, (2 * s + 3) * n_out - n_in, 2 * n_in
    lo, hi = a // d - 1, -((-b) // d) + 1
    if s == 0:
        lo = 0
    if s == n_in - 1:
        hi = n_out - 1
    return max(lo, 0), min(hi, n_out - 1)


def resize_adjoint_gather(g, size):
    """The kernel's gather form, loop for loop: per source the candidate outputs, each re-evaluated with the forward's
    arithmetic and accepted when it hits the source."""
    (h, w), (H, W) = size, g.shape[-2:]
    out = np.zeros(g.shape[:-2] + (h, w))

    def hits(s, n_in, n_out):
        lo, hi = resize_candidates(s, n_in, n_out)
        res = []
        for o in range(lo, hi + 1):
            i0, i1, l = resize_taps(o, n_in, n_out)
            wt = (float(f32(1.0) - l) if i0 == s else 0.0) + (float(l) if i1 == s else 0.0)
            if wt != 0.0:
                res.append((o, wt))
        return res
    cols = [hits(x, w, W) for x in range(w)]
    for y in range(h):
        for oy, wy in hits(y, h, H):
            for x in range(w):
                for ox, wx in cols[x]:
                    out[..., y, x] += wy * wx * g[..., oy, ox]
    return out


# ---- elementwise adjoints --------------------------------------------------------------------------------------------
def elu_backward(g, y):
    return np.where(y > 0, g, g * (y + 1.0))


def tanh_backward(g, y):
    return g * (1.0 - y * y)


def emit(pred, amp_in, max_amp):
    """vfi_phasenet_emit: pred, amp_in (N,8,H,W), max_amp (N,) -> phase, amp (N,4,H,W).  Works on numpy and torch."""
    beta = (pred[:, 4:8] + 1) / 2
    return pred[:, 0:4] * math.pi, (beta * amp_in[:, 4:8] + (1 - beta) * amp_in[:, 0:4]) * max_amp.reshape(-1, 1, 1, 1)


def emit_low(pred, low_in, max_low):
    alpha = (pred[:, 0] + 1) / 2
    return ((alpha * low_in[:, 0] + (1 - alpha) * low_in[:, 1]) * max_low.reshape(-1, 1, 1))[:, None]


def emit_backward(g_phase, g_amp, amp_in, max_amp):
    g = np.zeros(amp_in.shape)
    if g_phase is not None:
        g[:, 0:4] = math.pi * g_phase
    if g_amp is not None:
        g[:, 4:8] = g_amp * max_amp.reshape(-1, 1, 1, 1) * (amp_in[:, 4:8] - amp_in[:, 0:4]) / 2
    return g


def emit_low_backward(g_low, low_in, max_low):
    return g_low * max_low.reshape(-1, 1, 1, 1) * (low_in[:, 0:1] - low_in[:, 1:2]) / 2


def bn_unfold(g_wf, g_bf, w, b, gamma, mean, var, eps):
    """Gradients of (w, b, gamma, beta) from those of the folded wf = w s, bf = (b - mean) s + beta, s = gamma / sqrt(var + eps)."""
    inv = 1.0 / torch.sqrt(var + eps)
    s = gamma * inv
    return (g_wf * s.view(-1, 1, 1, 1), g_bf * s, ((g_wf * w).sum((1, 2, 3)) + g_bf * (b - mean)) * inv, g_bf)


# ---- the block, the level step and the loss as torch expressions --------------------------------------------------------
BLOCK_KEYS = ("feature_map.0.weight", "feature_map.0.bias", "feature_map.1.weight", "feature_map.1.bias",
              "feature_map.3.weight", "feature_map.3.bias", "prediction_map.0.weight", "prediction_map.0.bias")


def block_state(seed, cin, pred, ks, cout=64):
    """Seeded state dict of one PhaseNetBlock: torch's default convolution scale, gamma in [0.5, 1.5], running mean ~ N(0, 0.3)
    and running variance in [0.5, 2] (not the 0 / 1 of a fresh BatchNorm)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    b1, b2 = 1.0 / math.sqrt(cin * ks * ks), 1.0 / math.sqrt(cout * ks * ks)
    bp = 1.0 / math.sqrt(cout)
    return {"feature_map.0.weight": u((cout, cin, ks, ks), -b1, b1), "feature_map.0.bias": u((cout,), -b1, b1),
            "feature_map.1.weight": u((cout,), 0.5, 1.5), "feature_map.1.bias": torch.randn(cout, generator=g) * 0.1,
            "feature_map.1.running_mean": torch.randn(cout, generator=g) * 0.3, "feature_map.1.running_var": u((cout,), 0.5, 2.0),
            "feature_map.1.num_batches_tracked": torch.tensor(0, dtype=torch.long),
            "feature_map.3.weight": u((cout, cout, ks, ks), -b2, b2), "feature_map.3.bias": u((cout,), -b2, b2),
            "prediction_map.0.weight": u((pred, cout, 1, 1), -bp, bp), "prediction_map.0.bias": u((pred,), -bp, bp)}


def block(P, x, eps=1e-5):
    """(f, c) of reference block.py:15-32 with the BatchNorm in eval mode; P: a block state dict (any float dtype)."""
    ks = P["feature_map.0.weight"].shape[2]

    def conv(t, w, b):
        if ks == 3:
            t = F.pad(t, (1, 1, 1, 1), mode="reflect")
        return F.conv2d(t, w, b)
    t = conv(x, P["feature_map.0.weight"], P["feature_map.0.bias"])
    t = F.batch_norm(t, P["feature_map.1.running_mean"], P["feature_map.1.running_var"], P["feature_map.1.weight"],
                     P["feature_map.1.bias"], False, 0.0, eps)
    f = F.elu(conv(F.elu(t), P["feature_map.3.weight"], P["feature_map.3.bias"]))
    return f, torch.tanh(F.conv2d(f, P["prediction_map.0.weight"], P["prediction_map.0.bias"]))


def wrap(d):
    return torch.atan2(torch.sin(d), torch.cos(d))


def phase_term(phase_o, phase_t, nbands):
    """loss.py:11-16 for one level, orientation by orientation."""
    r = phase_o.reshape(-1, nbands, phase_o.shape[2], phase_o.shape[3]).permute(1, 0, 2, 3)
    g = phase_t.reshape(-1, nbands, phase_o.shape[2], phase_o.shape[3]).permute(1, 0, 2, 3)
    return sum(torch.mean(torch.abs(wrap(og - orr).reshape(-1)), 0) for orr, og in zip(r, g))


def get_loss(phases_o, phases_t, output, target, nbands, weighting_factor=0.005):
    """loss.py:5-26 restated -> (total_loss, l_1_p, phase_loss_p)."""
    phase_loss = sum(phase_term(o, t, nbands) for o, t in zip(phases_o, phases_t))
    l_1 = torch.mean(torch.abs(output - target))
    total = l_1 + weighting_factor * phase_loss
    return total, 100 * l_1.detach() / total, 100 * weighting_factor * phase_loss.detach() / total


def level_step(P0, P1, data, resize, blk=block, blend=None, blend_low_=None, phase_loss=None, l1=None):
    """One composed level (phase_net.py:113-116, 138-168): block 0 on the low level, resize of cat(f, c), cat with the
    level's phase and amplitude in the reference's order, block 1, both blends, then 0.005 * phase term + L1 on the
    amplitudes + L1 on the low level.  `resize(x, size)` and the optional callables let the product's pieces be plugged
    into the same walk; data: dict of tensors (low_in, max_low, phase, amp, max_amp, phase_t, amp_t, low_t)."""
    blend = blend or (lambda c, a, m: tuple(t.reshape(-1, 1, *t.shape[2:]) for t in emit(c, a, m)))
    blend_low_ = blend_low_ or emit_low
    phase_loss = phase_loss or (lambda o, t: phase_term(o, t, 4))
    l1 = l1 or (lambda a, b: torch.mean(torch.abs(a - b)))
    f0, c0 = blk(P0, data["low_in"])
    size = tuple(data["phase"].shape[2:])
    r = resize(torch.cat((f0, c0), 1), size)
    x1 = torch.cat((r[:, :64], data["phase"], data["amp"], r[:, 64:]), 1)
    _, c1 = blk(P1, x1)
    phase_out, amp_out = blend(c1, data["amp"], data["max_amp"])
    low_out = blend_low_(c0, data["low_in"], data["max_low"])
    return 0.005 * phase_loss(phase_out, data["phase_t"]) + l1(amp_out, data["amp_t"]) + l1(low_out, data["low_t"])


def torch_resize(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)
