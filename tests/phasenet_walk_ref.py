"""Float64 restatements for the whole PhaseNet's backward, shared by tests/test_phasenet_walk_host.py
(CPU), tests/test_phasenet_walk_backward_gpu.py and tests/golden/make_golden_phasenet_walk.py:

  * seeded weights of the eight blocks and seeded normalised inputs of a small pyramid;
  * the coarse-to-fine walk of reference src/phase_net/phase_net.py:107-177 (`phasenet_grad_ref.level_step` generalised to L
    levels, m, and the last block shared by every level from index 7 on) with reverse_normalize folded in;
  * the hierarchical form of reference src/phase_net/architecture.py:38-71 from given analysis outputs;
  * the formulas of the head adjoint (vfi_phasenet_predict_backward).
"""
import math

import torch

import phasenet_grad_ref as R

BLOCKS = [(2, 1, 1), (81, 8, 1)] + [(88, 8, 1)] + [(88, 8, 3)] * 5         # (c_in, pred_out, kernel) of phase_net.py:30-35
S2 = math.sqrt(2)


def net_state(seed):
    """Seeded state dict of PhaseNet.layers (keys `layers.<i>.<block key>`), each block drawn by R.block_state."""
    return {f"layers.{i}.{k}": v for i, (cin, pred, ks) in enumerate(BLOCKS)
            for k, v in R.block_state(seed * 100 + i, cin, pred, ks).items()}


def block_params(sd, i, dtype=torch.float64, grad=True):
    """Block i's tensors of a net state dict as `dtype` leaves (the BatchNorm buffers do not require grad)."""
    pre = f"layers.{i}."
    return {k[len(pre):]: (v.to(dtype).clone().requires_grad_(grad and k[len(pre):] in R.BLOCK_KEYS)
                           if v.dtype.is_floating_point else v) for k, v in sd.items() if k.startswith(pre)}


def net_params(sd, dtype=torch.float64):
    return [block_params(sd, i, dtype) for i in range(len(BLOCKS))]


def level_sizes(h, w, nlev):
    """Band-level sizes, finest first, then the low residual's: each ceil(previous / sqrt 2) (the pyramid's rule)."""
    sizes = [(h, w)]
    for _ in range(nlev):
        sizes.append((int(math.ceil(sizes[-1][0] / S2)), int(math.ceil(sizes[-1][1] / S2))))
    return sizes


def seeded_inputs(seed, n, h, w, height):
    """Normalised inputs as PhaseNet.normalize_vals returns them, lists COARSEST first: phase in [-1, 1], amplitudes in
    [0, 1], low level in [-1, 1], maxima in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    sizes = level_sizes(h, w, height - 2)
    bands = sizes[:-1][::-1]
    return {"low": u((n, 2, *sizes[-1]), -1, 1), "max_low": u((n,), 0.5, 1.5), "high_shape": (n, 2, h, w),
            "phase": [u((n, 8, *s), -1, 1) for s in bands], "amp": [u((n, 8, *s), 0, 1) for s in bands],
            "max_amp": [u((n,), 0.5, 1.5) for _ in bands]}


def to_dtype(inp, dtype=torch.float64, device=None):
    f = lambda t: t.to(dtype=dtype, device=device) if torch.is_tensor(t) else t
    return {k: [f(t) for t in v] if isinstance(v, list) else f(v) for k, v in inp.items()}


def walk(P, inp, m, resize=R.torch_resize):
    """phase_net.py:107-177 with reverse_normalize (:80-105): P a list of block parameter dicts, inp as seeded_inputs ->
    (low (N,1,hL,wL), [phase_out], [amp_out]) of the m coarsest levels, COARSEST first, each (N*4,1,h,w)."""
    f, c = R.block(P[0], inp["low"])
    low = R.emit_low(c, inp["low"], inp["max_low"])
    phases, amps = [], []
    for idx in range(m):
        size = tuple(inp["phase"][idx].shape[2:])
        x = torch.cat((resize(f, size), inp["phase"][idx], inp["amp"][idx], resize(c, size)), 1)
        i = idx + 1 if idx + 1 < len(P) - 1 else len(P) - 1
        f, c = R.block(P[i], x)
        ph, am = R.emit(c, inp["amp"][idx], inp["max_amp"][idx])
        phases.append(ph.reshape(-1, 1, *size))
        amps.append(am.reshape(-1, 1, *size))
    return low, phases, amps


def walk_targets(seed, low, phases, amps):
    """Targets a fixed distance from the float64 outputs: |wrap(phase_t - phase)| in [0.05, pi - 0.05], |amp_t - amp| and
    |low_t - low| in [0.01, 0.5] -- neither the cut of atan2 nor the kink of |.| is within reach of float32 rounding."""
    g = torch.Generator().manual_seed(seed)
    u = lambda t, lo, hi: (torch.rand(t.shape, generator=g, dtype=torch.float64) * (hi - lo) + lo) * \
        (torch.randint(0, 2, t.shape, generator=g).double() * 2 - 1)
    return {"low": (low.detach().double() + u(low, 0.01, 0.5)).float(),
            "phase": [(p.detach().double() + u(p, 0.05, math.pi - 0.05)).float() for p in phases],
            "amp": [(a.detach().double() + u(a, 0.01, 0.5)).float() for a in amps]}


def walk_loss(low, phases, amps, tgt, phase_term=None, l1=None):
    """0.005 * phase term + L1 on the amplitudes per level, + L1 on the low level (level_step's loss over all levels)."""
    phase_term = phase_term or (lambda o, t: R.phase_term(o, t, 4))
    l1 = l1 or (lambda a, b: torch.mean(torch.abs(a - b)))
    total = l1(low, tgt["low"])
    for p, a, pt, at in zip(phases, amps, tgt["phase"], tgt["amp"]):
        total = total + 0.005 * phase_term(p, pt) + l1(a, at)
    return total


def named_grads(P):
    return {f"layers.{i}.{k}": P[i][k].grad for i in range(len(P)) for k in R.BLOCK_KEYS}


# ---- the head adjoint's formulas -----------------------------------------------------------------------------------------
def head_forward(f, w, b, amp_in, max_amp):
    """vfi_phasenet_predict: f (N,64,H,W), w (8,64), b (8,) -> (pred, phase (N,4,H,W), amp (N,4,H,W)); torch, any dtype."""
    pred = torch.tanh(torch.einsum("jk,nkhw->njhw", w, f) + b.view(1, -1, 1, 1))
    return (pred, *R.emit(pred, amp_in, max_amp))


def head_backward(f, pred, amp_in, max_amp, w, g_phase=None, g_amp=None, g_pred_in=None):
    """vfi_phasenet_predict_backward's formulas -> (grad_f, grad_w (8,64), grad_b (8,)); None = zero."""
    g = torch.zeros_like(pred)
    if g_phase is not None:
        g[:, 0:4] = math.pi * g_phase
    if g_amp is not None:
        g[:, 4:8] = g_amp * max_amp.view(-1, 1, 1, 1) * (amp_in[:, 4:8] - amp_in[:, 0:4]) / 2
    if g_pred_in is not None:
        g = g + g_pred_in
    gz = g * (1 - pred * pred)
    return torch.einsum("jk,njhw->nkhw", w, gz), torch.einsum("njhw,nkhw->jk", gz, f), gz.sum((0, 2, 3))


# ---- architecture.PhaseNet.forward, hierarchical form ---------------------------------------------------------------------
def normalize(vals_in, eps=1e-8):
    """phase_net.py:42-78 on concatenated inputs {low (N,2,..), phase [..], amp [..]} (coarsest first) -> walk inputs."""
    n = vals_in["low"].shape[0]
    mx = lambda t: t.reshape(n, -1).max(1)[0] + eps
    max_amp = [mx(a) for a in vals_in["amp"]]
    max_low = mx(vals_in["low"])
    return {"low": vals_in["low"] / max_low.view(-1, 1, 1, 1), "max_low": max_low,
            "phase": [p / math.pi for p in vals_in["phase"]],
            "amp": [a / m_.view(-1, 1, 1, 1) for a, m_ in zip(vals_in["amp"], max_amp)], "max_amp": max_amp}
