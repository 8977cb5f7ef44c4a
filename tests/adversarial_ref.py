"""Plain-torch restatements for the discriminator tests: the phase split and the expanded stride-2
filter by indexing, the discriminator's layout written out, and its forward as a function of an ordered parameter list, in
any dtype, with optional LeakyReLU masks.  No GPU, no vfi_amd import."""
import types

import torch
import torch.nn.functional as F

SLOPE = 0.2
EPS = 1e-5
MOMENTUM = 0.1
# (in, out, stride) of the eight blocks for 3 input channels; FI: the first `in` is 6
BLOCKS = [(3, 64, 1), (64, 64, 2), (64, 128, 1), (128, 128, 2), (128, 256, 1), (256, 256, 2), (256, 512, 1), (512, 512, 2)]
TAP = ((1, 0), (0, 1), (1, 1))      # tap k of the stride-2 filter -> (phase, tap) of the stride-1 filter


def args(patch_size, **kw):
    base = dict(patch_size=patch_size, optimizer='ADAMax', lr=1e-3, weight_decay=0, decay_type='step', lr_decay=20, gamma=0.5,
                gpu_id=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def layout(patch_size, in_channels=3):
    """{state_dict key: shape} of Discriminator / FI_Discriminator, written out."""
    out = {}
    for i, (cin, cout, _) in enumerate(BLOCKS):
        cin = in_channels if i == 0 else cin
        out[f"features.{i}.0.weight"] = (cout, cin, 3, 3)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"features.{i}.1.{k}"] = (cout,)
        out[f"features.{i}.1.num_batches_tracked"] = ()
    p = patch_size // 16
    out["classifier.0.weight"] = (1024, 512 * p * p)
    out["classifier.0.bias"] = (1024,)
    out["classifier.2.weight"] = (1, 1024)
    out["classifier.2.bias"] = (1,)
    return out


def param_keys():
    """The order of the autograd node's parameters."""
    keys = []
    for i in range(len(BLOCKS)):
        keys += [f"features.{i}.0.weight", f"features.{i}.1.weight", f"features.{i}.1.bias"]
    return keys + ["classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias"]


def phase_split(x):
    """xs[n, (2 py + px) C + c, i, j] = x[n, c, 2 i + py, 2 j + px], zero beyond the edge, by indexing."""
    n, c, h, w = x.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    xp = x.new_zeros((n, c, 2 * h2, 2 * w2))
    xp[:, :, :h, :w] = x
    return torch.cat([xp[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], dim=1)


def phase_merge(gs, size):
    h, w = size
    n, c4, h2, w2 = gs.shape
    c = c4 // 4
    full = gs.new_zeros((n, c, 2 * h2, 2 * w2))
    for py in (0, 1):
        for px in (0, 1):
            full[:, :, py::2, px::2] = gs[:, (2 * py + px) * c:(2 * py + px + 1) * c]
    return full[:, :, :h, :w].contiguous()


def stride2_weight(w):
    cout, c = w.shape[:2]
    out = w.new_zeros((cout, 4, c, 3, 3))
    for ky in range(3):
        for kx in range(3):
            (py, ty), (px, tx) = TAP[ky], TAP[kx]
            out[:, 2 * py + px, :, ty, tx] = w[:, :, ky, kx]
    return out.reshape(cout, 4 * c, 3, 3)


def _leaky(z, mask):
    if mask is None:
        return F.leaky_relu(z, SLOPE)
    return z * torch.where(mask, torch.ones((), dtype=z.dtype), torch.full((), SLOPE, dtype=z.dtype))


def forward(params, x, masks=None, stats=None):
    """Logits (B, 1) of the discriminator in training mode from the ordered parameters (param_keys()), in their dtype.
    masks: 9 bool tensors (the eight blocks' outputs > 0, the hidden layer's > 0) fixing every LeakyReLU's branch; None:
    the sign of this forward's own values.  stats: a list that receives (mean, biased var, count) per block."""
    t = x
    for i, (_, _, stride) in enumerate(BLOCKS):
        w, gamma, beta = params[3 * i:3 * i + 3]
        y = F.conv2d(t, w, stride=stride, padding=1)
        if y.shape[0] * y.shape[2] * y.shape[3] < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        if stats is not None:
            stats.append((mean.detach(), var.detach(), y.shape[0] * y.shape[2] * y.shape[3]))
        z = (y - mean.view(1, -1, 1, 1)) * (gamma / torch.sqrt(var + EPS)).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        t = _leaky(z, None if masks is None else masks[i])
    l1w, l1b, l2w, l2b = params[24:]
    hid = _leaky(F.linear(t.flatten(1), l1w, l1b), None if masks is None else masks[8])
    return F.linear(hid, l2w, l2b)


def gradients(params, x, masks, dtype, upstream):
    """(logits, dx, [dparam]) of sum(logits * upstream) by autograd in `dtype` on the CPU."""
    ps = [p.detach().cpu().to(dtype).requires_grad_(True) for p in params]
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    out = forward(ps, xd, [m.cpu() for m in masks])
    grads = torch.autograd.grad((out * upstream.cpu().to(dtype)).sum(), [xd] + ps)
    return out.detach(), grads[0], list(grads[1:])


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
