"""Float64 restatements for PhaseNet on batch-statistics BatchNorm, shared by
tests/test_phasenet_bn_host.py (CPU), tests/test_phasenet_bn_gpu.py and tests/golden/make_golden_phasenet_walk_bn.py:

  * one PhaseNetBlock with its BatchNorm in training mode (reference src/phase_net/block.py:15-32, never switched to eval by
    src/train/trainer.py:107-134) and the coarse-to-fine walk built from it, on top of phasenet_grad_ref / phasenet_walk_ref;
    the running statistics in the parameter dicts move as nn.BatchNorm2d's do;
  * the closed forms of the three entry points: the two-stage (count, mean, M2) statistics with Chan's merge, the
    normalise + activation pass, its adjoint, and the running-statistics update.
"""
import numpy as np
import torch
import torch.nn.functional as F

import phasenet_grad_ref as R
import phasenet_walk_ref as W

MOMENTUM = 0.1          # nn.BatchNorm2d's default, which block.py:17 takes
f32 = np.float32


# ---- the block and the walk ---------------------------------------------------------------------------------------------
def block(P, x, eps=1e-5):
    """(f, c) of reference block.py:15-32 with the BatchNorm in TRAINING mode: the batch's statistics normalise, and
    P's running_mean / running_var / num_batches_tracked are updated (in place for the two float buffers)."""
    ks = P["feature_map.0.weight"].shape[2]

    def conv(t, w, b):
        if ks == 3:
            t = F.pad(t, (1, 1, 1, 1), mode="reflect")
        return F.conv2d(t, w, b)
    y = conv(x, P["feature_map.0.weight"], P["feature_map.0.bias"])
    t = F.batch_norm(y, P["feature_map.1.running_mean"], P["feature_map.1.running_var"], P["feature_map.1.weight"],
                     P["feature_map.1.bias"], True, MOMENTUM, eps)
    P["feature_map.1.num_batches_tracked"] = P["feature_map.1.num_batches_tracked"] + 1
    f = F.elu(conv(F.elu(t), P["feature_map.3.weight"], P["feature_map.3.bias"]))
    return f, torch.tanh(F.conv2d(f, P["prediction_map.0.weight"], P["prediction_map.0.bias"]))


def walk(P, inp, m, resize=R.torch_resize):
    """phasenet_walk_ref.walk with every block on batch statistics: the last block takes fresh statistics at each level it
    serves and updates its running statistics once per level, coarse to fine."""
    f, c = block(P[0], inp["low"])
    low = R.emit_low(c, inp["low"], inp["max_low"])
    phases, amps = [], []
    for idx in range(m):
        size = tuple(inp["phase"][idx].shape[2:])
        x = torch.cat((resize(f, size), inp["phase"][idx], inp["amp"][idx], resize(c, size)), 1)
        i = idx + 1 if idx + 1 < len(P) - 1 else len(P) - 1
        f, c = block(P[i], x)
        ph, am = R.emit(c, inp["amp"][idx], inp["max_amp"][idx])
        phases.append(ph.reshape(-1, 1, *size))
        amps.append(am.reshape(-1, 1, *size))
    return low, phases, amps


BUFFERS = ("feature_map.1.running_mean", "feature_map.1.running_var", "feature_map.1.num_batches_tracked")


def named_buffers(P):
    return {f"layers.{i}.{k}": P[i][k] for i in range(len(P)) for k in BUFFERS}


# ---- closed forms of the entry points -------------------------------------------------------------------------------------
def chan_merge(a, b, dtype=f32):
    """(n, mean, M2) of two runs merged by Chan's formula, every operation rounded to `dtype`; an empty side is skipped."""
    (na, ma, qa), (nb, mb, qb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    t = dtype
    n, d = t(na + nb), t(mb - ma)
    r = t(t(nb) / n)
    return n, t(ma + t(d * r)), t(t(qa + qb) + t(t(t(d * d) * t(na)) * r))


def chan_stats(x, block=256, dtype=f32):
    """(mean, biased variance) of the 1-d array x the way vfi_bn_stats forms them: (count, mean, M2) of each run of `block`
    values (a two-pass in `dtype`), merged in run order by Chan's formula in `dtype`."""
    x = np.asarray(x, dtype=dtype).ravel()
    acc = (dtype(0), dtype(0), dtype(0))
    for s in range(0, x.size, block):
        run = x[s:s + block]
        m = dtype(run[0] + dtype((run - run[0]).sum(dtype=dtype) / dtype(run.size)))      # exact on a constant run
        acc = chan_merge(acc, (dtype(run.size), m, dtype(((run - m) ** 2).sum(dtype=dtype))), dtype)
    return acc[1], dtype(acc[2] / acc[0])


def naive_stats(x, dtype=f32):
    """The form vfi_bn_stats must not take: E[x^2] - E[x]^2 in `dtype`."""
    x = np.asarray(x, dtype=dtype).ravel()
    m = dtype(x.sum(dtype=dtype) / dtype(x.size))
    return m, dtype(dtype((x * x).sum(dtype=dtype) / dtype(x.size)) - dtype(m * m))


def batch_stats(y):
    """(mean, biased var) per channel of y (N,C,...), torch or numpy, in y's own precision."""
    y = torch.as_tensor(y)
    dims = [0] + list(range(2, y.dim()))
    return y.mean(dims), y.var(dims, unbiased=False)


def _cv(v, y):
    return v.reshape(1, -1, *([1] * (y.dim() - 2)))


def bn_act_forward(y, mean, var, gamma, beta, eps, act="elu"):
    """vfi_bn_act_forward: act(gamma (y - mean) / sqrt(var + eps) + beta)."""
    z = (y - _cv(mean, y)) * _cv(gamma / torch.sqrt(var + eps), y) + _cv(beta, y)
    return F.elu(z) if act == "elu" else z


def bn_act_backward(g_t, t, y, mean, var, gamma, eps, act="elu"):
    """vfi_bn_act_backward's formulas -> (g_y, g_gamma, g_beta); ELU' from the output t."""
    g_z = torch.where(t > 0, g_t, g_t * (t + 1)) if act == "elu" else g_t
    inv = 1.0 / torch.sqrt(var + eps)
    xh = (y - _cv(mean, y)) * _cv(inv, y)
    dims = [0] + list(range(2, y.dim()))
    n = y.numel() // y.shape[1]
    g_beta, g_gamma = g_z.sum(dims), (g_z * xh).sum(dims)
    return _cv(gamma * inv, y) * (g_z - _cv(g_beta, y) / n - xh * _cv(g_gamma, y) / n), g_gamma, g_beta


def running_update(running_mean, running_var, mean, var, n, momentum=MOMENTUM):
    """nn.BatchNorm2d's update from the batch's mean and BIASED variance over n values per channel."""
    return (1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var * n / (n - 1)


# ---- the statistics' criterion ------------------------------------------------------------------------------------------------
# (n, mean, sigma) of the issue's table; the last is the offset channel on which E[y^2] - E[y]^2 loses the variance
STAT_INPUTS = [(n, mu, sd) for n in (3, 12, 3069, 12300) for mu, sd in ((0.0, 1.0), (-3.0, 2.0))] + [(12300, 100.0, 0.1)]


def stat_input(n, mu, sd):
    g = torch.Generator().manual_seed(n + int(mu * 7))
    return (torch.randn(n, generator=g, dtype=torch.float64) * sd + mu).float().numpy()


def stat_criterion(mean, var, x):
    """|mean error| <= 1e-6 |mu| + 1e-5 sigma and variance relative error <= 1e-5, against float64 on the float32 values."""
    x64 = x.astype(np.float64)
    mu, v = x64.mean(), x64.var()
    return abs(float(mean) - mu) <= 1e-6 * abs(mu) + 1e-5 * np.sqrt(v), abs(float(var) - v) <= 1e-5 * v
