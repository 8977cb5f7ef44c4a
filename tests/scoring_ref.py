"""Plain CPU references of the scoring kernels (csrc/vfi_image.hip: vfi_diff_sums, vfi_ssim_sum, vfi_mul, vfi_avg_pool,
and the Gaussian behind vfi_amd.evaluation.evaluate_image.ssim), the inputs and cases their tests share, and the mistakes
planted to show that those tests can fail (tests/test_scoring_host.py, tests/test_scoring_gpu.py).  torch / numpy only.

Inputs.  A mean of SSIM over homogeneous noise does not move when the interior is walked transposed, the border is off by
one or the pooling factor is wrong: every pixel holds the same value.  `structured_pair` makes the local SSIM depend on
the position, differently along the rows and along the columns (the distortion grows as x^2 and linearly in y), so that
each of those mistakes moves the mean by far more than the bound the kernels are held to.

Bounds.  An SSIM case is held to max(2e-5, 4 * mean|map32 - map64|): 2e-5 is the tolerance the project already states for
SSIM (test_evaluate_image_matches_reference_expressions), the second term is what one valid float32 evaluation of the
published formula loses per pixel on these inputs, with glue_ref's factor 4.  A vfi_ssim_sum case is held to
n_valid * glue_ref.tol_of(map32, map64): glue_ref's per-element rule, summed over the pixels the kernel adds."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from glue_ref import tol_of

KS, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03            # piq.ssim defaults
U53 = 2.0 ** -53


def pool_factor(h, w):
    """piq.ssim: f = max(1, round(min(H, W) / 256)), Python's round (half to even)."""
    return max(1, round(min(h, w) / 256))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def structured_pair(shape, seed):
    """(p, t) float32 (C,H,W) in [0,1]: a smooth pattern with texture, and a copy whose distortion grows across the frame.

    The texture and the distortion are drawn once per f x f block, f the pooling factor of the shape, and with amplitude
    0.3.  With one draw per pixel at amplitude 0.15 the pooled images keep so little local variance (about 1e-4 at f = 4)
    that sxx = E[xx] - mu^2 cancels seven digits: the float32 reference then loses 4e-5 to 7e-5 per pixel, the bound
    4 * mean|map32 - map64| grows to 1.5e-4 ... 2.7e-4, and a border off by one (6e-4 ... 9e-4) is no longer ten bounds
    away.  With blocks, every case keeps the 2e-5 floor or stays within 1.3 times it."""
    c, h, w = shape
    f = pool_factor(h, w)
    g = torch.Generator().manual_seed(seed)
    x = torch.linspace(0, 1, w, dtype=torch.float64)[None, None, :]
    y = torch.linspace(0, 1, h, dtype=torch.float64)[None, :, None]
    base = 0.5 + 0.25 * torch.sin(6 * x + 2 * y) * torch.cos(3 * y)
    blocks = lambda t: t.repeat_interleave(f, 1).repeat_interleave(f, 2)[:, :h, :w]
    u = blocks(torch.rand((c, -(-h // f), -(-w // f)), generator=g, dtype=torch.float64))
    n = blocks(torch.randn((c, -(-h // f), -(-w // f)), generator=g, dtype=torch.float64))
    p = (base + 0.3 * (u - 0.5)).clamp(0, 1)
    t = (p + 0.3 * x ** 2 * (0.25 + 0.75 * y) * n).clamp(0, 1)
    return p.float(), t.float()


# ---- references --------------------------------------------------------------------------------------------------------
def diff_sums_ref(a, b):
    """((sum d, sum d^2), (bound1, bound2)) for d = a - b.  d and d*d are exact in double for float32 inputs of similar
    exponent, and the sums here are math.fsum's (correctly rounded), so only the kernel's order of n - 1 additions can
    differ: each rounds a partial sum no larger than sum|.| by at most 2**-53 of it."""
    d = (a.double() - b.double()).reshape(-1)
    n = d.numel()
    d2 = d * d
    s1, s2 = math.fsum(d.tolist()), math.fsum(d2.tolist())
    return (s1, s2), ((n + 2) * U53 * math.fsum(d.abs().tolist()), (n + 2) * U53 * s2)


def avg_pool_ref(x, f, dtype):
    """F.avg_pool2d(kernel_size=f) of (P,H,W) in `dtype`."""
    return F.avg_pool2d(x.to(dtype).unsqueeze(0), kernel_size=f)[0]


def ssim_map_ref(mx, my, exx, eyy, exy, border, c1, c2, dtype):
    """The expression above ssim_partial_kernel, per pixel of the valid interior of (P,H,W) maps, every step in `dtype`."""
    h, w = mx.shape[-2:]
    a, b, exx, eyy, exy = (t.to(dtype)[..., border:h - border, border:w - border] for t in (mx, my, exx, eyy, exy))
    sxx, syy, sxy = exx - a * a, eyy - b * b, exy - a * b
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    return (2 * a * b + c1) / (a * a + b * b + c1) * cs


def _taps(dtype):
    co = torch.arange(KS, dtype=dtype) - KS // 2
    g = torch.exp(-co ** 2 / (2 * SIGMA ** 2))
    return g / g.sum()


def ssim_ref(x, y, dtype, downsample=True, factor=None):
    """piq.ssim's published formula for (C,H,W) images, every step in `dtype` -> (scalar, (C,H-10,W-10) map).
    `factor` overrides the pooling factor (the planted mistakes)."""
    f = factor if factor is not None else (pool_factor(*x.shape[-2:]) if downsample else 1)
    x, y = x.to(dtype).unsqueeze(0), y.to(dtype).unsqueeze(0)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    c = x.shape[1]
    g = _taps(dtype)
    k = (g[:, None] * g[None, :]).expand(c, 1, KS, KS)
    conv = lambda t: F.conv2d(t, k, groups=c)
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    cs = (2 * sxy + K2 ** 2) / (sxx + syy + K2 ** 2)
    m = (2 * mx * my + K1 ** 2) / (mx * mx + my * my + K1 ** 2) * cs
    return float(m.mean()), m[0]


def moments_ref(x, y, dtype, factor=1):
    """The five Gaussian-filtered maps (mu_x, mu_y, E[xx], E[yy], E[xy]) at full (C,H,W) size, as ssim() hands them to
    vfi_ssim_sum: average-pooled by `factor`, half-sample-symmetric reflection at the edges, every step in `dtype`."""
    x, y = x.to(dtype).unsqueeze(0), y.to(dtype).unsqueeze(0)
    if factor > 1:
        x, y = F.avg_pool2d(x, factor), F.avg_pool2d(y, factor)
    c, r = x.shape[1], KS // 2
    g = _taps(dtype)
    k = (g[:, None] * g[None, :]).expand(c, 1, KS, KS)
    pad = lambda t: torch.from_numpy(np.pad(t.numpy(), ((0, 0), (0, 0), (r, r), (r, r)), mode="symmetric"))
    conv = lambda t: F.conv2d(pad(t), k, groups=c)[0]
    return conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)


# ---- planted mistakes (float64) ----------------------------------------------------------------------------------------
def planted_windows(maps, border, c1, c2):
    """{"true" | mistake: float64 SSIM values the walk would add} for the window mistakes that fit (P,H,W) `maps`."""
    full = ssim_map_ref(*maps, 0, c1, c2, torch.float64)
    p, h, w = full.shape
    b = border
    out = {"true": full[:, b:h - b, b:w - b]}
    if b >= 1:
        out["border-1"] = full[:, b - 1:h - b + 1, b - 1:w - b + 1]
        out["row+1"] = full[:, b + 1:h - b + 1, b:w - b]
        out["col+1"] = full[:, b:h - b, b + 1:w - b + 1]
    if h > 2 * (b + 1) and w > 2 * (b + 1):
        out["border+1"] = full[:, b + 1:h - b - 1, b + 1:w - b - 1]
    if h != w and b >= 1:                        # (border 0: either walk adds the whole plane)
        out["transposed"] = full.reshape(p, w, h)[:, b:w - b, b:h - b]
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------
# ssim(): ((C,H,W), downsample, seed).  128x32 is what --vimeo_testset leaves of a 448x256 image at --dim 512; 384 and 767
# pool by 2, 641 by 3, 896 by 4 (round half to even); 11x11 has one valid pixel.
SSIM_CASES = [((3, 128, 32), True, 1), ((1, 11, 11), True, 2), ((3, 11, 40), True, 3), ((2, 40, 11), True, 4),
              ((3, 13, 12), True, 5), ((1, 384, 385), True, 6), ((1, 767, 390), True, 7), ((1, 641, 643), True, 8),
              ((1, 896, 899), True, 9), ((1, 384, 385), False, 10)]
# vfi_ssim_sum alone: ((planes,H,W), border, seed)
SUM_CASES = [((1, 11, 11), 5, 11), ((3, 11, 40), 5, 12), ((2, 40, 11), 5, 13), ((3, 13, 12), 5, 14), ((3, 128, 32), 5, 15),
             ((2, 9, 14), 0, 16), ((1, 27, 64), 3, 17)]
C_PAIRS = [(K1 ** 2, K2 ** 2), (4e-4, 2.5e-3)]


def case_id(case):
    shape, other, _ = case
    return "x".join(map(str, shape)) + ("" if other is True else f"-{other}")


@functools.lru_cache(maxsize=None)
def ssim_case(i):
    """Everything the tests of SSIM_CASES[i] share: inputs, float64 scalar, bound, float32-vs-float64 gap, planted scalars."""
    shape, downsample, seed = SSIM_CASES[i]
    x, y = structured_pair(shape, seed)
    s64, m64 = ssim_ref(x, y, torch.float64, downsample)
    s32, m32 = ssim_ref(x, y, torch.float32, downsample)
    bound = max(2e-5, 4.0 * (m32.double() - m64).abs().mean().item())
    f = pool_factor(*shape[1:]) if downsample else 1
    maps = moments_ref(x, y, torch.float64, f)
    planted = {k: float(v.mean()) for k, v in planted_windows(maps, KS // 2, K1 ** 2, K2 ** 2).items()}
    for name, g in (("pool f-1", f - 1), ("pool f+1", f + 1)):
        if g >= 1 and min(shape[1:]) // g >= KS:
            planted[name] = ssim_ref(x, y, torch.float64, factor=g)[0]
    return dict(x=x, y=y, f=f, ref64=s64, ref32=s32, bound=bound, planted=planted)


@functools.lru_cache(maxsize=None)
def sum_case(i, j):
    """SUM_CASES[i] with C_PAIRS[j]: the five float32 maps, sum(map64), the bound, sum(map32), planted sums."""
    shape, border, seed = SUM_CASES[i]
    c1, c2 = C_PAIRS[j]
    maps = moments_ref(*structured_pair(shape, seed), torch.float32)
    m64 = ssim_map_ref(*maps, border, c1, c2, torch.float64)
    m32 = ssim_map_ref(*maps, border, c1, c2, torch.float32)
    planted = {k: float(v.sum()) for k, v in planted_windows(maps, border, c1, c2).items()}
    return dict(maps=maps, border=border, c1=c1, c2=c2, ref64=float(m64.sum()), ref32=float(m32.double().sum()),
                bound=m64.numel() * tol_of(m32, m64), n_valid=m64.numel(), planted=planted)
