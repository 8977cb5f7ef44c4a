"""What the SSIM-loss tests share (tests/test_ssim_loss_host.py, tests/test_ssim_loss_gpu.py): the
expression of scoring_ref.ssim_ref extended to a batch and to any window, its gradients by torch autograd in float64 and
float32, the closed form of the gradient the backward kernel evaluates, and the cases.  CPU only; scoring_ref and glue_ref
are imported as they are.

Bounds come from the reference alone.  A value (per image) is held to scoring_ref's SSIM bound,
max(2e-5, 4 * mean|map32 - map64|) over that image's map; a gradient to glue_ref.tol_of(g32, g64) over the whole gradient
tensor, g32 the float32 autograd gradient of the same expression."""
import functools

import torch
import torch.nn.functional as F

from glue_ref import tol_of
from scoring_ref import K1, K2, pool_factor, structured_pair

TILE = 32          # T: kTile of csrc/vfi_ssim.hip, the edge of a tile of the SSIM map (forward) and of grad_x (backward)

# ((N, C, H, W), kernel_size, sigma) for the two entries: one valid pixel; one valid row / column; odd and non-square shapes, more than one tile;
# valid extents T and T + 1 both ways ((42, 43): 32 x 33 valid, (43, 42): 33 x 32); a 7-tap window
ENTRY_CASES = [((1, 1, 11, 11), 11, 1.5), ((2, 3, 11, 40), 11, 1.5), ((1, 2, 40, 11), 11, 1.5), ((1, 3, 13, 12), 11, 1.5),
               ((3, 1, 27, 64), 11, 1.5), ((1, 3, 37, 70), 11, 1.5), ((2, 3, 64, 64), 11, 1.5), ((1, 3, 128, 32), 11, 1.5),
               ((1, 2, TILE + 10, TILE + 11), 11, 1.5), ((2, 1, TILE + 11, TILE + 10), 11, 1.5), ((1, 3, 27, 64), 7, 1.0)]
# 2 x 2 tiles per plane, 1028 in all: more than the 1024 blocks of the forward's grid, so blocks 0 ... 3 walk two tiles
WALK_CASE = ((1, 257, TILE + 11, TILE + 11), 11, 1.5)
# through the module with piq's pooling: f = 2 with the last column dropped, f = 3
POOLED_CASES = [((1, 1, 384, 385), 11, 1.5), ((1, 1, 641, 643), 11, 1.5)]


def case_id(case):
    shape, ks, _ = case
    return "x".join(map(str, shape)) + ("" if ks == 11 else f"-k{ks}")


def taps(ks, sigma, dtype):
    co = torch.arange(ks, dtype=dtype) - ks // 2
    g = torch.exp(-co ** 2 / (2 * sigma ** 2))
    return g / g.sum()


def ssim_map(x, y, ks=11, sigma=1.5, factor=1):
    """ssim_ref's expression on (N, C, H, W) batches in their dtype -> the (N, C, H - 2r, W - 2r) map; pooled by `factor` first"""
    if factor > 1:
        x, y = F.avg_pool2d(x, factor), F.avg_pool2d(y, factor)
    c = x.shape[1]
    g = taps(ks, sigma, x.dtype)
    k = (g[:, None] * g[None, :]).expand(c, 1, ks, ks)
    conv = lambda t: F.conv2d(t, k, groups=c)
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    cs = (2 * sxy + K2 ** 2) / (sxx + syy + K2 ** 2)
    return (2 * mx * my + K1 ** 2) / (mx * mx + my * my + K1 ** 2) * cs


def ssim_batch(x, y, ks=11, sigma=1.5, factor=1):
    """-> (N,) mean SSIM per image"""
    return ssim_map(x, y, ks, sigma, factor).flatten(1).mean(1)


def upstream(n):
    """distinct per image"""
    return torch.linspace(0.5, 1.5, n) if n > 1 else torch.tensor([0.7])


def evaluate(x, y, up, dtype, ks=11, sigma=1.5, factor=1):
    """-> (loss (N,), map, d/dx, d/dy of sum_n up[n] * loss[n]) in `dtype`, loss = 1 - mean SSIM"""
    xx, yy = x.detach().to(dtype).clone().requires_grad_(True), y.detach().to(dtype).clone().requires_grad_(True)
    m = ssim_map(xx, yy, ks, sigma, factor)
    loss = 1 - m.flatten(1).mean(1)
    (loss * up.to(dtype)).sum().backward()
    return loss.detach(), m.detach(), xx.grad, yy.grad


def closed_form_grad_x(x, y, up, ks=11, sigma=1.5):
    """d/dx of sum_n up[n] (1 - mean ssim) by the closed form of include/vfi_hip.h, in x's dtype, without autograd"""
    c = x.shape[1]
    g = taps(ks, sigma, x.dtype)
    k = (g[:, None] * g[None, :]).expand(c, 1, ks, ks)
    conv = lambda t: F.conv2d(t, k, groups=c)
    c1, c2 = K1 ** 2, K2 ** 2
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    n1, d1, d2 = 2 * mx * my + c1, mx * mx + my * my + c1, sxx + syy + c2
    l, cs = n1 / d1, (2 * sxy + c2) / d2
    b = -l * cs / d2
    cm = 2 * l / d2
    a = cs * (2 * my / d1 - 2 * mx * n1 / d1 ** 2) - 2 * mx * b - my * cm
    full = lambda t: F.conv_transpose2d(t, k, groups=c)          # the full correlation of the zero-extended map
    count = mx[0].numel()
    return -(up.to(x.dtype) / count).view(-1, 1, 1, 1) * (full(a) + 2 * x * full(b) + y * full(cm))


def batch_inputs(shape, seed0):
    """x, y (N, C, H, W) float32: scoring_ref.structured_pair per image, seeds seed0, seed0 + 1, ..."""
    n = shape[0]
    pairs = [structured_pair(tuple(shape[1:]), seed0 + i) for i in range(n)]
    return torch.stack([p for p, _ in pairs]), torch.stack([t for _, t in pairs])


@functools.lru_cache(maxsize=None)
def case(shape, ks, sigma, pooled=False):
    """Everything the tests of one case share, computed once: inputs, upstream, float64 loss and gradients, the float32
    autograd gradients, the per-image value bound and the gradient tolerances."""
    x, y = batch_inputs(shape, 100 + 7 * sum(shape) + ks)
    f = pool_factor(*shape[2:]) if pooled else 1
    up = upstream(shape[0])
    v64, m64, gx64, gy64 = evaluate(x, y, up, torch.float64, ks, sigma, f)
    v32, m32, gx32, gy32 = evaluate(x, y, up, torch.float32, ks, sigma, f)
    bound = [max(2e-5, 4.0 * (m32[i].double() - m64[i]).abs().mean().item()) for i in range(shape[0])]
    return dict(x=x, y=y, up=up, f=f, ks=ks, sigma=sigma, v64=v64, v32=v32, gx64=gx64, gx32=gx32, gy64=gy64, gy32=gy32,
                bound=bound, tol_gx=tol_of(gx32, gx64), tol_gy=tol_of(gy32, gy64))


@functools.lru_cache(maxsize=None)
def reduced_grads(shape, ks, sigma, reduction):
    """(gx32, gx64, gy32, gy64) of the 'mean' or 'sum' of the per-image losses of case(shape, ks, sigma)"""
    c = case(shape, ks, sigma)
    n = shape[0]
    wts = torch.full((n,), 1.0 / n if reduction == 'mean' else 1.0)
    (gx32, gy32), (gx64, gy64) = (evaluate(c["x"], c["y"], wts, d, ks, sigma)[2:] for d in (torch.float32, torch.float64))
    return gx32, gx64, gy32, gy64
