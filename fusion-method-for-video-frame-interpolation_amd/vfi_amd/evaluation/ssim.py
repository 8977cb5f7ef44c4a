"""SSIM as a loss on the device -- counterpart of `piq.SSIMLoss` / `piq.ssim`, which the reference imports beside LPIPS at
src/fusion_net/trainer.py:13.  piq is absent here, so the arithmetic is restated from its published
formula, as in `evaluate_image.ssim`: PARITY UNPINNED.

    f = max(1, round(min(H, W) / 256));  x, y <- avg_pool2d(x, f), avg_pool2d(y, f) when downsample and f > 1
    g[i] ~ exp(-(i - r)^2 / (2 sigma^2)), r = kernel_size // 2, normalised; G separable, valid region only
    mu_x = G*x, mu_y = G*y, sxx = G*x^2 - mu_x^2, syy = G*y^2 - mu_y^2, sxy = G*xy - mu_x mu_y
    ssim = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * (2 sxy + c2) / (sxx + syy + c2),  c_i = (k_i data_range)^2
    ssim(x, y)[n] = mean over C (H - 2r) (W - 2r);   SSIMLoss = reduction(1 - ssim(x, y))

(piq divides both images by data_range and uses c_i = k_i^2; the two are the same function.)

On HIP float32 tensors the value is one launch pair of `vfi_ssim_loss_forward` and, with grad mode on, one autograd node
whose backward is `vfi_ssim_loss_backward` per argument that needs a gradient (SSIM is symmetric: the target's gradient is
the same entry with the arguments exchanged) and `vfi_avg_pool_backward` when f > 1.  The node keeps alive the (pooled)
x and y, nothing else.  CPU or float64 arguments take the same formula in plain torch.  An image smaller than the window
(after pooling) raises ValueError before any launch.

`evaluate_image.ssim` (the metric column, one (C, H, W) image, double accumulation) stays on its own kernels."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def pool_factor(h, w):
    """piq: max(1, round(min(H, W) / 256)), Python's round"""
    return max(1, round(min(h, w) / 256))


def _check(x, y, kernel_size, kernel_sigma, downsample):
    """-> pooling factor; raises ValueError on anything the kernels would refuse"""
    if x.dim() != 4 or tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"ssim: x {tuple(x.shape)} and y {tuple(y.shape)} must be equal (N, C, H, W)")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"ssim: empty batch or no channels: {tuple(x.shape)}")
    if kernel_size % 2 != 1 or not 3 <= kernel_size <= 11:
        raise ValueError(f"ssim: kernel_size must be odd, from 3 to 11, got {kernel_size}")
    if not kernel_sigma > 0:
        raise ValueError(f"ssim: kernel_sigma must be positive, got {kernel_sigma}")
    h, w = int(x.shape[2]), int(x.shape[3])
    f = pool_factor(h, w) if downsample else 1
    if h // f < kernel_size or w // f < kernel_size:
        pooled = f" (pooled by {f}: {h // f}x{w // f})" if f > 1 else ""
        raise ValueError(f"ssim: a {h}x{w} image{pooled} is smaller than the {kernel_size}-tap window")
    return f


def ssim_torch(x, y, kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, downsample=True, data_range=1.0):
    """(N,) in x's dtype: the formula above in plain torch, differentiable by autograd"""
    f = _check(x, y, kernel_size, kernel_sigma, downsample)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    c = x.shape[1]
    co = torch.arange(kernel_size, dtype=x.dtype, device=x.device) - kernel_size // 2
    g = torch.exp(-co ** 2 / (2 * kernel_sigma ** 2))
    g = g / g.sum()
    k = (g[:, None] * g[None, :]).expand(c, 1, kernel_size, kernel_size)
    conv = lambda t: F.conv2d(t, k, groups=c)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    m = (2 * mx * my + c1) / (mx * mx + my * my + c1) * ((2 * sxy + c2) / (sxx + syy + c2))
    return m.flatten(1).mean(1)


def _on_hip(x, y):
    return x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32


class _SSIMLossFunction(torch.autograd.Function):
    """(x, y, f, kernel_size, sigma, c1, c2) -> (N,) = 1 - mean SSIM; gradients to x and y"""

    @staticmethod
    def forward(ctx, x, y, f, kernel_size, sigma, c1, c2):
        ctx.size = tuple(x.shape[2:])
        if f > 1:
            x, y = ops.avg_pool(x.contiguous(), f), ops.avg_pool(y.contiguous(), f)
        ctx.conf = (f, kernel_size, sigma, c1, c2)
        ctx.save_for_backward(x, y)
        return ops.ssim_loss_forward(x, y, kernel_size, sigma, c1, c2)

    @staticmethod
    def backward(ctx, upstream):
        x, y = ctx.saved_tensors
        f, kernel_size, sigma, c1, c2 = ctx.conf
        up = upstream.contiguous()
        grads = []
        for need, (a, b) in zip(ctx.needs_input_grad[:2], ((x, y), (y, x))):
            g = None
            if need:
                g = ops.ssim_loss_backward(a, b, up, kernel_size, sigma, c1, c2)
                if f > 1:
                    g = ops.avg_pool_backward(g, ctx.size, f)
            grads.append(g)
        return grads[0], grads[1], None, None, None, None, None


def _dense(t):
    """a (N, C, H, W) tensor whose per-sample block is dense, as the entries take it (a batch slice stays a view)"""
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    ok = (sw == 1 or w == 1) and (sh == w or h == 1) and (sc == h * w or c == 1) and (n == 1 or sn >= c * h * w)
    return t if ok else t.contiguous()


def _loss_per_image(x, y, kernel_size, kernel_sigma, k1, k2, downsample, data_range):
    """(N,) = 1 - ssim per image, on whichever path the arguments select"""
    f = _check(x, y, kernel_size, kernel_sigma, downsample)
    if not _on_hip(x, y):
        return 1 - ssim_torch(x, y, kernel_size, kernel_sigma, k1, k2, downsample, data_range)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _SSIMLossFunction.apply(_dense(x), _dense(y), f, int(kernel_size), float(kernel_sigma), c1, c2)
    x, y = x.detach(), y.detach()
    if f > 1:
        x, y = ops.avg_pool(x.contiguous(), f), ops.avg_pool(y.contiguous(), f)
    return ops.ssim_loss_forward(_dense(x), _dense(y), int(kernel_size), float(kernel_sigma), c1, c2)


def ssim(x, y, kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, downsample=True, data_range=1.0):
    """(N,) SSIM of each image of (N, C, H, W) batches: 1 - SSIMLoss(reduction='none')"""
    return 1 - _loss_per_image(x, y, kernel_size, kernel_sigma, k1, k2, downsample, data_range)


class SSIMLoss(nn.Module):
    """piq.SSIMLoss: reduction(1 - ssim(x, y)); reduction 'none' | 'mean' | 'sum'"""

    def __init__(self, kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, downsample=True, reduction='mean', data_range=1.0):
        super(SSIMLoss, self).__init__()
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"reduction {reduction!r}: 'none', 'mean' or 'sum'")
        if kernel_size % 2 != 1 or not 3 <= kernel_size <= 11:
            raise ValueError(f"SSIMLoss: kernel_size must be odd, from 3 to 11, got {kernel_size}")
        self.kernel_size, self.kernel_sigma, self.k1, self.k2 = kernel_size, kernel_sigma, k1, k2
        self.downsample, self.reduction, self.data_range = downsample, reduction, data_range

    def forward(self, x, y):
        v = _loss_per_image(x, y, self.kernel_size, self.kernel_sigma, self.k1, self.k2, self.downsample, self.data_range)
        return v if self.reduction == 'none' else (v.mean() if self.reduction == 'mean' else v.sum())
