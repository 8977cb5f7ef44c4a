"""LPIPS on the device -- `piq.LPIPS(reduction='none')` with its defaults, as reference src/evaluation/evaluate_image.py:22
calls it, and as a perceptual loss (reference src/fusion_net/trainer.py:13 imports it).  DESIGN.md section 24.

The arithmetic is restated from piq's published formula (piq is not here: PARITY UNPINNED, as for `ssim`):

1. `(x - mean) / std` per channel of the [0, 1] image, mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225);
2. `vgg16.features[:30]` (`CONV_INDICES`, `CHANNELS`, `POOL_AFTER` below): thirteen 3x3 zero-padded convolutions, a ReLU
   after each, `MaxPool2d(2)` after the 2nd, 4th, 7th and 10th;
3. taps: the ReLU outputs of convolutions 2, 4, 7, 10, 13 (relu1_2 ... relu5_3), before their pools; C = 64, 128, 256, 512, 512;
4. per tap, at every pixel `xh_c = x_c / (sqrt(sum_k x_k^2) + 1e-10)`, `yh` likewise,
   `d_l[n] = 1 / HW * sum_p sum_c w_{l,c} (xh_c - yh_c)^2`; the score of image n is `sum_l d_l[n]` in tap order.

`LPIPS(vgg_weights, lpips_weights, reduction='none')`; `forward(x, y)` takes the prediction and the target, (B, 3, H, W) in
[0, 1], and returns (B,) scores ('none'), their mean or their sum.  Nothing is downloaded:

* `vgg_weights`: a torchvision `vgg16` state dict, or the path of the file `torch.load` reads (`vgg16-397923af.pth`); the keys
  `features.{0,2,...,28}.{weight,bias}` are read, every other key is ignored.
* `lpips_weights`: the file piq downloads (a sequence of five tensors with 64, 128, 256, 512, 512 elements), or the `lpips`
  package's state dict (keys `lin{0..4}.model.1.weight`), or either object itself.

Both are frozen.  With fp32 HIP tensors prediction and target run as one batch of 2B through `ops.conv2d(act="relu")` /
`ops.conv2d_pool2`, and every tap goes through `ops.lpips_head_forward` (one read of each map).  When grad mode is on and the
prediction requires grad the whole term is one autograd node (`_LPIPSFunction`): its backward walks from relu5_3 down with
`ops.conv2d_backward_data` and `ops.pool2_max_backward`, and at each tap `ops.lpips_head_backward` adds the head's gradient and
applies the ReLU mask in the same pass.  The node keeps the five tapped 2B tensors and the prediction half of the eight other
ReLU outputs (views: their 2B tensors stay alive; 2160 bytes per pixel of a batch image in all).  The target gets no gradient.  That face needs H and W to be multiples of
16 (ValueError before any kernel otherwise); the no-grad face takes any H, W >= 16 (an odd plane is convolved unfused and
pooled with `MaxPool2d`'s floor).  CPU or float64 arguments take `_score_torch`, the same table in plain torch.

At a pixel whose feature vector is zero piq's autograd returns NaN (sqrt is differentiated at 0); here the head's gradient
is 0 there, on every path.  Inside the network that is no choice: all channels of a ReLU output are zero at such a pixel,
and the mask stops the gradient anyway.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # of vgg16.features
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_AFTER = (1, 3, 6, 9)                                            # convolutions (0-based) followed by MaxPool2d(2)
TAPS = (1, 3, 6, 9, 12)                                              # convolutions whose ReLU output is tapped
TAP_CHANNELS = tuple(CHANNELS[i + 1] for i in TAPS)
LAST = len(CONV_INDICES) - 1
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EPS = 1e-10
VGG_FORMAT = ("a torchvision vgg16 state dict (the file vgg16-397923af.pth of torchvision.models.vgg16, or any dict / "
              "torch.save file with the keys features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias})")
HEAD_FORMAT = ("the LPIPS head weights: piq's file (a sequence of five tensors with 64, 128, 256, 512, 512 elements) or the "
               "lpips package's state dict (keys lin{0..4}.model.1.weight), as an object or a torch.save file")
VGG_WEIGHTS_ENV, LPIPS_WEIGHTS_ENV = 'VFI_VGG16_WEIGHTS', 'VFI_LPIPS_WEIGHTS'


def _sequential():
    """vgg16.features[:30]"""
    layers = []
    for i in range(len(CONV_INDICES)):
        layers.append(nn.Conv2d(CHANNELS[i], CHANNELS[i + 1], kernel_size=3, padding=1))
        layers.append(nn.ReLU(inplace=True))
        if i in POOL_AFTER:
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    assert tuple(k for k, m in enumerate(layers) if isinstance(m, nn.Conv2d)) == CONV_INDICES and len(layers) == 30
    return nn.Sequential(*layers)


def _load_file(weights, what, fmt, flag, env):
    if weights is None:
        raise ValueError(f"LPIPS needs {what}: pass {flag} (or set {env}) to {fmt}")
    if isinstance(weights, (str, os.PathLike)):
        path = os.fspath(weights)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: not found; LPIPS needs {fmt}")
        weights = torch.load(path, map_location='cpu')
    return weights


def load_vgg16_features(weights):
    """-> {'<index>.weight' / '<index>.bias': tensor} of the thirteen convolutions from a vgg16 state dict or its file."""
    weights = _load_file(weights, "the VGG16 weights", VGG_FORMAT, "--vgg_weights", VGG_WEIGHTS_ENV)
    if not isinstance(weights, dict):
        raise TypeError(f"{type(weights).__name__}: LPIPS needs {VGG_FORMAT}")
    out = {}
    for i, idx in enumerate(CONV_INDICES):
        for kind, shape in (('weight', (CHANNELS[i + 1], CHANNELS[i], 3, 3)), ('bias', (CHANNELS[i + 1],))):
            key = f'features.{idx}.{kind}'
            if key not in weights:
                raise KeyError(f"{key} is missing: LPIPS needs {VGG_FORMAT}")
            if tuple(weights[key].shape) != shape:
                raise ValueError(f"{key} has shape {tuple(weights[key].shape)}, not {shape}: LPIPS needs {VGG_FORMAT}")
            out[f'{idx}.{kind}'] = weights[key]
    return out


def load_head_weights(weights):
    """-> five 1-d float32 tensors (64, 128, 256, 512, 512) from either format of the head weights, or their file."""
    weights = _load_file(weights, "its head weights", HEAD_FORMAT, "--lpips_weights", LPIPS_WEIGHTS_ENV)
    if isinstance(weights, dict):
        seq = []
        for l in range(len(TAPS)):
            key = f'lin{l}.model.1.weight'
            if key not in weights:
                raise KeyError(f"{key} is missing: LPIPS needs {HEAD_FORMAT}")
            seq.append(weights[key])
    elif isinstance(weights, (list, tuple)):
        seq = list(weights)
    else:
        raise TypeError(f"{type(weights).__name__}: LPIPS needs {HEAD_FORMAT}")
    if len(seq) != len(TAPS):
        raise ValueError(f"{len(seq)} tensors, not {len(TAPS)}: LPIPS needs {HEAD_FORMAT}")
    out = []
    for l, (t, c) in enumerate(zip(seq, TAP_CHANNELS)):
        if not isinstance(t, torch.Tensor) or t.numel() != c:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"head weight {l} is {got}, not {c} elements: LPIPS needs {HEAD_FORMAT}")
        out.append(t.detach().reshape(c).to(torch.float32).clone())
    return out


def _unit(x):
    """x / (|x| + eps) over the channels, and the constant 0 at a pixel where x is zero"""
    n2 = (x * x).sum(1, keepdim=True)
    live = n2 > 0
    norm = torch.sqrt(torch.where(live, n2, torch.ones_like(n2)))
    return torch.where(live, x / (norm + EPS), torch.zeros_like(x))


def head_torch(x, y, w):
    """(N,) = mean_p sum_c w_c (xh_c - yh_c)^2 in plain torch; the gradient is 0 at pixels where x is zero"""
    d = (_unit(x) - _unit(y)) ** 2 * w.to(x.dtype).view(1, -1, *([1] * (x.dim() - 2)))
    return d.flatten(1).sum(1) / (x[0, 0].numel())


class LPIPS(nn.Module):
    def __init__(self, vgg_weights=None, lpips_weights=None, reduction='none'):
        super(LPIPS, self).__init__()
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"reduction {reduction!r}: 'none', 'mean' or 'sum'")
        self.reduction = reduction
        state = load_vgg16_features(vgg_weights)
        heads = load_head_weights(lpips_weights)
        self.features = _sequential()
        self.features.load_state_dict(state)
        self.weights = nn.ParameterList([nn.Parameter(w, requires_grad=False) for w in heads])
        for param in self.features.parameters():
            param.requires_grad = False
        self._packs = None

    def convs(self):
        return [self.features[i] for i in CONV_INDICES]

    def packed(self):
        """[key, forward packs, transposed packs or None] of the thirteen frozen convolutions on their device, made once;
        made again when the module has moved or a weight was written."""
        convs = self.convs()
        key = (convs[0].weight.device,) + tuple(t._version for c in convs for t in (c.weight, c.bias))
        if self._packs is None or self._packs[0] != key:
            self._packs = [key, [ops.PackedConv(c.weight, c.bias) for c in convs], None]
        return self._packs

    def packed_transposed(self):
        p = self.packed()
        if p[2] is None:
            p[2] = [ops.packed_transposed(c.weight) for c in self.convs()]
        return p[2]

    def _reduce(self, score):
        return score if self.reduction == 'none' else (score.mean() if self.reduction == 'mean' else score.sum())

    def _score_torch(self, x, y):
        """(B,) in x's dtype, in plain torch"""
        mean, std = (torch.tensor(v, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) for v in (MEAN, STD))
        z = torch.cat([(x - mean) / std, (y - mean) / std], 0)
        b, score, tap = x.shape[0], 0, 0
        for i, c in enumerate(self.convs()):
            z = F.relu(F.conv2d(z, c.weight.to(z.dtype), c.bias.to(z.dtype), padding=1))
            if i in TAPS:
                score = score + head_torch(z[:b], z[b:], self.weights[tap])
                tap += 1
            if i in POOL_AFTER:
                z = F.max_pool2d(z, 2, 2)
        return score

    def _score_hip(self, x, y, keep=None):
        """(B,) fp32 on the device; `keep` (a list or None) receives the thirteen ReLU outputs of the 2B batch."""
        packs = self.packed()[1]
        b = x.shape[0]
        z = ops.lpips_normalize(torch.cat([x, y], 0))
        score, tap = None, 0
        for i, pc in enumerate(packs):
            h, w = z.shape[2:]
            if i in POOL_AFTER and h % 2 == 0 and w % 2 == 0:
                t, z = ops.conv2d_pool2(z, pc, True, "zeros", "relu")
            else:
                t = ops.conv2d(z, pc, "zeros", "relu")
                z = ops.pool2(t, True) if i in POOL_AFTER else t
            if i in TAPS:
                score = ops.lpips_head_forward(t[:b], t[b:], self.weights[tap], score)
                tap += 1
            if keep is not None:
                keep.append(t)
        return score

    def forward(self, x, y):
        if x.dim() != 4 or x.shape[1] != 3 or tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"LPIPS: prediction {tuple(x.shape)} and target {tuple(y.shape)} must be equal (B, 3, H, W)")
        h, w = int(x.shape[2]), int(x.shape[3])
        if h < 16 or w < 16:
            raise ValueError(f"LPIPS: H and W must be at least 16, got {h}x{w}")
        y = y.detach()
        if not (x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32):
            return self._reduce(self._score_torch(x, y))
        if torch.is_grad_enabled() and x.requires_grad:
            if h % 16 or w % 16:
                raise ValueError(f"LPIPS as a loss: H and W must be multiples of 16, got {h}x{w}")
            return self._reduce(_LPIPSFunction.apply(self, x, y))
        return self._reduce(self._score_hip(x.detach(), y))


class _LPIPSFunction(torch.autograd.Function):
    """(net, x, y) -> (B,) scores; gradient to `x` alone."""

    @staticmethod
    def forward(ctx, net, x, y):
        b = x.shape[0]
        ts = []
        score = net._score_hip(x.detach(), y, ts)
        ctx.net, ctx.keep = net, [t if i in TAPS else t[:b] for i, t in enumerate(ts)]
        return score

    @staticmethod
    def backward(ctx, upstream):
        net, ts = ctx.net, ctx.keep
        b = upstream.shape[0]
        pT = net.packed_transposed()
        up = upstream.contiguous()
        tap = len(TAPS) - 1
        g = ops.lpips_head_backward(ts[LAST][:b], ts[LAST][b:], net.weights[tap], up)        # at relu5_3: the head alone
        for i in range(LAST, 0, -1):
            gx = ops.conv2d_backward_data(g, pT[i], "zeros")            # gradient of layer i's input
            j = i - 1
            if j in TAPS:                                               # a tapped ReLU output (each feeds a pool): route, head, mask
                tap -= 1
                above = ops.pool2_max_backward(ts[j][:b], gx)
                g = ops.lpips_head_backward(ts[j][:b], ts[j][b:], net.weights[tap], up, above=above, out=above)
            else:
                g = ops.relu_mask_(gx, ts[j])
        ctx.keep = None
        return None, ops.lpips_normalize(ops.conv2d_backward_data(g, pT[0], "zeros"), adjoint=True), None
