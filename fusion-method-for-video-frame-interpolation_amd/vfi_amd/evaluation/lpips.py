"""LPIPS on the device -- `piq.LPIPS(reduction='none')` with its defaults, as reference src/evaluation/evaluate_image.py:22
calls it, and as a perceptual loss (reference src/fusion_net/trainer.py:13 imports it).  DESIGN.md section 24.

The arithmetic is restated from piq's published formula (piq is not here: PARITY UNPINNED, as for `ssim`):

1. `(x - mean) / std` per channel of the [0, 1] image, mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225);
2. `vgg16.features[:30]`: the thirteen convolutions of `vfi_amd.vgg16`'s table, a ReLU after each, `MaxPool2d(2)` after
   the 2nd, 4th, 7th and 10th; that module holds the table, the loader, the pack cache and the walks (`Trunk`);
3. taps: the ReLU outputs of convolutions 2, 4, 7, 10, 13 (relu1_2 ... relu5_3), before their pools; C = 64, 128, 256, 512, 512;
4. per tap, at every pixel `xh_c = x_c / (sqrt(sum_k x_k^2) + 1e-10)`, `yh` likewise,
   `d_l[n] = 1 / HW * sum_p sum_c w_{l,c} (xh_c - yh_c)^2`; the score of image n is `sum_l d_l[n]` in tap order.

`LPIPS(vgg_weights, lpips_weights, reduction='none')`; `forward(x, y)` takes the prediction and the target, (B, 3, H, W) in
[0, 1], and returns (B,) scores ('none'), their mean or their sum.  Nothing is downloaded:

* `vgg_weights`: a torchvision `vgg16` state dict, or the path of the file `torch.load` reads (`vgg16-397923af.pth`); the keys
  `features.{0,2,...,28}.{weight,bias}` are read, every other key is ignored.
* `lpips_weights`: the file piq downloads (a sequence of five tensors with 64, 128, 256, 512, 512 elements), or the `lpips`
  package's state dict (keys `lin{0..4}.model.1.weight`), or either object itself.

Both are frozen.  With fp32 HIP tensors prediction and target run as one batch of 2B through `Trunk.forward_hip`, and every
tap goes through `ops.lpips_head_forward` (one read of each map).  When grad mode is on and the prediction requires grad the
whole term is one autograd node (`_LPIPSFunction`): its backward walks from relu5_3 down with `Trunk.backward_hip`, and at
each tap `ops.lpips_head_backward` adds the head's gradient and applies the ReLU mask in the same pass.  The node keeps the five tapped 2B tensors and the prediction half of the eight other
ReLU outputs (views: their 2B tensors stay alive; 2160 bytes per pixel of a batch image in all).  The target gets no gradient.  That face needs H and W to be multiples of
16 (ValueError before any kernel otherwise); the no-grad face takes any H, W >= 16 (an odd plane is convolved unfused and
pooled with `MaxPool2d`'s floor).  CPU or float64 arguments take `_score_torch`, the same walk in plain torch.

At a pixel whose feature vector is zero piq's autograd returns NaN (sqrt is differentiated at 0); here the head's gradient
is 0 there, on every path.  Inside the network that is no choice: all channels of a ReLU output are zero at such a pixel,
and the mask stops the gradient anyway.
"""
import torch
import torch.nn as nn

from .. import ops, vgg16
from ..vgg16 import CHANNELS, CONV_INDICES  # noqa: F401  (the whole table: all thirteen convolutions)

N_CONVS = 13
TAPS = (1, 3, 6, 9, 12)                                              # convolutions whose ReLU output is tapped
TAP_CHANNELS = tuple(CHANNELS[i + 1] for i in TAPS)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EPS = 1e-10
HEAD_FORMAT = ("the LPIPS head weights: piq's file (a sequence of five tensors with 64, 128, 256, 512, 512 elements) or the "
               "lpips package's state dict (keys lin{0..4}.model.1.weight), as an object or a torch.save file")
VGG_WEIGHTS_ENV, LPIPS_WEIGHTS_ENV = vgg16.WEIGHTS_ENV, 'VFI_LPIPS_WEIGHTS'


def load_vgg16_features(weights):
    """-> {'<index>.weight' / '<index>.bias': tensor} of the thirteen convolutions from a vgg16 state dict or its file."""
    return vgg16.load_vgg16_features(weights, N_CONVS, "LPIPS", "the VGG16 weights")


def load_head_weights(weights):
    """-> five 1-d float32 tensors (64, 128, 256, 512, 512) from either format of the head weights, or their file."""
    weights = vgg16.load_file(weights, "LPIPS", "its head weights", HEAD_FORMAT, "--lpips_weights", LPIPS_WEIGHTS_ENV)
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
        self._trunk = vgg16.Trunk(N_CONVS, True, state)
        self.features = self._trunk.seq
        self.weights = nn.ParameterList([nn.Parameter(w, requires_grad=False) for w in heads])

    def packed(self):
        return self._trunk.packed()

    def packed_transposed(self):
        return self._trunk.packed_transposed()

    def _reduce(self, score):
        return score if self.reduction == 'none' else (score.mean() if self.reduction == 'mean' else score.sum())

    def _score_torch(self, x, y):
        """(B,) in x's dtype, in plain torch"""
        mean, std = (torch.tensor(v, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) for v in (MEAN, STD))
        b, score = x.shape[0], 0

        def tap(i, z):
            nonlocal score
            if i in TAPS:
                score = score + head_torch(z[:b], z[b:], self.weights[TAPS.index(i)])
        self._trunk.forward_torch(torch.cat([(x - mean) / std, (y - mean) / std], 0), tap)
        return score

    def _score_hip(self, x, y, keep=None):
        """(B,) fp32 on the device; `keep` (a list or None) receives the thirteen ReLU outputs of the 2B batch."""
        b, score = x.shape[0], None

        def tap(i, t):
            nonlocal score
            if i in TAPS:
                score = ops.lpips_head_forward(t[:b], t[b:], self.weights[TAPS.index(i)], score)
        self.packed()                                                   # a first forward packs before its first kernel
        self._trunk.forward_hip(ops.lpips_normalize(torch.cat([x, y], 0)), tap, keep)
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
        net.packed_transposed()                                         # a first backward packs before its first kernel
        up = upstream.contiguous()

        def head(i, above=None):                                        # a tapped ReLU output: route, head, mask
            return ops.lpips_head_backward(ts[i][:b], ts[i][b:], net.weights[TAPS.index(i)], up, above=above, out=above)
        g = net._trunk.backward_hip(head(TAPS[-1]), [t[:b] for t in ts], head)      # at relu5_3: the head alone
        ctx.keep = None
        return None, ops.lpips_normalize(g, adjoint=True), None
