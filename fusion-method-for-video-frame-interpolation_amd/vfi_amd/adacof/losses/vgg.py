"""Perceptual loss of the AdaCoF trainer -- mirror of reference src/adacof/losses/vgg.py:7-22:
`F.mse_loss(conv4_3(output), conv4_3(gt.detach()))` with the first 22 layers of torchvision's `vgg16.features`, frozen,
on the raw [0, 1] images (the reference applies no ImageNet normalisation).

The layers (`TABLE`): ten 3x3 zero-padded convolutions 3->64->64 | 128, 128 | 256, 256, 256 | 512, 512, 512 at the indices
0, 2, 5, 7, 10, 12, 14, 17, 19, 21 of `features`; a ReLU after each but the last (the slice ends on conv4_3, before its
ReLU); `MaxPool2d(2)` after the 2nd, 4th and 7th.  They are held as the same `nn.Sequential` the reference slices out, under
the same name, so `state_dict()` has the reference's keys (`vgg16_conv_4_3.<index>.{weight,bias}`).

With fp32 HIP tensors the whole term is one autograd node (`_VGGFunction`): output and target run as one batch of 2B through
`ops.conv2d(act="relu")` / `ops.conv2d_pool2(is_max=True)`, the loss is `ops.mse_forward` on the two halves of the conv4_3
tensor, and the backward is `ops.mse_backward` followed by `ops.conv2d_backward_data`, `ops.relu_mask_` and
`ops.pool2_max_backward` down the ten layers on the B images of the output half.  Only `output` gets a gradient.  Of each
ReLU output the node keeps the output half (a view: the 2B tensor's memory stays until the backward has run).  Without a
tensor that requires grad, or with grad mode off, the same forward runs without a node.  CPU or float64 arguments take
`_features_torch`, the same table in plain torch.

Differences from the reference:

* Nothing is downloaded.  `VGG(weights=...)` takes a torchvision `vgg16` state dict -- the dict itself or the path of a file
  `torch.load` reads (torchvision's `vgg16-397923af.pth`) -- and reads its keys `features.{0,2,...,21}.{weight,bias}`; every
  other key is ignored.  No weights, or a missing file, raise an error that says so.
* H and W must be multiples of 8 (the fused pool and its adjoint take even planes; the reference trains on 256x256
  patches): anything else raises ValueError before a kernel runs, on every path.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)            # of vgg16.features
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512)
POOL_AFTER = (1, 3, 6)                                         # convolutions (0-based) followed by MaxPool2d(2)
LAST = len(CONV_INDICES) - 1
FORMAT = ("a torchvision vgg16 state dict (the file vgg16-397923af.pth of torchvision.models.vgg16, or any dict / "
          "torch.save file with the keys features.{0,2,5,7,10,12,14,17,19,21}.{weight,bias})")


def _sequential():
    """vgg16.features[:22]"""
    layers = []
    for i in range(len(CONV_INDICES)):
        layers.append(nn.Conv2d(CHANNELS[i], CHANNELS[i + 1], kernel_size=3, padding=1))
        if i != LAST:
            layers.append(nn.ReLU(inplace=True))
        if i in POOL_AFTER:
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    assert tuple(k for k, m in enumerate(layers) if isinstance(m, nn.Conv2d)) == CONV_INDICES and len(layers) == 22
    return nn.Sequential(*layers)


def load_vgg16_features(weights):
    """-> {'<index>.weight' / '<index>.bias': tensor} of the ten convolutions from a vgg16 state dict or its file."""
    if weights is None:
        raise ValueError(f"the VGG loss needs weights: pass --vgg_weights (or set VFI_VGG16_WEIGHTS) to {FORMAT}")
    if not isinstance(weights, dict):
        path = os.fspath(weights)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: not found; the VGG loss needs {FORMAT}")
        weights = torch.load(path, map_location='cpu')
    out = {}
    for i, idx in enumerate(CONV_INDICES):
        for kind, shape in (('weight', (CHANNELS[i + 1], CHANNELS[i], 3, 3)), ('bias', (CHANNELS[i + 1],))):
            key = f'features.{idx}.{kind}'
            if key not in weights:
                raise KeyError(f"{key} is missing: the VGG loss needs {FORMAT}")
            if tuple(weights[key].shape) != shape:
                raise ValueError(f"{key} has shape {tuple(weights[key].shape)}, not {shape}: the VGG loss needs {FORMAT}")
            out[f'{idx}.{kind}'] = weights[key]
    return out


def _check_size(output, gt):
    if output.dim() != 4 or output.shape[1] != 3 or tuple(output.shape) != tuple(gt.shape):
        raise ValueError(f"VGG: output {tuple(output.shape)} and gt {tuple(gt.shape)} must be equal (B, 3, H, W)")
    h, w = int(output.shape[2]), int(output.shape[3])
    if h % 8 or w % 8 or h < 8 or w < 8:
        raise ValueError(f"VGG: H and W must be multiples of 8, got {h}x{w}")


class VGG(nn.Module):
    def __init__(self, weights=None):
        super(VGG, self).__init__()
        state = load_vgg16_features(weights)
        self.vgg16_conv_4_3 = _sequential()
        self.vgg16_conv_4_3.load_state_dict(state)
        for param in self.vgg16_conv_4_3.parameters():
            param.requires_grad = False
        self._packs = None

    def convs(self):
        return [self.vgg16_conv_4_3[i] for i in CONV_INDICES]

    def packed(self):
        """(forward packs, transposed packs or None) of the ten frozen convolutions on their device, made once; made again
        when the module has moved or a weight was written."""
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

    def _features_torch(self, x):
        """conv4_3 of x in x's dtype, in plain torch"""
        for i, c in enumerate(self.convs()):
            x = F.conv2d(x, c.weight.to(x.dtype), c.bias.to(x.dtype), padding=1)
            if i != LAST:
                x = F.relu(x)
            if i in POOL_AFTER:
                x = F.max_pool2d(x, 2, 2)
        return x

    def _features_hip(self, x, relu_outputs=None):
        """conv4_3 of x (N, 3, H, W) fp32 on the device; relu_outputs (a list or None) receives the nine ReLU outputs."""
        packs = self.packed()[1]
        for i, pc in enumerate(packs):
            if i == LAST:
                x = ops.conv2d(x, pc, "zeros", None)
            elif i in POOL_AFTER:
                y, x = ops.conv2d_pool2(x, pc, True, "zeros", "relu")
            else:
                y = x = ops.conv2d(x, pc, "zeros", "relu")
            if relu_outputs is not None and i != LAST:
                relu_outputs.append(y)
        return x

    def forward(self, output, gt):
        _check_size(output, gt)
        gt = gt.detach()
        if not (output.is_cuda and gt.is_cuda and output.dtype == torch.float32 and gt.dtype == torch.float32):
            vgg_output = self._features_torch(output)
            with torch.no_grad():
                vgg_gt = self._features_torch(gt)
            return F.mse_loss(vgg_output, vgg_gt)
        if torch.is_grad_enabled() and output.requires_grad:
            return _VGGFunction.apply(self, output, gt)
        b = output.shape[0]
        feat = self._features_hip(torch.cat([output.detach(), gt], 0))
        return ops.mse_forward(feat[:b], feat[b:])


class _VGGFunction(torch.autograd.Function):
    """(net, output, gt) -> the loss; gradient to `output` alone."""

    @staticmethod
    def forward(ctx, net, output, gt):
        b = output.shape[0]
        relu_outputs = []
        feat = net._features_hip(torch.cat([output.detach(), gt], 0), relu_outputs)
        ctx.net, ctx.keep = net, ([y[:b] for y in relu_outputs], feat)
        return ops.mse_forward(feat[:b], feat[b:])

    @staticmethod
    def backward(ctx, upstream):
        net, (ys, feat) = ctx.net, ctx.keep
        b = ys[0].shape[0]
        pT = net.packed_transposed()
        g, _ = ops.mse_backward(feat[:b], feat[b:], upstream.contiguous(), need_a=True, need_b=False)
        for i in range(LAST, 0, -1):
            gx = ops.conv2d_backward_data(g, pT[i], "zeros")            # gradient of layer i's input
            if i - 1 in POOL_AFTER:                                     # ... which is the max-pool of relu output i - 1
                g = ops.pool2_max_backward(ys[i - 1], gx)
            else:
                g = ops.relu_mask_(gx, ys[i - 1])
        ctx.keep = None
        return None, ops.conv2d_backward_data(g, pT[0], "zeros"), None
