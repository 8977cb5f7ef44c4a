"""The frozen torchvision VGG16 trunk that `adacof.losses.vgg.VGG` (ten convolutions, `vgg16.features[:22]`) and
`evaluation.lpips.LPIPS` (thirteen, `vgg16.features[:30]`) walk: the layer tables, the loader of torchvision state dicts,
the pack cache, and the plain-torch, HIP forward and HIP backward walks.

The layers: thirteen 3x3 zero-padded convolutions 3->64->64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512 at
`CONV_INDICES` of `features`, a ReLU after each, `MaxPool2d(2)` after the 2nd, 4th, 7th and 10th.  A trunk is the first
`n_convs` of them (10 or 13); `relu_last=False` ends it on the last convolution, before its ReLU.

`Trunk` is plain Python, no `nn.Module`: its owner registers `Trunk.seq` under the name the reference gives it, so the
owner's `state_dict()` keeps the reference's keys.  Each owner has its own weights and packs.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # of vgg16.features
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LAYERS = {10: 22, 13: 30}                                            # n_convs -> length of the slice of vgg16.features
WEIGHTS_ENV = 'VFI_VGG16_WEIGHTS'


def pool_after(n_convs):
    """the convolutions (0-based) of the slice that a MaxPool2d(2) follows; the slice ends before the pool of its last one"""
    return tuple(i for i in (1, 3, 6, 9) if i < n_convs - 1)


def weights_format(n_convs):
    return ("a torchvision vgg16 state dict (the file vgg16-397923af.pth of torchvision.models.vgg16, or any dict / "
            "torch.save file with the keys features.{%s}.{weight,bias})" % ",".join(map(str, CONV_INDICES[:n_convs])))


def sequential(n_convs, relu_last):
    """vgg16.features[:22] (10, False) or vgg16.features[:30] (13, True)"""
    layers = []
    for i in range(n_convs):
        layers.append(nn.Conv2d(CHANNELS[i], CHANNELS[i + 1], kernel_size=3, padding=1))
        if relu_last or i != n_convs - 1:
            layers.append(nn.ReLU(inplace=True))
        if i in pool_after(n_convs):
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    assert tuple(k for k, m in enumerate(layers) if isinstance(m, nn.Conv2d)) == CONV_INDICES[:n_convs]
    assert len(layers) == LAYERS[n_convs]
    return nn.Sequential(*layers)


def load_file(weights, who, what, fmt, flag, env):
    """`weights`, or what `torch.load` reads from it when it is a path; `who` needs `what` in the format `fmt`."""
    if weights is None:
        raise ValueError(f"{who} needs {what}: pass {flag} (or set {env}) to {fmt}")
    if isinstance(weights, (str, os.PathLike)):
        path = os.fspath(weights)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: not found; {who} needs {fmt}")
        weights = torch.load(path, map_location='cpu')
    return weights


def load_vgg16_features(weights, n_convs, who, what):
    """-> {'<index>.weight' / '<index>.bias': tensor} of the first n_convs convolutions from a vgg16 state dict or its file;
    `who` ("the VGG loss", "LPIPS") asks for `what`, in its error messages."""
    fmt = weights_format(n_convs)
    weights = load_file(weights, who, what, fmt, "--vgg_weights", WEIGHTS_ENV)
    if not isinstance(weights, dict):
        raise TypeError(f"{type(weights).__name__}: {who} needs {fmt}")
    out = {}
    for i, idx in enumerate(CONV_INDICES[:n_convs]):
        for kind, shape in (('weight', (CHANNELS[i + 1], CHANNELS[i], 3, 3)), ('bias', (CHANNELS[i + 1],))):
            key = f'features.{idx}.{kind}'
            if key not in weights:
                raise KeyError(f"{key} is missing: {who} needs {fmt}")
            if tuple(weights[key].shape) != shape:
                raise ValueError(f"{key} has shape {tuple(weights[key].shape)}, not {shape}: {who} needs {fmt}")
            out[f'{idx}.{kind}'] = weights[key]
    return out


class Trunk:
    def __init__(self, n_convs, relu_last, state):
        """state: what load_vgg16_features returned"""
        self.last, self.relu_last, self.pool_after = n_convs - 1, relu_last, pool_after(n_convs)
        self.seq = sequential(n_convs, relu_last)
        self.seq.load_state_dict(state)
        for param in self.seq.parameters():
            param.requires_grad = False
        self._packs = None

    def convs(self):
        return [self.seq[i] for i in CONV_INDICES[:self.last + 1]]

    def pack_key(self):
        """the device and every `_version`: another key when the owner has moved or a weight was written"""
        convs = self.convs()
        return (convs[0].weight.device,) + tuple(t._version for c in convs for t in (c.weight, c.bias))

    def packed(self):
        """[key, forward packs, transposed packs or None] of the frozen convolutions on their device, made once; made again
        when the key has changed."""
        key = self.pack_key()
        if self._packs is None or self._packs[0] != key:
            self._packs = [key, [ops.PackedConv(c.weight, c.bias) for c in self.convs()], None]
        return self._packs

    def packed_transposed(self):
        p = self.packed()
        if p[2] is None:
            p[2] = [ops.packed_transposed(c.weight) for c in self.convs()]
        return p[2]

    def forward_torch(self, x, tap=None):
        """The top layer of x in x's dtype, in plain torch; `tap(i, t)` sees every ReLU output t, before its pool."""
        for i, c in enumerate(self.convs()):
            x = F.conv2d(x, c.weight.to(x.dtype), c.bias.to(x.dtype), padding=1)
            if i == self.last and not self.relu_last:
                break
            x = F.relu(x)
            if tap is not None:
                tap(i, x)
            if i in self.pool_after:
                x = F.max_pool2d(x, 2, 2)
        return x

    def forward_hip(self, x, tap=None, keep=None):
        """The top layer of x (N, 3, H, W) fp32 on the device.  `tap(i, t)` sees every ReLU output t, before its pool, and
        `keep` (a list) receives them.  An odd plane is convolved unfused and pooled with MaxPool2d's floor."""
        for i, pc in enumerate(self.packed()[1]):
            if i == self.last and not self.relu_last:
                return ops.conv2d(x, pc, "zeros", None)
            h, w = x.shape[2:]
            if i in self.pool_after and h % 2 == 0 and w % 2 == 0:
                t, x = ops.conv2d_pool2(x, pc, True, "zeros", "relu")
            else:
                t = ops.conv2d(x, pc, "zeros", "relu")
                x = ops.pool2(t, True) if i in self.pool_after else t
            if tap is not None:
                tap(i, t)
            if keep is not None:
                keep.append(t)
        return x

    def backward_hip(self, g, ys, tap=None):
        """The gradient of the input (B, 3, H, W) from g, the gradient of the top convolution's output.  ys[i]: ReLU output
        i of forward_hip on those B images (even planes only).  `tap(i, above)` -> the gradient at a pooled ReLU output i
        from `above`, what the pool routes to it; without it that is `above` itself."""
        pT = self.packed_transposed()
        for i in range(self.last, 0, -1):
            gx = ops.conv2d_backward_data(g, pT[i], "zeros")            # gradient of layer i's input
            if i - 1 in self.pool_after:                                # ... which is the max-pool of relu output i - 1
                g = ops.pool2_max_backward(ys[i - 1], gx)
                if tap is not None:
                    g = tap(i - 1, g)
            else:
                g = ops.relu_mask_(gx, ys[i - 1])
        return ops.conv2d_backward_data(g, pT[0], "zeros")
