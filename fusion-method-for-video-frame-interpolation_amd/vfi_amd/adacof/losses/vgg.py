"""Perceptual loss of the AdaCoF trainer -- mirror of reference src/adacof/losses/vgg.py:7-22:
`F.mse_loss(conv4_3(output), conv4_3(gt.detach()))` with the first 22 layers of torchvision's `vgg16.features`, frozen,
on the raw [0, 1] images (the reference applies no ImageNet normalisation).

The layers are the first ten convolutions of `vfi_amd.vgg16`'s table, without the last one's ReLU (the slice ends on
conv4_3); that module holds the table, the loader, the pack cache and the walks.  The `nn.Sequential` of its `Trunk` is
registered here under the reference's name, so `state_dict()` has the reference's keys
(`vgg16_conv_4_3.<index>.{weight,bias}`).

With fp32 HIP tensors the whole term is one autograd node (`_VGGFunction`): output and target run as one batch of 2B through
`Trunk.forward_hip`, the loss is `ops.mse_forward` on the two halves of the conv4_3 tensor, and the backward is
`ops.mse_backward` followed by `Trunk.backward_hip` on the B images of the output half.  Only `output` gets a gradient.  Of
each ReLU output the node keeps the output half (a view: the 2B tensor's memory stays until the backward has run).  Without
a tensor that requires grad, or with grad mode off, the same forward runs without a node.  CPU or float64 arguments take
`Trunk.forward_torch`, the same table in plain torch.

Differences from the reference:

* Nothing is downloaded.  `VGG(weights=...)` takes a torchvision `vgg16` state dict -- the dict itself or the path of a file
  `torch.load` reads (torchvision's `vgg16-397923af.pth`) -- and reads its keys `features.{0,2,...,21}.{weight,bias}`; every
  other key is ignored.  No weights, or a missing file, raise an error that says so.
* H and W must be multiples of 8 (the fused pool and its adjoint take even planes; the reference trains on 256x256
  patches): anything else raises ValueError before a kernel runs, on every path.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops, vgg16

N_CONVS = 10
CONV_INDICES = vgg16.CONV_INDICES[:N_CONVS]
CHANNELS = vgg16.CHANNELS[:N_CONVS + 1]


def _sequential():
    """vgg16.features[:22]"""
    return vgg16.sequential(N_CONVS, False)


def load_vgg16_features(weights):
    """-> {'<index>.weight' / '<index>.bias': tensor} of the ten convolutions from a vgg16 state dict or its file."""
    return vgg16.load_vgg16_features(weights, N_CONVS, "the VGG loss", "weights")


def _check_size(output, gt):
    if output.dim() != 4 or output.shape[1] != 3 or tuple(output.shape) != tuple(gt.shape):
        raise ValueError(f"VGG: output {tuple(output.shape)} and gt {tuple(gt.shape)} must be equal (B, 3, H, W)")
    h, w = int(output.shape[2]), int(output.shape[3])
    if h % 8 or w % 8 or h < 8 or w < 8:
        raise ValueError(f"VGG: H and W must be multiples of 8, got {h}x{w}")


class VGG(nn.Module):
    def __init__(self, weights=None):
        super(VGG, self).__init__()
        self._trunk = vgg16.Trunk(N_CONVS, False, load_vgg16_features(weights))
        self.vgg16_conv_4_3 = self._trunk.seq

    def packed(self):
        return self._trunk.packed()

    def packed_transposed(self):
        return self._trunk.packed_transposed()

    def _features_hip(self, x, relu_outputs=None):
        """conv4_3 of x (N, 3, H, W) fp32 on the device; relu_outputs (a list or None) receives the nine ReLU outputs."""
        return self._trunk.forward_hip(x, keep=relu_outputs)

    def forward(self, output, gt):
        _check_size(output, gt)
        gt = gt.detach()
        if not (output.is_cuda and gt.is_cuda and output.dtype == torch.float32 and gt.dtype == torch.float32):
            vgg_output = self._trunk.forward_torch(output)
            with torch.no_grad():
                vgg_gt = self._trunk.forward_torch(gt)
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
        net.packed_transposed()                                         # a first backward packs before its first kernel
        g, _ = ops.mse_backward(feat[:b], feat[b:], upstream.contiguous(), need_a=True, need_b=False)
        ctx.keep = None
        return None, net._trunk.backward_hip(g, ys), None
