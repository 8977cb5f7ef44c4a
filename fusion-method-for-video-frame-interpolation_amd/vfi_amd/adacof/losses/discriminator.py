"""Discriminators of the AdaCoF trainer's GAN terms -- mirror of reference src/adacof/losses/discriminator.py:5-57,113-152
(`BasicBlock`, `Discriminator(args, gan_type)`, `FI_Discriminator(args)`; same structure, same submodule names, so
`state_dict()` has the reference's keys and a reference checkpoint loads).

Eight blocks `Conv2d(3x3, no bias) -> BatchNorm2d -> LeakyReLU(0.2)`, 3 (or 6) -> 64 channels, strides 1, 2, 1, 2, ..., the
channels doubling on every stride-1 block after the first, then `Linear(512 (patch_size // 16)^2, 1024) -> LeakyReLU(0.2) ->
Linear(1024, 1)`.

The submodules are real `nn.Conv2d` / `nn.BatchNorm2d` / `nn.Linear`; what runs depends on the call:

* the module in training mode, fp32 HIP tensors, grad enabled and the input or a parameter requiring grad: ONE autograd node
  over the HIP kernels -- `ops.conv2d` / `ops.conv2d_stride2` (the stride-2 blocks as a phase split + the stride-1 Winograd
  kernels), `ops.bn_stats` + `ops.bn_leaky_forward` (batch statistics), `ops.linear_forward`, and their adjoints;
* anything else (CPU tensors, float64, eval mode, no grad): the plain torch modules.

Either way a forward call in training mode updates `running_mean`, `running_var` (unbiased) and `num_batches_tracked` once, as
torch's BatchNorm2d does, and a batch with one value per channel raises torch's ValueError.

Differences from the reference:

* `gan_type='WGAN_GP'` and `Temporal_Discriminator` are not built (no double backward through the kernels, no Conv3d):
  `losses.Loss` refuses those types.
* `frozen()`: inside it the parameters enter the node detached, so a backward pass forms the input's gradient alone -- the
  generator's pass of `adversarial.Adversarial`, whose weight gradients the reference accumulates and zeroes unused.
"""
import contextlib

import torch
import torch.nn as nn

from ... import ops

SLOPE = 0.2


class BasicBlock(nn.Sequential):
    def __init__(
            self, in_channels, out_channels, kernel_size, stride=1, bias=False,
            bn=True, act=nn.ReLU(True)):

        m = [nn.Conv2d(
            in_channels, out_channels, kernel_size,
            padding=(kernel_size // 2), stride=stride, bias=bias)
        ]
        if bn: m.append(nn.BatchNorm2d(out_channels))
        if act is not None: m.append(act)
        super(BasicBlock, self).__init__(*m)


def _update_running(bn, mean, var, count):
    """nn.BatchNorm2d's bookkeeping of one training-mode forward call from the batch mean and BIASED variance."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    with torch.no_grad():
        bn.num_batches_tracked += 1
        m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
        bn.running_var.mul_(1.0 - m).add_(var, alpha=m * count / (count - 1.0))


class _DiscriminatorNode(torch.autograd.Function):
    """logits (B, 1) of the whole network from x (B, C, H, W); inputs: net, x, then per block (conv.weight, bn.weight, bn.bias),
    then (linear 1 weight, bias, linear 2 weight, bias)."""

    @staticmethod
    def forward(ctx, net, x, *params):
        blocks = list(net.features)
        saved = []
        t = x.contiguous()
        for i, blk in enumerate(blocks):
            conv, bn = blk[0], blk[1]
            w, gamma, beta = params[3 * i:3 * i + 3]
            n, _, h, wd = t.shape
            if conv.stride[0] == 2:
                w_eff = ops.stride2_weight(w)
                t_in = ops.phase_split(t)
            else:
                w_eff, t_in = w.detach(), t
            y = ops.conv2d(t_in, ops.PackedConv(w_eff), "zeros", None)
            mean, var = ops.bn_stats(y)
            _update_running(bn, mean, var, y.shape[0] * y.shape[2] * y.shape[3])
            out = ops.bn_leaky_forward(y, mean, var, gamma, beta, bn.eps, SLOPE)
            saved.append((t_in, (h, wd), w_eff, y, mean, var, out))
            t = out
        l1w, l1b, l2w, l2b = params[3 * len(blocks):]
        flat = t.view(t.shape[0], -1)
        hid = ops.linear_forward(flat, l1w, l1b, SLOPE)
        logits = ops.linear_forward(hid, l2w, l2b, 1.0)
        ctx.blocks, ctx.saved, ctx.flat, ctx.hid = blocks, saved, flat, hid
        ctx.params = [p.detach() for p in params]
        return logits

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        need_x, need_p = need[1], need[2:]
        blocks, params, nb = ctx.blocks, ctx.params, len(ctx.blocks)
        grads = [None] * len(params)
        l1w, l1b, l2w, l2b = params[3 * nb:]
        q = 3 * nb
        g_hid, grads[q + 2], grads[q + 3] = ops.linear_backward(ctx.hid, l2w, None, 1.0, g.contiguous(), True, need_p[q + 2],
                                                                need_p[q + 3])
        g_flat, grads[q], grads[q + 1] = ops.linear_backward(ctx.flat, l1w, ctx.hid, SLOPE, g_hid, True, need_p[q], need_p[q + 1])
        g_t = g_flat.view(ctx.saved[-1][6].shape)
        for i in range(nb - 1, -1, -1):
            t_in, size, w_eff, y, mean, var, out = ctx.saved[i]
            bn = blocks[i][1]
            stride2 = blocks[i][0].stride[0] == 2
            g_y, g_gamma, g_beta = ops.bn_leaky_backward(g_t, out, y, mean, var, params[3 * i + 1], bn.eps, SLOPE, out=g_t)
            if need_p[3 * i + 1]:
                grads[3 * i + 1] = g_gamma
            if need_p[3 * i + 2]:
                grads[3 * i + 2] = g_beta
            if need_p[3 * i]:
                dw, _ = ops.conv2d_backward_weight(t_in, g_y, 3, "zeros", bias=False)
                grads[3 * i] = ops.stride2_weight_gather(dw) if stride2 else dw
            if i == 0 and not need_x:
                g_t = None
                break
            g_in = ops.conv2d_backward_data(g_y, ops.packed_transposed(w_eff), "zeros")
            g_t = ops.phase_merge(g_in, size) if stride2 else g_in
        return (None, g_t) + tuple(grads)


class _HipRoute:
    """What Discriminator and FI_Discriminator share: the choice of route and the node's argument list."""
    _frozen = False

    @contextlib.contextmanager
    def frozen(self):
        """Inside: the HIP route takes the parameters detached (no weight gradients are formed); the plain-torch route is
        unchanged."""
        self._frozen = True
        try:
            yield self
        finally:
            self._frozen = False

    def _node_params(self):
        ps = []
        for blk in self.features:
            ps += [blk[0].weight, blk[1].weight, blk[1].bias]
        ps += [self.classifier[0].weight, self.classifier[0].bias, self.classifier[2].weight, self.classifier[2].bias]
        return ps

    def _on_hip(self, x):
        ps = self._node_params()
        return (self.training and torch.is_grad_enabled() and x.dim() == 4
                and all(t.is_cuda and t.dtype == torch.float32 for t in [x] + ps)
                and (x.requires_grad or any(p.requires_grad for p in ps)))

    def _run(self, x):
        if self._on_hip(x):
            ps = self._node_params()
            if self._frozen:
                ps = [p.detach() for p in ps]
            return _DiscriminatorNode.apply(self, x, *ps)
        features = self.features(x)
        return self.classifier(features.view(features.size(0), -1))


def _build(net, args, in_channels):
    """Reference discriminator.py:23-51 (and :117-145, which differs in in_channels alone)."""
    out_channels = 64
    depth = 7
    act = nn.LeakyReLU(negative_slope=SLOPE, inplace=True)

    m_features = [
        BasicBlock(in_channels, out_channels, 3, bn=True, act=act)
    ]
    for i in range(depth):
        in_channels = out_channels
        if i % 2 == 1:
            stride = 1
            out_channels *= 2
        else:
            stride = 2
        m_features.append(BasicBlock(
            in_channels, out_channels, 3, stride=stride, bn=True, act=act
        ))

    net.features = nn.Sequential(*m_features)

    patch_size = args.patch_size // (2 ** ((depth + 1) // 2))
    m_classifier = [
        nn.Linear(out_channels * patch_size ** 2, 1024),
        act,
        nn.Linear(1024, 1)
    ]
    net.classifier = nn.Sequential(*m_classifier)


class Discriminator(_HipRoute, nn.Module):
    def __init__(self, args, gan_type='GAN'):
        super(Discriminator, self).__init__()
        if gan_type == 'WGAN_GP':
            raise NotImplementedError("Discriminator: gan_type 'WGAN_GP' (no BatchNorm, a gradient penalty through a double "
                                      "backward) is not built")
        _build(self, args, 3)

    def forward(self, x):
        return self._run(x)


class FI_Discriminator(_HipRoute, nn.Module):
    def __init__(self, args):
        super(FI_Discriminator, self).__init__()
        _build(self, args, 6)

    def forward(self, f0, f1):
        return self._run(torch.cat((f0, f1), dim=1))
