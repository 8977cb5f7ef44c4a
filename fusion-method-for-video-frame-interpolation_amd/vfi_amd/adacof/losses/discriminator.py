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

`Discriminator(args, 'WGAN_GP')` is the reference's variant without BatchNorm (`BasicBlock(..., bn=False)`: state-dict keys
`features.{i}.0.weight` plus the classifier's four), built only when `args.gradient_penalty` is true.
On the HIP route it is one autograd node too (`ops.conv2d` -> `ops.leaky_mask` per block, the two `ops.linear_forward`s).
Both nodes are `_walk_forward` / `_walk_backward` over the eight blocks and the classifier, BatchNorm being a stage that the
network has or has not; a block's convolution and its adjoint, stride 1 or 2, are `_block_forward` / `_block_backward`.
`input_gradient(x)` returns d sum D(x) / dx as a function of the parameters: on the HIP route a second node whose backward is
the second-order pass of section 28 -- the existing weight-gradient and forward kernels with the tangent in the input's seat,
LeakyReLU's second derivative being zero -- and on the plain route torch's `autograd.grad(..., create_graph=True)`.

Differences from the reference:

* `gan_type='WGAN_GP'` needs `args.gradient_penalty` (without it: NotImplementedError, as before it was built), and
  `Temporal_Discriminator` is not built (no Conv3d): `losses.Loss` refuses `T_WGAN_GP`.
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


def _split(conv, t):
    """What the stride-1 kernels of a block read: its input t, or t's phase split when the block has stride 2."""
    return ops.phase_split(t) if conv.stride[0] == 2 else t


def _block_forward(conv, t, w=None, w_eff=None, split=None):
    """A block's convolution of t -> (split input, (H, W) of t, effective filter, pre-activation).  The filter is made from
    the weight w, or is `w_eff` of an earlier call; `split`: _split(conv, t) when the caller already has it."""
    stride2 = conv.stride[0] == 2
    if w_eff is None:
        w_eff = ops.stride2_weight(w) if stride2 else w.detach()
    if split is None:
        split = _split(conv, t)
    pc = ops.PackedConv(w_eff)
    y = ops.conv2d_stride2(t, pc, split=split) if stride2 else ops.conv2d(t, pc, "zeros", None)
    return split, tuple(t.shape[2:]), w_eff, y


def _block_backward(conv, t_in, size, w_eff, g_y, need_w, need_x=False):
    """The adjoint of _block_forward from g_y, the gradient at the pre-activation -> (weight gradient, gradient of the
    block's input), each None when not needed."""
    stride2 = conv.stride[0] == 2
    dw = g_in = None
    if need_w:
        dw = (ops.conv2d_stride2_backward_weight(None, g_y, bias=False, split=t_in) if stride2
              else ops.conv2d_backward_weight(t_in, g_y, 3, "zeros", bias=False))[0]
    if need_x:
        pct = ops.packed_transposed(w_eff)
        g_in = ops.conv2d_stride2_backward_data(g_y, pct, size) if stride2 else ops.conv2d_backward_data(g_y, pct, "zeros")
    return dw, g_in


def _walk_forward(net, x, params):
    """The network, one ops call after the other -> (logits, state).  Per block: the convolution, then with BatchNorm the
    batch statistics, the running ones' update and `bn_leaky_forward`; without, LeakyReLU in place (`leaky_mask` with the
    output as its own sign).  params: as _node_params() orders them.  state: (per block (input of the stride-1 convolution,
    (H, W) of the block's input, effective filter, activation's output[, pre-activation, mean, var]), flat, hid)."""
    k = 3 if net._bn else 1
    saved = []
    t = x.contiguous()
    for i, blk in enumerate(net.features):
        t_in, size, w_eff, y = _block_forward(blk[0], t, params[k * i])
        if net._bn:
            mean, var = ops.bn_stats(y)
            _update_running(blk[1], mean, var, y.shape[0] * y.shape[2] * y.shape[3])
            t = ops.bn_leaky_forward(y, mean, var, params[k * i + 1], params[k * i + 2], blk[1].eps, SLOPE)
            saved.append((t_in, size, w_eff, t, y, mean, var))
        else:
            t = ops.leaky_mask(y, y, SLOPE, out=y)
            saved.append((t_in, size, w_eff, t))
    l1w, l1b, l2w, l2b = params[-4:]
    flat = t.view(t.shape[0], -1)
    hid = ops.linear_forward(flat, l1w, l1b, SLOPE)
    logits = ops.linear_forward(hid, l2w, l2b, 1.0)
    return logits, (saved, flat, hid)


def _walk_backward(net, params, state, g, need_x, need_p, keep=None):
    """First backward of _walk_forward from the gradient g (B, 1) of the logits -> (dx or None, [dparam or None]).
    `keep`: a list that receives u_1 .. u_10, the gradients at the ten pre-activations, in that order."""
    saved, flat, hid = state
    k = 3 if net._bn else 1
    q = k * len(saved)
    grads = [None] * len(params)
    l1w, l2w = params[q], params[q + 2]
    g = g.contiguous()
    g_hid, grads[q + 2], grads[q + 3] = ops.linear_backward(hid, l2w, None, 1.0, g, True, need_p[q + 2], need_p[q + 3])
    if net._bn:
        g_flat, grads[q], grads[q + 1] = ops.linear_backward(flat, l1w, hid, SLOPE, g_hid, True, need_p[q], need_p[q + 1])
    else:                                                               # masked apart: u_9 is kept for the second-order pass
        g_hid = ops.leaky_mask(g_hid, hid, SLOPE, out=g_hid)
        g_flat, grads[q], grads[q + 1] = ops.linear_backward(flat, l1w, None, 1.0, g_hid, True, need_p[q], need_p[q + 1])
    us = [g_hid, g]
    g_t = g_flat.view(saved[-1][3].shape)
    for i in range(len(saved) - 1, -1, -1):
        t_in, size, w_eff, out = saved[i][:4]
        if net._bn:
            y, mean, var = saved[i][4:]
            g_y, g_gamma, g_beta = ops.bn_leaky_backward(g_t, out, y, mean, var, params[k * i + 1], net.features[i][1].eps, SLOPE,
                                                         out=g_t)
            if need_p[k * i + 1]:
                grads[k * i + 1] = g_gamma
            if need_p[k * i + 2]:
                grads[k * i + 2] = g_beta
        else:
            g_y = ops.leaky_mask(g_t, out, SLOPE, out=g_t)
        us.insert(0, g_y)
        grads[k * i], g_t = _block_backward(net.features[i][0], t_in, size, w_eff, g_y, need_p[k * i], i > 0 or need_x)
    if keep is not None:
        keep.extend(us)
    return g_t, grads


class _WalkNode(torch.autograd.Function):
    """logits (B, 1) of the whole network from x (B, C, H, W); inputs: net, x, then the parameters as _node_params() orders
    them."""

    @staticmethod
    def forward(ctx, net, x, *params):
        logits, ctx.state = _walk_forward(net, x, params)
        ctx.net, ctx.params = net, [p.detach() for p in params]
        return logits

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        g_x, grads = _walk_backward(ctx.net, ctx.params, ctx.state, g, need[1], need[2:])
        return (None, g_x) + tuple(grads)


class _DiscriminatorNode(_WalkNode):
    """The walk with BatchNorm: per block (conv.weight, bn.weight, bn.bias), then (linear 1 weight, bias, linear 2 weight,
    bias)."""


class _CriticNode(_WalkNode):
    """The walk of the WGAN_GP discriminator (no BatchNorm): the eight convolution weights, then (linear 1 weight, bias,
    linear 2 weight, bias)."""


class _InputGradientNode(torch.autograd.Function):
    """g (B, C, H, W) = d sum_b D(x_b) / d x of the WGAN_GP discriminator, differentiable in the weights (section 28).

    forward: the network's forward and its first backward from u_10 = 1, keeping the activations (their signs s_k) and the
    gradients u_1 .. u_10 at the pre-activations.  backward, from v_0 = the gradient of g: between the LeakyReLU kinks the
    network is linear in every weight tensor and LeakyReLU's second derivative is 0, so for k = 1 .. 10
        dA_k = wgrad(input = v_{k-1}, grad_out = u_k),    v_k = s_k * (A_k v_{k-1})
    -- the existing weight-gradient kernels with the tangent in the input's seat and the existing forward kernels without
    bias.  The biases and x get nothing from g."""

    @staticmethod
    def forward(ctx, net, x, *params):
        params = [p.detach() for p in params]
        _, state = _walk_forward(net, x, params)
        us = []
        ones = torch.ones((x.shape[0], 1), dtype=torch.float32, device=x.device)
        g, _ = _walk_backward(net, params, state, ones, True, [False] * len(params), keep=us)
        ctx.net, ctx.params, ctx.us = net, params, us
        ctx.signs = [s[3] for s in state[0]] + [state[2]]
        ctx.filters = [s[2] for s in state[0]]
        return g

    @staticmethod
    def backward(ctx, v):
        need_p = ctx.needs_input_grad[2:]
        net, params, us, signs = ctx.net, ctx.params, ctx.us, ctx.signs
        nb = len(ctx.filters)
        grads = [None] * len(params)
        v = v.contiguous()
        for i in range(nb):
            conv = net.features[i][0]
            v_in = _split(conv, v)
            grads[i] = _block_backward(conv, v_in, None, None, us[i], need_p[i])[0]
            w = _block_forward(conv, v, w_eff=ctx.filters[i], split=v_in)[3]
            v = ops.leaky_mask(w, signs[i], SLOPE, out=w)
        flat = v.view(v.shape[0], -1)
        if need_p[nb]:
            grads[nb] = ops.linear_backward(flat, None, None, 1.0, us[nb], False, True, False)[1]
        if need_p[nb + 2]:
            w = ops.linear_forward(flat, params[nb], None, 1.0)
            v = ops.leaky_mask(w, signs[nb], SLOPE, out=w)
            grads[nb + 2] = ops.linear_backward(v, None, None, 1.0, us[nb + 1], False, True, False)[1]
        return (None, None) + tuple(grads)


class _HipRoute:
    """What Discriminator and FI_Discriminator share: the choice of route and the node's argument list."""
    _frozen = False
    _bn = True

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
            ps += [blk[0].weight, blk[1].weight, blk[1].bias] if self._bn else [blk[0].weight]
        ps += [self.classifier[0].weight, self.classifier[0].bias, self.classifier[2].weight, self.classifier[2].bias]
        return ps

    def _on_hip(self, x, needs_x=True):
        ps = self._node_params()
        return (self.training and torch.is_grad_enabled() and x.dim() == 4
                and all(t.is_cuda and t.dtype == torch.float32 for t in [x] + ps)
                and ((needs_x and x.requires_grad) or any(p.requires_grad for p in ps)))

    def _run(self, x):
        if self._on_hip(x):
            ps = self._node_params()
            if self._frozen:
                ps = [p.detach() for p in ps]
            return (_DiscriminatorNode if self._bn else _CriticNode).apply(self, x, *ps)
        features = self.features(x)
        return self.classifier(features.view(features.size(0), -1))


def _build(net, args, in_channels, bn=True):
    """Reference discriminator.py:23-51 (and :117-145, which differs in in_channels alone); bn=False: gan_type 'WGAN_GP'."""
    out_channels = 64
    depth = 7
    act = nn.LeakyReLU(negative_slope=SLOPE, inplace=True)

    m_features = [
        BasicBlock(in_channels, out_channels, 3, bn=bn, act=act)
    ]
    for i in range(depth):
        in_channels = out_channels
        if i % 2 == 1:
            stride = 1
            out_channels *= 2
        else:
            stride = 2
        m_features.append(BasicBlock(
            in_channels, out_channels, 3, stride=stride, bn=bn, act=act
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
        if gan_type == 'WGAN_GP' and not getattr(args, 'gradient_penalty', False):
            raise NotImplementedError("Discriminator: gan_type 'WGAN_GP' (no BatchNorm, a gradient penalty through a double "
                                      "backward) is not built")
        self._bn = gan_type != 'WGAN_GP'
        _build(self, args, 3, bn=self._bn)

    def forward(self, x):
        return self._run(x)

    def input_gradient(self, x):
        """g (B, C, H, W) = d sum_b D(x_b) / d x, differentiable with respect to the parameters (not to x): what WGAN_GP's
        gradient penalty is a function of.  The no-BatchNorm variant on the HIP route (training mode, fp32 device tensors,
        grad enabled, a parameter requiring grad): one autograd node, _InputGradientNode.  Anything else: torch's double
        backward, `autograd.grad(D(x).sum(), x, create_graph=True)`."""
        if not self._bn and self._on_hip(x, needs_x=False):
            ps = self._node_params()
            if self._frozen:
                ps = [p.detach() for p in ps]
            return _InputGradientNode.apply(self, x.detach(), *ps)
        with torch.enable_grad():
            x = x.detach().requires_grad_(True)
            return torch.autograd.grad(self(x).sum(), x, create_graph=True)[0]


class FI_Discriminator(_HipRoute, nn.Module):
    def __init__(self, args):
        super(FI_Discriminator, self).__init__()
        _build(self, args, 6)

    def forward(self, f0, f1):
        return self._run(torch.cat((f0, f1), dim=1))
