"""Plain-torch restatements for the WGAN_GP tests, in any dtype, no GPU, no vfi_amd import:

* the discriminator without BatchNorm as a function of an ordered parameter list, every LeakyReLU an explicit multiplication
  by a scale tensor (1 where the mask holds, SLOPE elsewhere) built in the operand's dtype -- so in float64 the constant is
  the double 0.2, not a float32 rounding of it;
* the gradient penalty;
* the first backward and the second-order pass written out layer by layer (`chain`), the identity the HIP node is built on.

Layers k = 1..10 (eight convolutions, two linear layers): z_k = A_k h_{k-1} (+ b_k), h_k = s_k * z_k, no activation after 10.
First backward: u_10 = 1, ubar_{k-1} = A_k^T u_k, u_{k-1} = s_{k-1} * ubar_{k-1}, g = ubar_0.
Penalty P = weight * mean_b (||g_b|| - 1)^2, v_0 = dP/dg.  Second-order pass: dP/dA_k = wgrad(input = v_{k-1}, grad_out =
u_k), v_k = s_k * (A_k v_{k-1})."""
import torch
import torch.nn.functional as F
from torch.nn import grad as G

import adversarial_ref as AR

SLOPE = AR.SLOPE
WEIGHT = 10.0
BLOCKS = AR.BLOCKS
NB = len(BLOCKS)


def args(patch_size, **kw):
    kw.setdefault("gradient_penalty", True)
    return AR.args(patch_size, **kw)


def param_keys():
    """The order of the nodes' parameters: the eight filters, then the classifier's four."""
    return [f"features.{i}.0.weight" for i in range(NB)] + ["classifier.0.weight", "classifier.0.bias", "classifier.2.weight",
                                                           "classifier.2.bias"]


def weight_keys():
    return param_keys()[:NB] + ["classifier.0.weight", "classifier.2.weight"]


def layout(patch_size):
    out = {f"features.{i}.0.weight": (cout, cin, 3, 3) for i, (cin, cout, _) in enumerate(BLOCKS)}
    p = patch_size // 16
    out.update({"classifier.0.weight": (1024, 512 * p * p), "classifier.0.bias": (1024,), "classifier.2.weight": (1, 1024),
                "classifier.2.bias": (1,)})
    return out


def scale(mask, dtype):
    return torch.where(mask, torch.ones((), dtype=dtype), torch.full((), SLOPE, dtype=dtype))


def forward(params, x, masks=None, keep=None):
    """Logits (B, 1).  masks: 9 bool tensors (the eight blocks' pre-activations > 0, the hidden layer's > 0); None: the sign
    of this forward's own values.  keep: a list that receives the 9 masks used."""
    t = x
    used = []
    for i, (_, _, stride) in enumerate(BLOCKS):
        z = F.conv2d(t, params[i], stride=stride, padding=1)
        m = (z.detach() > 0) if masks is None else masks[i]
        used.append(m)
        t = z * scale(m, z.dtype)
    l1w, l1b, l2w, l2b = params[NB:]
    z = F.linear(t.flatten(1), l1w, l1b)
    m = (z.detach() > 0) if masks is None else masks[NB]
    used.append(m)
    if keep is not None:
        keep.extend(used)
    return F.linear(z * scale(m, z.dtype), l2w, l2b)


def penalty(g, weight=WEIGHT):
    return weight * g.flatten(1).norm(2, dim=1).sub(1).pow(2).mean()


def input_gradient(params, x, masks):
    """d sum(logits) / dx by autograd, with the graph kept (differentiable in the parameters)."""
    x = x.detach().requires_grad_(True)
    return torch.autograd.grad(forward(params, x, masks).sum(), x, create_graph=True)[0]


def chain(params, x, masks, weight=WEIGHT, drop_tangent_mask=False, shift_u=False):
    """-> (g, P, {key: dP/dparam}) by the written-out first backward and second-order pass; no autograd.  The two flags are
    the mutants of section 28: the mask left off the tangent; u_{k+1} used for u_k -- carried to layer k's shape by A_{k+1}^T,
    i.e. ubar_k, the gradient before layer k's own mask (the shapes of u_{k+1} and u_k differ at every layer)."""
    params = [p.detach() for p in params]
    dtype = x.dtype
    s = [scale(m, dtype) for m in masks]
    # forward, for the shapes and the layer inputs' sizes
    sizes, t = [], x.detach()
    for i, (_, _, stride) in enumerate(BLOCKS):
        sizes.append(tuple(t.shape))
        t = F.conv2d(t, params[i], stride=stride, padding=1) * s[i]
    feat_shape = tuple(t.shape)
    l1w, _, l2w, _ = params[NB:]
    b = x.shape[0]
    # first backward
    u, unmasked = [None] * (NB + 2), [None] * (NB + 2)
    u[NB + 1] = unmasked[NB + 1] = torch.ones((b, 1), dtype=dtype)
    unmasked[NB] = u[NB + 1] @ l2w
    u[NB] = unmasked[NB] * s[NB]
    ubar = (u[NB] @ l1w).view(feat_shape)
    for i in range(NB - 1, -1, -1):
        unmasked[i] = ubar
        u[i] = ubar * s[i]
        ubar = G.conv2d_input(sizes[i], params[i], u[i], stride=BLOCKS[i][2], padding=1)
    g = ubar
    if shift_u:
        u = unmasked
    # penalty and v_0
    norms = g.flatten(1).norm(2, dim=1)
    value = weight * (norms - 1).pow(2).mean()
    coef = torch.where(norms == 0, torch.zeros_like(norms), weight * 2 * (norms - 1) / (b * norms.clamp_min(1e-300)))
    v = coef.view(-1, 1, 1, 1) * g
    # second-order pass
    grads = {}
    keys = param_keys()
    for i, (_, _, stride) in enumerate(BLOCKS):
        grads[keys[i]] = G.conv2d_weight(v, tuple(params[i].shape), u[i], stride=stride, padding=1)
        v = F.conv2d(v, params[i], stride=stride, padding=1)
        if not drop_tangent_mask:
            v = v * s[i]
    v = v.flatten(1)
    grads["classifier.0.weight"] = u[NB].t() @ v
    grads["classifier.0.bias"] = torch.zeros_like(params[NB + 1])
    v = v @ l1w.t()
    if not drop_tangent_mask:
        v = v * s[NB]
    grads["classifier.2.weight"] = u[NB + 1].t() @ v
    grads["classifier.2.bias"] = torch.zeros_like(params[NB + 3])
    return g, value, grads


def autograd_reference(params, x, masks, dtype, upstream, weight=WEIGHT):
    """Everything the whole-network GPU test compares, by autograd of `forward` in `dtype` on the CPU with the masks fixed:
    dict(logits, dx, dparams (list), g, penalty, dpenalty (list over weight_keys()))."""
    ps = [p.detach().cpu().to(dtype).requires_grad_(True) for p in params]
    ms = [m.cpu() for m in masks]
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    out = forward(ps, xd, ms)
    grads = torch.autograd.grad((out * upstream.cpu().to(dtype)).sum(), [xd] + ps)
    g = input_gradient(ps, xd, ms)
    value = penalty(g, weight)
    index = {k: i for i, k in enumerate(param_keys())}
    dpen = torch.autograd.grad(value, [ps[index[k]] for k in weight_keys()])
    return dict(logits=out.detach(), dx=grads[0], dparams=list(grads[1:]), g=g.detach(), penalty=value.detach(), dpenalty=list(dpen))


rel = AR.rel
