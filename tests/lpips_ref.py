"""References of LPIPS (tests/test_lpips_host.py, tests/test_lpips_gpu.py).

* `vgg16_state`: a seeded dict with torchvision's vgg16 key set and real, He-scaled weights for all thirteen convolutions
  (std sqrt(2 / (9 Cin)): activations stay O(1) through the trunk); `classifier.*` as zero-stride views.
* `head_weights` / `head_weights_dict`: seeded head weights, uniform in [0, 1) with some exact zeros, in piq's format (five
  tensors (1, C, 1, 1)) and in the `lpips` package's (keys `lin{l}.model.1.weight`).
* `head`: the head's formula in the dtype of its arguments, the norm through a safe square root: a pixel whose x is zero
  gives x a gradient of 0 there, not NaN.
* `head_inputs`: ReLU-like maps with exact zeros and with pixels that are zero in x only, in y only and in both.
* `lpips_plain`: the thirteen layers written out with `MaxPool2d`'s floor, in plain torch.
* `lpips_decisions` / `lpips_pinned`: the score with every ReLU mask and every pool's argmax taken from the product's own
  fp32 forward, as sections 12 / 13 / 23 pin theirs: float64 autograd of it is the reference, float32 autograd of it the
  yardstick of what fp32 loses.
"""
import torch
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
WIDTHS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOLED = (1, 3, 6, 9)
TAPPED = (1, 3, 6, 9, 12)
TAP_WIDTHS = (64, 128, 256, 512, 512)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EPS = 1e-10


def vgg16_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, idx in enumerate(CONVS):
        cin, cout = WIDTHS[i], WIDTHS[i + 1]
        sd[f"features.{idx}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn((cout,), generator=g) * 0.05
    ghost = lambda *shape: torch.zeros(1).expand(*shape)
    for idx, (o, i) in ((0, (4096, 25088)), (3, (4096, 4096)), (6, (1000, 4096))):
        sd[f"classifier.{idx}.weight"], sd[f"classifier.{idx}.bias"] = ghost(o, i), ghost(o)
    return sd


def head_weights(seed=0):
    """piq's format: five tensors (1, C, 1, 1)"""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for c in TAP_WIDTHS:
        w = torch.rand((c,), generator=g)
        w[torch.rand((c,), generator=g) < 0.1] = 0.0
        out.append(w.view(1, c, 1, 1))
    return out


def head_weights_dict(seed=0):
    """the lpips package's format"""
    return {f"lin{l}.model.1.weight": w.clone() for l, w in enumerate(head_weights(seed))}


def unit(x):
    n2 = (x * x).sum(1, keepdim=True)
    live = n2 > 0
    norm = torch.sqrt(torch.where(live, n2, torch.ones_like(n2)))
    return torch.where(live, x / (norm + EPS), torch.zeros_like(x))


def head(x, y, w):
    """x, y (N, C, ...) -> (N,): 1 / HW sum_p sum_c w_c (xh_c - yh_c)^2"""
    d = (unit(x) - unit(y)) ** 2 * w.to(x.dtype).reshape(1, -1, *([1] * (x.dim() - 2)))
    return d.flatten(1).sum(1) / x[0, 0].numel()


def head_inputs(n, c, hw, seed=0):
    """-> x, y (N, C, HW) fp32, w (C,): ReLU-like, about a third exact zeros; when there is room, pixel 0 of every image is
    zero in x only, pixel 1 in y only, pixel 2 in both"""
    g = torch.Generator().manual_seed(seed * 7919 + n * 131 + c * 17 + hw)
    x = torch.relu(torch.randn((n, c, hw), generator=g) + 0.4)
    y = torch.relu(torch.randn((n, c, hw), generator=g) + 0.4)
    if hw >= 3:
        x[:, :, 0] = 0
        y[:, :, 1] = 0
        x[:, :, 2] = 0
        y[:, :, 2] = 0
    w = torch.rand((c,), generator=g)
    if c > 2:
        w[torch.rand((c,), generator=g) < 0.1] = 0.0
    return x, y, w


def normalize(x):
    mean, std = (torch.tensor(v, dtype=x.dtype).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (x - mean) / std


def lpips_plain(sd, heads, x, y):
    """(B,) in x's dtype: normalisation, the thirteen layers, the five heads in tap order; MaxPool2d floors odd planes"""
    c = lambda z, idx: F.relu(F.conv2d(z, sd[f"features.{idx}.weight"].to(z.dtype), sd[f"features.{idx}.bias"].to(z.dtype), padding=1))
    h = lambda a, b, l: head(a, b, heads[l].reshape(-1))
    fx, fy = normalize(x), normalize(y)
    score = 0
    r12x, r12y = c(c(fx, 0), 2), c(c(fy, 0), 2)
    score = score + h(r12x, r12y, 0)
    r22x, r22y = c(c(F.max_pool2d(r12x, 2), 5), 7), c(c(F.max_pool2d(r12y, 2), 5), 7)
    score = score + h(r22x, r22y, 1)
    r33x, r33y = c(c(c(F.max_pool2d(r22x, 2), 10), 12), 14), c(c(c(F.max_pool2d(r22y, 2), 10), 12), 14)
    score = score + h(r33x, r33y, 2)
    r43x, r43y = c(c(c(F.max_pool2d(r33x, 2), 17), 19), 21), c(c(c(F.max_pool2d(r33y, 2), 17), 19), 21)
    score = score + h(r43x, r43y, 3)
    r53x, r53y = c(c(c(F.max_pool2d(r43x, 2), 24), 26), 28), c(c(c(F.max_pool2d(r43y, 2), 24), 26), 28)
    return score + h(r53x, r53y, 4)


def lpips_decisions(node, x, y):
    """node: the product's LPIPS on the device; x, y (B, 3, H, W) fp32 on the device -> per layer (mask (2B, C, H, W) bool,
    argmax indices of its 2x2 pool or None), on the host, from the product's own fp32 forward."""
    ts = []
    with torch.no_grad():
        node._score_hip(x, y, ts)
    out = []
    for i, t in enumerate(ts):
        t = t.cpu()
        idx = F.max_pool2d(t, 2, 2, return_indices=True)[1] if i in POOLED else None
        out.append((t > 0, idx))
    return out


def _taps_pinned(sd, x, decisions):
    z, taps = normalize(x), []
    for i, idx in enumerate(CONVS):
        z = F.conv2d(z, sd[f"features.{idx}.weight"].to(z.dtype), sd[f"features.{idx}.bias"].to(z.dtype), padding=1)
        mask, arg = decisions[i]
        z = z * mask.to(z.dtype)
        if i in TAPPED:
            taps.append(z)
        if arg is not None:
            n, c, h, w = z.shape
            z = z.flatten(2).gather(2, arg.flatten(2)).view(n, c, h // 2, w // 2)
    return taps


def lpips_pinned(sd, heads, x, y, decisions):
    """decisions: of the batch cat([x, y]); -> (B,) scores, differentiable in x"""
    b = x.shape[0]
    tx = _taps_pinned(sd, x, [(m[:b], None if a is None else a[:b]) for m, a in decisions])
    with torch.no_grad():
        ty = _taps_pinned(sd, y, [(m[b:], None if a is None else a[b:]) for m, a in decisions])
    score = 0
    for l in range(len(TAPPED)):
        score = score + head(tx[l], ty[l], heads[l].reshape(-1))
    return score
