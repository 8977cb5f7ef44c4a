"""References of the AdaCoF trainer's loss side (tests/test_adacof_losses_host.py, test_adacof_losses_gpu.py,
test_adacof_trainer_gpu.py).

* `vgg16_state`: a seeded dict with torchvision's full vgg16 key set.  The ten convolutions the loss reads are He-scaled
  (std sqrt(2 / (9 Cin)), so activations stay O(1) through ten layers); the keys it must ignore (features.24/26/28,
  classifier.*) have torchvision's shapes as zero-stride views, so the 4096 x 25088 matrix costs no memory.
* `vgg_sequential`: vgg16.features[:22] written out.
* `vgg_loss_pinned`: the loss in a given dtype with every ReLU mask and every pool's argmax taken from recorded decisions
  (`vgg_decisions`: the product's fp32 forward, op by op), as sections 12 / 13 pin theirs: float64 autograd of it is the
  reference, float32 autograd of it the yardstick of what fp32 loses.
* `write_middlebury`: a Middlebury-shaped tree (`input/<name>/frame10.png, frame11.png`, `gt/<name>/frame10i11.png`).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
WIDTHS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512)
POOLED = (1, 3, 6)
MIDDLEBURY = ['Beanbags', 'Dimetrodon', 'DogDance', 'Grove2', 'Grove3', 'Hydrangea', 'MiniCooper', 'RubberWhale', 'Urban2',
              'Urban3', 'Venus', 'Walking']


def vgg16_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, idx in enumerate(CONVS):
        cin, cout = WIDTHS[i], WIDTHS[i + 1]
        sd[f"features.{idx}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn((cout,), generator=g) * 0.05
    ghost = lambda *shape: torch.zeros(1).expand(*shape)
    for idx in (24, 26, 28):
        sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"] = ghost(512, 512, 3, 3), ghost(512)
    for idx, (o, i) in ((0, (4096, 25088)), (3, (4096, 4096)), (6, (1000, 4096))):
        sd[f"classifier.{idx}.weight"], sd[f"classifier.{idx}.bias"] = ghost(o, i), ghost(o)
    return sd


def vgg_sequential(sd, dtype=torch.float64):
    """torchvision's vgg16.features[:22] with the weights of `sd`"""
    c = lambda i, o: nn.Conv2d(i, o, kernel_size=3, padding=1)
    seq = nn.Sequential(c(3, 64), nn.ReLU(), c(64, 64), nn.ReLU(), nn.MaxPool2d(2, 2),
                        c(64, 128), nn.ReLU(), c(128, 128), nn.ReLU(), nn.MaxPool2d(2, 2),
                        c(128, 256), nn.ReLU(), c(256, 256), nn.ReLU(), c(256, 256), nn.ReLU(), nn.MaxPool2d(2, 2),
                        c(256, 512), nn.ReLU(), c(512, 512), nn.ReLU(), c(512, 512))
    assert len(seq) == 22
    seq.load_state_dict({k[len("features."):]: v for k, v in sd.items()
                         if k.startswith("features.") and int(k.split(".")[1]) in CONVS})
    return seq.to(dtype)


def vgg_decisions(node, x):
    """node: the product's VGG on the device; x (N, 3, H, W) fp32 on the device -> per ReLU layer (mask (N, C, H, W) bool,
    argmax indices of its 2x2 pool or None), on the host, from the product's own fp32 forward."""
    ys = []
    with torch.no_grad():
        node._features_hip(x.contiguous(), ys)
    out = []
    for i, y in enumerate(ys):
        y = y.cpu()
        idx = F.max_pool2d(y, 2, 2, return_indices=True)[1] if i in POOLED else None
        out.append((y > 0, idx))
    return out


def vgg_features_pinned(sd, x, decisions):
    """conv4_3 of x in x's dtype; ReLU = multiplication by the recorded mask, pool = gather at the recorded indices"""
    for i, idx in enumerate(CONVS):
        x = F.conv2d(x, sd[f"features.{idx}.weight"].to(x.dtype), sd[f"features.{idx}.bias"].to(x.dtype), padding=1)
        if i == len(CONVS) - 1:
            break
        mask, arg = decisions[i]
        x = x * mask.to(x.dtype)
        if arg is not None:
            n, c, h, w = x.shape
            x = x.flatten(2).gather(2, arg.flatten(2)).view(n, c, h // 2, w // 2)
    return x


def vgg_loss_pinned(sd, output, gt, decisions):
    """decisions: of the batch cat([output, gt]); -> the loss, differentiable in `output`"""
    b = output.shape[0]
    f_out = vgg_features_pinned(sd, output, [(m[:b], None if a is None else a[:b]) for m, a in decisions])
    with torch.no_grad():
        f_gt = vgg_features_pinned(sd, gt, [(m[b:], None if a is None else a[b:]) for m, a in decisions])
    return F.mse_loss(f_out, f_gt)


def write_middlebury(root, height, width, seed=0, names=MIDDLEBURY):
    """-> (input_dir, gt_dir): smooth seeded frames with a small motion"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    for n, name in enumerate(names):
        ph = rng.random(3) * 6
        for k, (sub, fname) in enumerate((("input", "frame10.png"), ("gt", "frame10i11.png"), ("input", "frame11.png"))):
            img = np.stack([0.5 + 0.4 * np.sin((xx + 1.5 * k) * (0.21 + 0.05 * c) + ph[c]) * np.cos((yy - k) * (0.17 + 0.04 * c) + n)
                            for c in range(3)], -1)
            d = os.path.join(root, sub, name)
            os.makedirs(d, exist_ok=True)
            Image.fromarray((img * 255).round().astype(np.uint8)).save(os.path.join(d, fname))
    return os.path.join(root, "input"), os.path.join(root, "gt")
