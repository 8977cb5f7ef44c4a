#!/usr/bin/env python3
"""AdaCoFNet training step cost at the reference's training shape (batch 4, 256x256, kernel_size 5, dilation 1;
src/adacof/train.py): inference forward, training forward (activations kept), the HIP backward split by per-call HIP events
into weight gradients, input gradients, sampler and glue, and each new streaming kernel's effective TB/s (to be read
against profiles/r04_hbm_rates.txt: vfi_resize_bilinear 4.1-4.5 TB/s, plain copy 4.75-5.3 TB/s).  The same
KernelEstimation as plain torch.nn layers (MIOpen convolutions) on the same GPU is timed for context.

`--loss STRING` adds the trainer's step with that `vfi_amd.adacof.losses.Loss` (forward, loss, backward, Adamax step) next
to the default loss's, and, when the string has a VGG term, the VGG node alone (forward, backward to the image) and torch's
own nn.Sequential of the same ten layers (MIOpen), forward + backward to the input.  `--vgg-weights FILE` is a torchvision
vgg16 state dict; without it seeded He-scaled weights are used (the time does not depend on the values).  When the string
has a GAN term (`GAN`, `WGAN`, `FI_GAN`; the discriminator is sized by the frame: patch_size = H) it also prints the
discriminator alone: forward, and backward to the input and every parameter, next to torch's own
modules (MIOpen) of the same layers, and the two linear kernels' bytes per second on the 512 (H/16)^2 -> 1024 layer.  When it
has a `WGAN_GP` term (built with `gradient_penalty=True`) it prints the penalty pass split into the
forward, the first backward and the second-order pass (with the two penalty kernels), next to the `create_graph` double
backward of torch's own modules of the same layers.

`--device-optimizer` (with `--loss`) times every trainer step a second time with `device_optimizer=True`: the network's and
the discriminator's optimiser steps as one HIP pass each (vfi_amd.optim), all cases alternating over
five rounds: median and min .. max of each."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
from oracle import nets_cpu  # noqa: E402
from vfi_amd import _lib  # noqa: E402
from vfi_amd.adacof.models.adacofnet import AdaCoFNet  # noqa: E402


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


DEFAULT_LOSS = "1*Charb+0.01*g_Spatial+0.005*g_Occlusion"


def seeded_vgg16_state(seed=0):
    """He-scaled weights under torchvision's keys features.{0,...,21}.{weight,bias}"""
    from vfi_amd import vgg16
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, idx in enumerate(vgg16.CONV_INDICES[:10]):
        cin, cout = vgg16.CHANNELS[i], vgg16.CHANNELS[i + 1]
        sd[f"features.{idx}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn((cout,), generator=g) * 0.05
    return sd


def loss_section(net, f0, f1, f2, loss_string, vgg_weights, iters, warm, device_optimizer=False):
    from vfi_amd.adacof import losses, utility
    from vfi_amd.adacof.losses import vgg
    weights = vgg_weights or seeded_vgg16_state()
    net.train(True)
    cases = [(string, False) for string in dict.fromkeys((DEFAULT_LOSS, loss_string))]
    cases += [(string, True) for string, _ in cases] if device_optimizer else []
    steps = []
    for string, flag in cases:
        opt_args = types.SimpleNamespace(optimizer="ADAMax", lr=1e-3, weight_decay=0, device_optimizer=flag)
        crit = losses.Loss(types.SimpleNamespace(loss=string, vgg_weights=weights, gpu_id=0, patch_size=f0.shape[2],
                                                 gradient_penalty="WGAN_GP" in string.replace("T_WGAN_GP", ""),
                                                 decay_type="step", lr_decay=20, gamma=0.5, **vars(opt_args)))
        opt = utility.make_optimizer(opt_args, net)

        def step(crit=crit, opt=opt):
            opt.zero_grad()
            crit(net(f0, f2), f1, [f0, f2]).backward()
            opt.step()
        steps.append((f"  trainer step{', device optimiser' if flag else ''}, --loss {string}", step))
    rounds = 5 if device_optimizer else 1      # alternating, so that a difference can be read against the spread
    ms = [[] for _ in steps]
    for r in range(rounds):
        for i, (_, step) in enumerate(steps):
            ms[i].append(timed(step, iters, warm))
    for (label, _), m in zip(steps, ms):
        m.sort()
        spread = f"  (median of {rounds}, {m[0]:.3f} .. {m[-1]:.3f})" if rounds > 1 else ""
        print(f"{label}: {m[len(m) // 2]:8.3f} ms{spread}")
    if "GAN" in loss_string:
        discriminator_section(f0, iters, warm)
    if "WGAN_GP" in loss_string:
        gradient_penalty_section(f0, f1, iters, warm)
    if "VGG" not in loss_string:
        return
    node = vgg.VGG(weights).to(f0.device)
    x = f0.clone().requires_grad_(True)
    t_f = timed(lambda: node(x, f1), iters, warm)

    def vstep():
        x.grad = None
        node(x, f1).backward()
    t_s = timed(vstep, iters, warm)
    print(f"  VGG node alone: forward {t_f:.3f} ms, backward {t_s - t_f:.3f} ms")
    seq = vgg._sequential().to(f0.device)
    seq.load_state_dict(node.vgg16_conv_4_3.state_dict())
    for p in seq.parameters():
        p.requires_grad = False
    import torch.nn.functional as F

    def tloss():
        with torch.no_grad():
            t = seq(f1)
        return F.mse_loss(seq(x), t)
    t_tf = timed(tloss, iters, warm)

    def tstep():
        x.grad = None
        tloss().backward()
    t_ts = timed(tstep, iters, warm)
    print(f"  torch/MIOpen nn.Sequential of the ten layers: forward {t_tf:.3f} ms, backward {t_ts - t_tf:.3f} ms")


def discriminator_section(f0, iters, warm):
    from vfi_amd import ops
    from vfi_amd.adacof.losses.discriminator import Discriminator
    torch.manual_seed(0)
    net = Discriminator(types.SimpleNamespace(patch_size=f0.shape[2]), 'GAN').to(f0.device)
    x = f0.clone().requires_grad_(True)

    def step(module):
        x.grad = None
        module.zero_grad()
        module(x).sum().backward()
    t_f = timed(lambda: net(x), iters, warm)
    t_s = timed(lambda: step(net), iters, warm)
    print(f"  discriminator alone (HIP node): forward {t_f:.3f} ms, backward {t_s - t_f:.3f} ms")
    plain = torch.nn.Sequential(net.features, torch.nn.Flatten(), net.classifier)      # the same modules, torch's route
    t_tf = timed(lambda: plain(x), iters, warm)
    t_ts = timed(lambda: step(plain), iters, warm)
    print(f"  torch/MIOpen modules of the same layers: forward {t_tf:.3f} ms, backward {t_ts - t_tf:.3f} ms")
    lin = net.classifier[0]
    b, k, j = x.shape[0], lin.in_features, lin.out_features
    flat = torch.randn((b, k), device=x.device)
    g = torch.randn((b, j), device=x.device)
    y = ops.linear_forward(flat, lin.weight, lin.bias, 0.2)
    t_lf = timed(lambda: ops.linear_forward(flat, lin.weight, lin.bias, 0.2), iters, warm)
    t_lb = timed(lambda: ops.linear_backward(flat, lin.weight, y, 0.2, g), iters, warm)
    wb = 4.0 * j * k
    print(f"  linear {k} -> {j}, B {b}: forward {t_lf:.3f} ms, {wb / t_lf * 1e-9:.2f} TB/s (w read once); backward (dx, dw, dbias) "
          f"{t_lb:.3f} ms, {2 * wb / t_lb * 1e-9:.2f} TB/s (w read, dw written)")


def gradient_penalty_section(f0, f1, iters, warm):
    """The penalty pass of one WGAN_GP step on hat = mix(f0, f1): forward, first backward, second-order pass."""
    from vfi_amd import ops
    from vfi_amd.adacof.losses import adversarial, discriminator
    torch.manual_seed(0)
    net = discriminator.Discriminator(types.SimpleNamespace(patch_size=f0.shape[2], gradient_penalty=True), 'WGAN_GP').to(f0.device)
    hat = ops.gp_mix(f0, f1, torch.rand_like(f0))
    params = [p.detach() for p in net._node_params()]

    def whole():
        net.zero_grad(set_to_none=True)
        adversarial.gradient_penalty(net.input_gradient(hat)).backward()
    t_f = timed(lambda: discriminator._walk_forward(net, hat, params), iters, warm)
    t_g = timed(lambda: net.input_gradient(hat), iters, warm)
    t_w = timed(whole, iters, warm)
    print(f"  gradient penalty pass (HIP nodes): forward {t_f:.3f} ms, first backward {t_g - t_f:.3f} ms, second-order pass + "
          f"penalty kernels {t_w - t_g:.3f} ms, together {t_w:.3f} ms")
    net.eval()                                   # the plain-torch route of the same modules (no BatchNorm: the same function)

    def plain_whole():
        net.zero_grad(set_to_none=True)
        g = net.input_gradient(hat)
        (10 * g.view(g.size(0), -1).norm(2, dim=1).sub(1).pow(2).mean()).backward()
    t_p = timed(plain_whole, iters, warm)
    print(f"  torch/MIOpen create_graph double backward of the same layers, penalty and its backward: {t_p:.3f} ms")
    net.train()


def main(n=4, h=256, w=256, iters=10, warm=3, loss_string=None, vgg_weights=None, device_optimizer=False):
    dev = torch.device("cuda:0")
    sd = nets_cpu.adacofnet_random_state_dict(0)
    net = AdaCoFNet(types.SimpleNamespace(kernel_size=5, dilation=1, gpu_id=0)).to(dev)
    net.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    f0, f2 = (torch.rand((n, 3, h, w), generator=g).to(dev) for _ in range(2))
    grad = torch.randn((n, 3, h, w), generator=g).to(dev)

    def loss(out):
        return (out["frame1"] * grad).sum() + 0.01 * out["g_Spatial"] + 0.005 * out["g_Occlusion"]

    net.eval()
    with torch.no_grad():
        t_inf = timed(lambda: net(f0, f2), iters, warm)
    net.train(True)
    t_fwd = timed(lambda: net(f0, f2), iters, warm)

    def step():
        net.zero_grad(set_to_none=True)
        loss(net(f0, f2)).backward()
    t_step = timed(step, iters, warm)
    t_bwd = t_step - t_fwd

    _lib.PROFILE = rec = _lib.Recorder()
    agg = {}
    for _ in range(iters):
        out = loss(net(f0, f2))
        rec.rows.clear()
        out.backward()
        for label, a in rec.summary().items():
            b = agg.setdefault(label, dict(entry=a["entry"], kind=a["kind"], seconds=0.0, work=0.0))
            b["seconds"] += a["seconds"] / iters
            b["work"] += a["work"] / iters
        rec.rows.clear()
    _lib.PROFILE = None
    split = {"wgrad": 0.0, "dgrad": 0.0, "sampler": 0.0, "glue": 0.0}
    for a in agg.values():
        kind = {"vfi_conv2d_backward_weight": "wgrad", "vfi_conv2d_backward_data": "dgrad",
                "vfi_adacof_backward": "sampler"}.get(a["entry"], "glue")
        split[kind] += a["seconds"] * 1e3
    print(f"AdaCoFNet N={n} {h}x{w} kernel_size=5 dilation=1")
    print(f"  inference forward          {t_inf:8.3f} ms")
    print(f"  training forward           {t_fwd:8.3f} ms")
    print(f"  backward                   {t_bwd:8.3f} ms = {t_bwd / t_inf:.2f} x inference forward")
    print("    per-call events: " + ", ".join(f"{k} {v:.3f} ms" for k, v in split.items()))
    for label, a in sorted(agg.items()):
        if a["kind"] == "byte" and a["seconds"]:
            print(f"    {label:26s} {a['seconds'] * 1e3:7.3f} ms  {a['work'] / a['seconds'] / 1e12:5.2f} TB/s")

    # context only: the same KernelEstimation as torch layers (MIOpen), fp32
    import adacofnet_grad_ref as R
    P = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    x6 = torch.rand((n, 6, h, w), generator=g).to(dev) - 0.5
    gs = None

    def tfwd():
        return R.kernel_estimation(P, x6)

    def tstep():
        nonlocal gs
        for v in P.values():
            v.grad = None
        outs = tfwd()
        if gs is None:
            gs = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, gs)
    with torch.no_grad():
        t_tinf = timed(tfwd, iters, warm)
    t_tfwd = timed(tfwd, iters, warm)
    t_tstep = timed(tstep, iters, warm)
    net.get_kernel.train(True)
    kfwd = lambda: net.get_kernel.forward_x6(x6)

    def kstep():
        net.zero_grad(set_to_none=True)
        torch.autograd.backward(kfwd(), gs)
    t_kfwd = timed(kfwd, iters, warm)
    t_kstep = timed(kstep, iters, warm)
    print(f"  KernelEstimation alone: forward {t_kfwd:.3f} ms, backward {t_kstep - t_kfwd:.3f} ms")
    print(f"  torch/MIOpen KernelEstimation: inference {t_tinf:.3f} ms, forward {t_tfwd:.3f} ms, "
          f"backward {t_tstep - t_tfwd:.3f} ms")


    if loss_string:
        f1 = torch.rand((n, 3, h, w), generator=g).to(dev)
        loss_section(net, f0, f1, f2, loss_string, vgg_weights, iters, warm, device_optimizer)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--loss", default=None, help="also time the trainer's step with this loss string")
    ap.add_argument("--vgg-weights", default=None, help="torchvision vgg16 state dict (default: seeded weights)")
    ap.add_argument("--device-optimizer", action="store_true",
                    help="with --loss: time each trainer step again with the optimisers of vfi_amd.optim (DESIGN.md section 29)")
    a = ap.parse_args()
    main(loss_string=a.loss, vgg_weights=a.vgg_weights, device_optimizer=a.device_optimizer)
