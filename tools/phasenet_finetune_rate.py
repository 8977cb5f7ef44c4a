#!/usr/bin/env python3
"""Cost of fine-tuning the whole PhaseNet on a 1080x1920 Lab frame pair (N = 3 colours): the inference
forward of the coarse-to-fine walk, the same forward as an autograd graph, and the HIP backward of one full step, at full m
and at m = 4; and the head adjoint at the finest level's shape, vfi_phasenet_predict_backward against the five-launch
composition of the section-14 entry points.  Per-call HIP events.

--batch-stats: the same step with BatchNorm on the batch's statistics (the forward without a graph is
then that route under no_grad, running statistics updated), and the three batch-statistics kernels alone at the finest level's
shape (3 x 64 x 1080 x 1920) with their algorithmic bytes.

--num-img 3 | 4: the same measurements for the pyramid-domain fusion networks: the head adjoint is
vfi_phasenet_predict_n_backward against the composition over vfi_phasenet_emit_n_backward, the step runs
PhaseNetCore(num_img).fine_tune(fusion=True) on 3 * num_img images.  The default, 2, prints what it always did.

--batch B (with --size H W, default 1080 1920): one training step of architecture.PhaseNet on a batch of B samples instead
(DESIGN.md section 21): img_batch of (num_img + 1) * 3 * B channel-images through one Pyramid.filter call, the walk on 3 * B
planes, get_loss, backward.  The default, 1, prints what it always did."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
import phasenet_fusion_ref as FR  # noqa: E402
import phasenet_walk_ref as W  # noqa: E402
from vfi_amd import ops  # noqa: E402
from vfi_amd.phase_net import grad as G  # noqa: E402
from vfi_amd.phase_net.core import PhaseNetCore  # noqa: E402
from vfi_amd.train.loss import l1_loss, phase_term  # noqa: E402
from vfi_amd.train.pyramid import Pyramid  # noqa: E402
from vfi_amd.train.utils import calc_pyr_height  # noqa: E402


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


def head(h, w, n=3, iters=10, warm=3):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g).to(dev)
    fp = r(n, 72, h, w)
    fp[:, 64:] = torch.tanh(fp[:, 64:])
    f, pred, amp, mx, wp = fp[:, :64], fp[:, 64:], torch.rand((n, 8, h, w), generator=g).to(dev), torch.ones(n, device=dev), r(8, 64, 1, 1) / 8
    gp, ga, gc = r(n * 4, 1, h, w), r(n * 4, 1, h, w), r(n, 8, h, w)
    t_new = timed(lambda: ops.phasenet_predict_backward(f, pred, amp, mx, wp, gp, ga, gc), iters, warm)
    t_old = timed(lambda: G.head_backward_composed(f, pred, amp, mx, wp, gp, ga, gc), iters, warm)
    planes = 64 + 8 + 8 + 16 + 64
    print(f"head adjoint, N={n} {h}x{w}: one pass {t_new:.3f} ms ({4e-9 * n * h * w * planes / (t_new * 1e-3):.0f} GB/s of {planes} planes), "
          f"five-launch composition {t_old:.3f} ms, ratio {t_old / t_new:.2f}")


def head_n(h, w, num_img, n=3, iters=10, warm=3):
    """head() for three and four input images, on the walk's own layouts: [feature | pred] and the whole amplitude block."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g).to(dev)
    pb = FR.pred_channels(num_img)[1]
    fp = r(n, 64 + pb, h, w)
    fp[:, 64:] = torch.tanh(fp[:, 64:])
    f, pred, amp, mx, wp = fp[:, :64], fp[:, 64:], torch.rand((n, 4 * num_img, h, w), generator=g).to(dev), torch.ones(n, device=dev), r(pb, 64, 1, 1) / 8
    gp, ga, gc = r(n * 4, 1, h, w), r(n * 4, 1, h, w), r(n, pb, h, w)
    t_new = timed(lambda: ops.phasenet_predict_n_backward(f, pred, amp, mx, wp, num_img, gp, ga, gc), iters, warm)
    t_old = timed(lambda: G.head_backward_composed(f, pred, amp, mx, wp, gp, ga, gc, num_img=num_img), iters, warm)
    planes = 64 + pb + pb + 4 + (20 if num_img == 3 else 12) + 64
    print(f"head adjoint, num_img={num_img} N={n} {h}x{w}: one pass {t_new:.3f} ms ({4e-9 * n * h * w * planes / (t_new * 1e-3):.0f} GB/s of {planes} planes), "
          f"composition {t_old:.3f} ms, ratio {t_old / t_new:.2f}")


def bn_kernels(h, w, n=3, c=64, iters=10, warm=3):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    y = torch.randn((n, c, h, w), device=dev) * 1.5 + 0.5
    g_t = torch.randn((n, c, h, w), device=dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    mean, var = ops.bn_stats(y)
    t = ops.bn_act_forward(y, mean, var, gamma, beta, 1e-5, "elu")
    planes = 4e-9 * n * c * h * w
    rows = [("vfi_bn_stats", 1, lambda: ops.bn_stats(y)),
            ("vfi_bn_act_forward (elu)", 2, lambda: ops.bn_act_forward(y, mean, var, gamma, beta, 1e-5, "elu", out=t)),
            ("vfi_bn_act_backward, reductions only", 3, lambda: ops.bn_act_backward(g_t, t, y, mean, var, gamma, 1e-5, "elu", need_data=False)),
            ("vfi_bn_act_backward, in place", 7, lambda: ops.bn_act_backward(g_t, t, y, mean, var, gamma, 1e-5, "elu", out=g_t))]
    print(f"batch-statistics kernels, N={n} C={c} {h}x{w} ({planes:.2f} GB per tensor)")
    for name, passes, fn in rows:
        ms = timed(fn, iters, warm)
        print(f"  {name:40s} {ms:7.3f} ms  {passes * planes / (ms * 1e-3):6.0f} GB/s of {passes} tensor passes")


def step(h, w, m, n=3, iters=3, warm=1, batch_stats=False, num_img=2):
    dev = torch.device("cuda:0")
    height = calc_pyr_height(torch.empty(1, h, w))
    pyr = Pyramid(height=height, nbands=4, scale_factor=W.S2, device=dev)
    imgs = torch.rand((num_img * n, h, w), generator=torch.Generator().manual_seed(1)).to(dev)
    if num_img == 2:
        core = PhaseNetCore(height, dev).fine_tune(batch_stats=batch_stats)
        core.load_state_dict(W.net_state(0))
        vals, bufs = pyr.filter(imgs, concat_frames=2, phase_scale=1.0 / math.pi)
    else:
        core = PhaseNetCore(height, dev, num_img=num_img).fine_tune(batch_stats=batch_stats, fusion=True)
        core.load_state_dict(FR.net_state(0, num_img))
        vals, bufs = pyr.filter(imgs, concat_frames=num_img, phase_scale=1.0 / math.pi, pred_channels=core.pred_channels)
    nv = core.normalize_vals(vals, concat=bufs)
    with torch.no_grad():
        t_inf = timed(lambda: core(nv, m), iters, warm)
        out = core(nv, m)
    tp = [p.clone() + 0.3 if torch.is_tensor(p) else p for p in out.phase]
    ta = [a.clone() + 0.1 if torch.is_tensor(a) else a for a in out.amplitude]
    tl = out.low_level.clone() + 0.1
    del out

    def loss():
        v = core(nv, m)
        total = l1_loss(v.low_level, tl)
        for p, a, pt, at in zip(v.phase, v.amplitude, tp, ta):
            if torch.is_tensor(p):
                total = total + 0.005 * phase_term(p, pt, 4) + l1_loss(a, at)
        return total
    t_fwd = timed(loss, iters, warm)

    def full():
        core.zero_grad(set_to_none=True)
        loss().backward()
    t_step = timed(full, iters, warm)
    t_bwd = t_step - t_fwd
    print(f"PhaseNet walk, N={n} {h}x{w}, height {height}, m = {m if m is not None else height - 2}" +
          (", batch statistics" if batch_stats else "") + (f", num_img = {num_img}" if num_img != 2 else ""))
    print(f"  {'forward without a graph' if batch_stats else 'inference forward'      :26s} {t_inf:8.3f} ms")
    print(f"  forward as a graph + loss  {t_fwd:8.3f} ms")
    print(f"  backward                   {t_bwd:8.3f} ms = {t_bwd / t_inf:.2f} x that forward")


def batch_step(h, w, b, m, iters=5, warm=2, batch_stats=False, num_img=2):
    """One step of reference src/train/trainer.py:107-134 on B samples: architecture.PhaseNet.forward(img_batch, m=m), get_loss,
    backward; and its parts that run without a graph."""
    from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
    from vfi_amd.train.loss import get_loss
    dev = torch.device("cuda:0")
    height = calc_pyr_height(torch.empty(1, h, w))
    net = ArchPhaseNet(height, dev, num_img=num_img).fine_tune(batch_stats=batch_stats, fusion=num_img != 2)
    net.core.load_state_dict(W.net_state(0) if num_img == 2 else FR.net_state(0, num_img))
    n = (num_img + 1) * 3 * b
    img_batch = torch.rand((n, h, w), generator=torch.Generator().manual_seed(1)).to(dev)
    target = img_batch[-3 * b:]
    m_ = height - 2 if m is None else m
    with torch.no_grad():
        t_ana = timed(lambda: net.pyr.filter(img_batch), iters, warm)
        vals = net.pyr.filter(img_batch)
        t_syn = timed(lambda: net.pyr.inv_filter(vals), iters, warm)
        del vals
        t_inf = timed(lambda: net(img_batch, m=m_), iters, warm)

    def full():
        net.core.zero_grad(set_to_none=True)
        prediction, vals_pred, vals_target = net(img_batch, m=m_)
        get_loss(vals_pred, vals_target, prediction, target, net.pyr)[0].backward()
    t_step = timed(full, iters, warm)
    print(f"PhaseNet training step, batch {b} ({n} channel-images, {-(-n // 16)} pyramid slices) {h}x{w}, height {height}, m = {m_}" +
          (", batch statistics" if batch_stats else "") + (f", num_img = {num_img}" if num_img != 2 else ""))
    print(f"  analysis of the batch       {t_ana:8.3f} ms")
    print(f"  synthesis of {n:3d} images     {t_syn:8.3f} ms")
    print(f"  forward without a graph     {t_inf:8.3f} ms")
    print(f"  forward + loss + backward   {t_step:8.3f} ms = {t_step / b:.3f} ms per sample")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch-stats", action="store_true", help="BatchNorm on batch statistics (DESIGN.md section 17)")
    ap.add_argument("--num-img", type=int, choices=(2, 3, 4), default=2, help="input images of the network (DESIGN.md section 20)")
    ap.add_argument("--batch", type=int, default=1, help="samples per step (DESIGN.md section 21); above 1: architecture.PhaseNet's step on the batch")
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"), help="frame size of the --batch step")
    args = ap.parse_args()
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    if args.batch > 1:
        for m in (None, 4):
            batch_step(args.size[0], args.size[1], args.batch, m, batch_stats=args.batch_stats, num_img=args.num_img)
            torch.cuda.empty_cache()
        return
    if args.batch_stats:
        bn_kernels(1080, 1920)
    elif args.num_img == 2:
        head(1080, 1920)
    else:
        head_n(1080, 1920, args.num_img)
    torch.cuda.empty_cache()
    for m in (None, 4):
        step(1080, 1920, m, batch_stats=args.batch_stats, num_img=args.num_img)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
