#!/usr/bin/env python3
"""AdaCoFNet training step cost at the reference's training shape (batch 4, 256x256, kernel_size 5, dilation 1;
src/adacof/train.py): inference forward, training forward (activations kept), the HIP backward split by per-call HIP events
into weight gradients, input gradients, sampler and glue, and each new streaming kernel's effective TB/s (to be read
against profiles/r04_hbm_rates.txt: vfi_resize_bilinear 4.1-4.5 TB/s, plain copy 4.75-5.3 TB/s).  The same
KernelEstimation as plain torch.nn layers (MIOpen convolutions) on the same GPU is timed for context."""
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


def main(n=4, h=256, w=256, iters=10, warm=3):
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


if __name__ == "__main__":
    main()
