#!/usr/bin/env python3
"""FusionNet training step cost at batch 16, 256x256, uncertainty_maps = 0 (the configuration src/fusion_net/train.py
trains): inference forward, forward with the activations kept for the backward, the HIP backward split into weight
gradients, input gradients and glue (per-call HIP events), and the weight-gradient kernel's fraction of the fp32 MFMA
peak (155 TF) on the 5x5 layers.  The same network in torch (MIOpen convolutions) on the same GPU is timed for context."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd")]
from oracle import nets_cpu  # noqa: E402
from vfi_amd import _lib  # noqa: E402
from vfi_amd.fusion_net.fusion_net import FusionNet  # noqa: E402

PEAK_FP32_MFMA = 155e12


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


def main(n=16, h=256, w=256, iters=10, warm=3):
    dev = torch.device("cuda:0")
    sd = nets_cpu.fusionnet_random_state_dict(0, uncertainty_maps=0)
    net = FusionNet(uncertainty_maps=0).to(dev)
    net.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    ins = [torch.rand((n, c, h, w), generator=g).to(dev) for c in (3, 3, 3, 6)] + [None]
    grad = torch.randn((n, 3, h, w), generator=g).to(dev)

    net.eval()
    with torch.no_grad():
        t_inf = timed(lambda: net(*ins), iters, warm)
    net.train(True)
    t_fwd = timed(lambda: net(*ins), iters, warm)

    def fwd_bwd():
        net.zero_grad(set_to_none=True)
        net(*ins).backward(grad)
    t_step = timed(fwd_bwd, iters, warm)
    t_bwd = t_step - t_fwd

    outs = []
    _lib.PROFILE = rec = _lib.Recorder()
    for _ in range(iters):
        out = net(*ins)
        rec.rows.clear()
        out.backward(grad)
        outs.append(rec.summary())
    _lib.PROFILE = None
    agg = {}
    for s in outs:
        for label, a in s.items():
            b = agg.setdefault(label, dict(entry=a["entry"], seconds=0.0, work=0.0, calls=0))
            b["seconds"] += a["seconds"] / iters
            b["work"] += a["work"] / iters
            b["calls"] += a["calls"]
    split = {"wgrad": 0.0, "dgrad": 0.0, "glue": 0.0}
    for label, a in agg.items():
        kind = "wgrad" if a["entry"] == "vfi_conv2d_backward_weight" else (
            "dgrad" if a["entry"] == "vfi_conv2d_backward_data" else "glue")
        split[kind] += a["seconds"] * 1e3
    print(f"FusionNet N={n} {h}x{w} uncertainty_maps=0")
    print(f"  inference forward        {t_inf:8.3f} ms")
    print(f"  forward, activations kept {t_fwd:7.3f} ms")
    print(f"  backward                 {t_bwd:8.3f} ms = {t_bwd / t_inf:.2f} x inference forward")
    print(f"    per-call events: wgrad {split['wgrad']:.3f} ms, dgrad {split['dgrad']:.3f} ms, glue {split['glue']:.3f} ms")
    for label, a in sorted(agg.items()):
        if a["entry"] == "vfi_conv2d_backward_weight":
            tf = a["work"] / a["seconds"] if a["seconds"] else 0.0
            print(f"    {label:28s} {a['seconds'] * 1e3:7.3f} ms  {tf / 1e12:6.1f} TF = {100 * tf / PEAK_FP32_MFMA:5.1f} % of fp32 MFMA peak")
    k5 = [(a["work"], a["seconds"]) for label, a in agg.items() if label == "conv_wgrad_kernel<5>"]
    if k5:
        print(f"  wgrad on the 5x5 layers: {100 * k5[0][0] / k5[0][1] / PEAK_FP32_MFMA:.1f} % of fp32 MFMA peak")

    # context only: the same network in torch (MIOpen), fp32
    P = {k: v.to(dev).requires_grad_(not k.startswith("net.")) for k, v in sd.items()}
    with torch.no_grad():
        t_tinf = timed(lambda: nets_cpu.fusionnet_forward(P, *ins, 0), iters, warm)

    def tstep():
        for v in P.values():
            v.grad = None
        nets_cpu.fusionnet_forward(P, *ins, 0).backward(grad)
    t_tfwd = timed(lambda: nets_cpu.fusionnet_forward(P, *ins, 0), iters, warm)
    t_tstep = timed(tstep, iters, warm)
    print(f"  torch/MIOpen reference: inference {t_tinf:.3f} ms, forward {t_tfwd:.3f} ms, "
          f"backward {t_tstep - t_tfwd:.3f} ms")


if __name__ == "__main__":
    main()
