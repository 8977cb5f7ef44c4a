#!/usr/bin/env python3
"""Training cost of one 3x3 PhaseNet block (batch 3, 88 -> 64 -> 64 -> 8) at the sizes of PhaseNet's
two finest levels of a 1080p frame: the inference forward (three launches), the forward as an autograd node, and the HIP
backward split by per-call HIP events into weight gradients, data gradients and glue (activation backward, add)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd"), os.path.join(ROOT, "tests")]
import phasenet_grad_ref as R  # noqa: E402
from vfi_amd import _lib  # noqa: E402
from vfi_amd.phase_net.phase_net import PhaseNetBlock  # noqa: E402


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


def measure(h, w, n=3, iters=5, warm=2):
    dev = torch.device("cuda:0")
    blk = PhaseNetBlock(88, 64, 8, (3, 3)).to(dev)
    blk.load_state_dict(R.block_state(0, 88, 8, 3))
    g = torch.Generator().manual_seed(0)
    x = torch.randn((n, 88, h, w), generator=g).to(dev)
    gf, gc = torch.randn((n, 64, h, w), generator=g).to(dev), torch.randn((n, 8, h, w), generator=g).to(dev)
    with torch.no_grad():
        t_inf = timed(lambda: blk(x), iters, warm)
    t_fwd = timed(lambda: blk(x), iters, warm)

    def step():
        blk.zero_grad(set_to_none=True)
        torch.autograd.backward(blk(x), (gf, gc))
    t_step = timed(step, iters, warm)
    t_bwd = t_step - t_fwd

    _lib.PROFILE = rec = _lib.Recorder()
    split = {"wgrad": 0.0, "dgrad": 0.0, "glue": 0.0}
    for _ in range(iters):
        outs = blk(x)
        rec.rows.clear()
        torch.autograd.backward(outs, (gf, gc))
        for a in rec.summary().values():
            kind = {"vfi_conv2d_backward_weight": "wgrad", "vfi_conv2d_backward_data": "dgrad"}.get(a["entry"], "glue")
            split[kind] += a["seconds"] * 1e3 / iters
        rec.rows.clear()
    _lib.PROFILE = None
    print(f"PhaseNet 3x3 block 88->64->64->8, N={n} {h}x{w}")
    print(f"  inference forward          {t_inf:8.3f} ms")
    print(f"  forward as a node          {t_fwd:8.3f} ms")
    print(f"  backward                   {t_bwd:8.3f} ms = {t_bwd / t_inf:.2f} x inference forward")
    print("    per-call events: " + ", ".join(f"{k} {v:.3f} ms" for k, v in split.items()))


def main():
    for h, w in ((1080, 1920), (764, 1358)):
        measure(h, w)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
