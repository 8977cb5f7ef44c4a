#!/usr/bin/env python3
"""Generates tests/golden/adacof_grad_*.npz FROM THE REFERENCE ITSELF: the three gradients of
FunctionAdaCoF.backward (reference src/adacof/cupy_module/adacof.py:364-445).

Runs only in the build container (needs the reference checkout, which never travels to the GPU box).
Same method as the sampling fixtures of make_golden.py: the reference's own pure-Python specialiser
`cupy_kernel()` (adacof.py:261-299) turns each backward kernel (kernel_AdaCoF_updateGradWeight,
...updateGradAlpha, ...updateGradBeta, adacof.py:67-258) into plain C for the fixture's shapes; that text
is written to a TEMP dir (never into the repo), compiled with g++ together with a host loop that iterates
the launch grid, run on the seeded inputs and deleted again.  The fixtures hold data only.

    python tests/golden/make_golden_adacof_grad.py

All cases have C = 3: the reference's channel loop is hard-coded to c < 3 (adacof.py:86, :150, :215).
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _placeholders, adacof_inputs, save  # noqa: E402

_HOST_LOOP = r"""
#include <cstdlib>
struct dim3_ { int x, y, z; };
static thread_local dim3_ blockIdx, threadIdx;
static dim3_ blockDim = {512, 1, 1}, gridDim = {1, 1, 1};
#define __global__
%(KERNEL)s
extern "C" void run(int n, %(PARAMS)s) {
    gridDim.x = (n + 512 - 1) / 512;                       /* adacof.py:408, :424, :440 */
    for (int b = 0; b < gridDim.x; ++b)
        for (int t = 0; t < blockDim.x; ++t) {
            blockIdx.x = b; threadIdx.x = t;
            %(NAME)s(n, %(ARGS)s);
        }
}
"""

# kernel name -> (tensor arguments in launch order, output tensor); adacof.py:400-443
KERNELS = {
    "kernel_AdaCoF_updateGradWeight": (("gradLoss", "input", "offset_i", "offset_j"), "gradWeight"),
    "kernel_AdaCoF_updateGradAlpha": (("gradLoss", "input", "weight", "offset_i", "offset_j"), "gradOffset_i"),
    "kernel_AdaCoF_updateGradBeta": (("gradLoss", "input", "weight", "offset_i", "offset_j"), "gradOffset_j"),
}

CASES = {  # tag: (n, c, h, w, f, dilation, big offsets)
    "f5d1": (1, 3, 31, 45, 5, 1, True),
    "f5d1_b2": (2, 3, 18, 32, 5, 1, False),
    "f11d2": (1, 3, 16, 20, 11, 2, True),
    "f3d1": (1, 3, 21, 27, 3, 1, True),
}


def _run_kernel(ref, name, f, dil, arrays):
    ins, out_name = KERNELS[name]
    out = np.zeros_like(arrays["offset_i"])
    tens = {k: torch.from_numpy(arrays[k]) for k in ins}
    tens[out_name] = torch.from_numpy(out)
    text = ref.cupy_kernel(name, f, dil, tens).replace('extern "C" __global__', "static")
    names = ins + (out_name,)
    params = ", ".join(("float* " if k == out_name else "const float* ") + k for k in names)
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "k.cpp")
        with open(src, "w") as fh:
            fh.write(_HOST_LOOP % {"KERNEL": text, "PARAMS": params, "NAME": name, "ARGS": ", ".join(names)})
        so = os.path.join(td, "k.so")
        # plain fp32 evaluation (no fma contraction), as for the sampling fixtures
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, src])
        lib = ctypes.CDLL(so)
        fp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        lib.run(ctypes.c_int(out.size), *[fp(arrays[k]) for k in ins], fp(out))
    return out


def main():
    _placeholders()
    from src.adacof.cupy_module import adacof as ref  # reference module
    for tag, (n, c, h, w, f, dil, big) in CASES.items():
        seed = 1000 + len(tag) * 7 + f
        inp, wgt, a, b = adacof_inputs(seed, n, c, h, w, f, dil, big)
        g = np.random.default_rng(seed + 1).standard_normal((n, c, h, w)).astype(np.float32)
        arrays = dict(gradLoss=g, input=inp, weight=wgt, offset_i=a, offset_j=b)
        gw = _run_kernel(ref, "kernel_AdaCoF_updateGradWeight", f, dil, arrays)
        ga = _run_kernel(ref, "kernel_AdaCoF_updateGradAlpha", f, dil, arrays)
        gb = _run_kernel(ref, "kernel_AdaCoF_updateGradBeta", f, dil, arrays)
        save("adacof_grad_" + tag, input=inp, weight=wgt, offset_i=a, offset_j=b, dilation=dil,
             grad_output=g, grad_weight=gw, grad_offset_i=ga, grad_offset_j=gb)


if __name__ == "__main__":
    main()
