"""CPU checks of the AdaCoF backward: the C entry point exists and rejects bad calls before touching a device, and
the reference-generated gradient fixtures agree with an independent float64 restatement of the forward (which pins
both the fixtures and the restatement the GPU tests compare against)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from adacof_grad_ref import restated_grads
from conftest import GOLDEN

import vfi_amd
from vfi_amd import _lib

GRAD_CASES = sorted(glob.glob(os.path.join(GOLDEN, "adacof_grad_*.npz")))


def test_backward_is_declared_exported_and_bound():
    assert "vfi_adacof_backward" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(vfi_amd.library_path()), "vfi_adacof_backward")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "vfi_hip.h")).read()
    assert "int vfi_adacof_backward(" in header


def test_backward_argument_validation_needs_no_gpu():
    h = vfi_amd.lib()
    one = ctypes.c_void_p(16)
    # null required pointers
    assert h.vfi_adacof_backward(None, None, None, None, None, one, one, one, 1, 3, 8, 8, 4, 4, 5, 1, None) == -1
    assert b"null pointer" in h.vfi_last_error()
    # weight is required when an offset gradient is requested ...
    assert h.vfi_adacof_backward(one, one, None, one, one, None, one, None, 1, 3, 8, 8, 4, 4, 5, 1, None) == -1
    # ... and no gradient at all is an error
    assert h.vfi_adacof_backward(one, one, one, one, one, None, None, None, 1, 3, 8, 8, 4, 4, 5, 1, None) == -1
    assert b"no gradient" in h.vfi_last_error()
    # non-positive sizes
    assert h.vfi_adacof_backward(one, one, one, one, one, one, one, one, 1, 0, 8, 8, 4, 4, 5, 1, None) == -1
    assert h.vfi_adacof_backward(one, one, one, one, one, one, one, one, 1, 3, 8, 8, 4, 4, 5, 0, None) == -1
    assert b"non-positive" in h.vfi_last_error()
    # adacof.py:326-327 shape relation
    assert h.vfi_adacof_backward(one, one, one, one, one, one, one, one, 1, 3, 9, 8, 4, 4, 5, 1, None) == -2
    assert b"does not match" in h.vfi_last_error()
    # too large
    assert h.vfi_adacof_backward(one, one, one, one, one, one, one, one,
                                 1, 3, 65540, 65540, 65536, 65536, 5, 1, None) == -4   # VFI_ERR_UNSUPPORTED
    assert b"too large" in h.vfi_last_error()


def test_cpu_tensors_are_refused_on_backward():
    from vfi_amd.adacof.cupy_module.adacof import FunctionAdaCoF
    x = torch.zeros(1, 3, 8, 8)
    w = torch.zeros(1, 25, 4, 4, requires_grad=True)
    with pytest.raises(NotImplementedError):   # the forward has no CPU path (reference adacof.py:356-357)
        FunctionAdaCoF.apply(x, w, w, w, 1)


@pytest.mark.parametrize("path", GRAD_CASES, ids=[os.path.basename(p)[12:-4] for p in GRAD_CASES])
def test_fixture_gradients_match_float64_restatement(path):
    g = np.load(path)
    got = restated_grads(g["input"], g["weight"], g["offset_i"], g["offset_j"], int(g["dilation"]), g["grad_output"])
    # fp32 left-to-right (reference) against fp64: a few ulp of sums of <= 3 * F*F terms of magnitude <= ~10
    for name, r in zip(("grad_weight", "grad_offset_i", "grad_offset_j"), got):
        np.testing.assert_allclose(g[name], r.numpy(), rtol=0, atol=1e-4, err_msg=name)


def test_fixtures_cover_the_edge_cases():
    g = np.load(os.path.join(GOLDEN, "adacof_grad_f5d1.npz"))
    a, b = g["offset_i"], g["offset_j"]
    assert (np.abs(a) == 1000).any() and (np.abs(b) == 1000).any()            # clamps on every side
    assert ((a < 0) & (a != np.trunc(a))).any()                                # negative fractions
    assert (np.signbit(a) & (a == 0)).any() and ((~np.signbit(b)) & (b == 0)).any()   # -0.0 / +0.0
    assert ((a == np.round(a)) & (a != 0)).any()                               # exact integers
    assert g["input"].shape[1] == 3
