"""Shared helpers of the glue / image kernel tests (test_glue_ops_gpu.py, test_image_ops_gpu.py).

Tolerance of a rounded operation: computed from the reference alone,
    tol = max(4 * max|ref32 - ref64|, 2**-23 * max|ref64|)
with ref64 the float64 reference and ref32 the same torch / numpy expression evaluated in float32 on the CPU.  ref32 shows
what one valid float32 evaluation loses on these inputs; the kernel may sum in another order or use a libm that differs
by 1-2 ulp (factor 4); the floor keeps the bound from collapsing where float32 happens to be exact.

Canaries: a slice an op writes lives in a buffer pre-filled with one NaN bit pattern; everything outside the slice must
hold that pattern bit for bit afterwards.  The same NaN surrounds a slice an op reads.
"""
import torch

SENTINEL = 0x7FC0BEEF          # a quiet NaN with a payload


def tol_of(ref32, ref64):
    ref32, ref64 = torch.as_tensor(ref32), torch.as_tensor(ref64)
    return max(4.0 * (ref32.double() - ref64.double()).abs().max().item(), 2.0 ** -23 * ref64.double().abs().max().item())


def assert_close(got, ref32, ref64, what):
    """max|got - ref64| <= tol_of(ref32, ref64); prints and returns (err, tol)."""
    ref64 = torch.as_tensor(ref64).double()
    got = torch.as_tensor(got).detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    tol = tol_of(ref32, ref64)
    assert torch.isfinite(got).all(), f"{what}: non-finite output (tol {tol:.3e})"
    err = (got - ref64).abs().max().item()
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, f"{what}: max|got - ref64| {err:.3e} > tol {tol:.3e}"
    return err, tol


def canary_buffer(numel, device):
    """Flat int32 buffer of `numel` sentinels; carve float32 views out of it with fview()."""
    return torch.full((numel,), SENTINEL, dtype=torch.int32, device=device)


def fview(flat, shape, offset=0, strides=None):
    """float32 view of `shape` into the canary buffer, starting `offset` floats in (dense unless `strides`)."""
    shape = tuple(shape)
    if strides is None:
        strides, s = [], 1
        for d in reversed(shape):
            strides.insert(0, s)
            s *= d
    return flat.view(torch.float32).as_strided(shape, tuple(strides), offset)


def assert_untouched(flat, *written, what=""):
    """Every element of the canary buffer outside the `written` views still holds the sentinel, bit for bit."""
    c = flat.clone()
    for v in written:
        c.as_strided(tuple(v.shape), tuple(v.stride()), v.storage_offset()).fill_(SENTINEL)
    bad = int((c != SENTINEL).sum().item())
    assert bad == 0, f"{what}: {bad} elements outside the written slice were modified"


def nan_wide(shape, device, offset=0):
    """(flat, wide): a float32 tensor of `shape` full of sentinel NaNs, starting `offset` floats into its allocation."""
    n = 1
    for d in shape:
        n *= d
    flat = canary_buffer(n + offset, device)
    return flat, fview(flat, shape, offset)
