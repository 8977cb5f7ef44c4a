"""The WGAN_GP term's entry points on the MI355X, through the C ABI: vfi_leaky_mask and vfi_gp_mix
bit for bit against the float32 expressions, vfi_grad_penalty_forward / _backward against float64.

As tests/test_discriminator_ops_gpu.py: every output is a view into a buffer of NaN sentinels that must stay untouched around
it; operands start on a 16-byte boundary and one float past one, and their batch strides are padded (by 4 floats, and by 3).

Bounds.
* leaky_mask, gp_mix: the bits of `where(s > 0, a, a * slope)` and of `fake.mul(1 - eps) + real.mul(eps)` in float32 on the
  CPU (int32 views are compared, so -0 and +0 differ).
* Penalty forward: norms[b]^2 within 1e-5 relative of the float64 sum of squares -- section 27's linear-forward bound on a
  sum of non-negative terms (an fp32 chain-and-tree sum loses at most its length times 2^-24 of the sum of the absolute
  terms; here those are the terms).  The value against weight / B * sum (norms[b] - 1)^2 evaluated in float64 FROM THE KERNEL'S
  OWN float32 norms: per term one rounding of the difference (exact for a norm in [0.5, 2]) and one of the square, the tree
  over at most 9 terms, the rounding of weight / B and the last product -- under 16 * 2^-24 relative.
* Penalty backward: 4 units in the last place of the float64 formula evaluated from the kernel's own float32 norms (the
  row's factor is formed in double and rounded once, then one product per element)."""
import numpy as np
import pytest
import torch

from glue_ref import assert_untouched
from test_discriminator_ops_gpu import LAYOUTS, _call, _held
from vfi_amd import _lib, ops

pytestmark = pytest.mark.gpu

COUNTS = [1, 7, 8, 255, 256, 257, 4099]
EPS24 = 2.0 ** -24
DENORMAL = float(np.float32(1e-41))
SPECIAL = [0.0, -0.0, DENORMAL, -DENORMAL, float(np.finfo(np.float32).tiny), -float(np.finfo(np.float32).tiny)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _values(shape, g):
    """randn with +0, -0, denormals and the smallest normals scattered over the leading elements"""
    t = torch.randn(shape, generator=g)
    flat = t.view(-1)
    k = min(flat.numel(), len(SPECIAL))
    idx = torch.randperm(flat.numel(), generator=g)[:k]
    flat[idx] = torch.tensor(SPECIAL[:k])
    return t


# ---- leaky_mask -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", [1, 3])
def test_leaky_mask_bits(n, count, device):
    g = torch.Generator().manual_seed(n * 10000 + count)
    a0, s0 = _values((n, count), g), _values((n, count), g)
    for slope in (0.2, 1.0):
        sl = np.float32(slope)
        for name, off, pad in LAYOUTS:
            for alias in ("none", "s is a", "out is a", "all three"):
                s_src = a0 if alias in ("s is a", "all three") else s0
                want = torch.from_numpy(np.where(s_src.numpy() > 0, a0.numpy(), a0.numpy() * sl).astype(np.float32))
                flat_a, a = _held((n, count), device, off, pad, a0)
                s = a if alias in ("s is a", "all three") else _held((n, count), device, off, pad, s0)[1]
                if alias in ("out is a", "all three"):
                    flat, out = flat_a, a
                else:
                    flat, out = _held((n, count), device, off, pad)
                _call("vfi_leaky_mask", a.data_ptr(), a.stride(0), s.data_ptr(), s.stride(0), out.data_ptr(), out.stride(0), n, count,
                      slope, _lib.stream_ptr())
                assert_untouched(flat, out, what="vfi_leaky_mask")
                assert torch.equal(_bits(out), _bits(want)), (slope, name, alias)
                if out is not a:
                    assert torch.equal(_bits(a), _bits(a0)), "the operand was written"
    one = torch.zeros(4, device=device)
    h = _lib.lib()
    for slope in (0.0, -0.2):
        assert h.vfi_leaky_mask(one.data_ptr(), 4, one.data_ptr(), 4, one.data_ptr(), 4, 1, 4, slope, _lib.stream_ptr()) == -1
    assert not bool(one.any())


def test_leaky_mask_through_ops(device):
    g = torch.Generator().manual_seed(1)
    wide = torch.randn((2, 9, 5, 6), generator=g).to(device)
    a, s = wide[:, 1:4], wide[:, 4:7]                                   # channel slices
    want = torch.where(s > 0, a, a * 0.2)
    assert torch.equal(ops.leaky_mask(a, s, 0.2), want)
    y = a.clone()
    assert ops.leaky_mask(y, y, 0.2, out=y) is y and torch.equal(y, torch.nn.functional.leaky_relu(a, 0.2))
    m = torch.randn((3, 70), generator=g).to(device)
    assert torch.equal(ops.leaky_mask(m, m, 0.2), torch.nn.functional.leaky_relu(m, 0.2))
    with pytest.raises(_lib.VfiLibraryError):
        ops.leaky_mask(a, s[:, :2], 0.2)
    with pytest.raises(_lib.VfiLibraryError):
        ops.leaky_mask(a, s, 0.0)


# ---- gp_mix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", [1, 3])
def test_gp_mix_bits(n, count, device):
    g = torch.Generator().manual_seed(n * 777 + count)
    fake, real = _values((n, count), g), torch.rand((n, count), generator=g)
    eps = torch.rand((n, count), generator=g)
    edge = [0.0, float(np.nextafter(np.float32(1), np.float32(0))), 1.0 - 2.0 ** -23, float(np.float32(2.0 ** -25)), 0.5]
    flat_e = eps.view(-1)
    k = min(flat_e.numel(), len(edge))
    flat_e[torch.randperm(flat_e.numel(), generator=g)[:k]] = torch.tensor(edge[:k])
    want = fake.mul(1 - eps) + real.mul(eps)
    for name, off, pad in LAYOUTS:
        f, r, e = (_held((n, count), device, off, pad, t)[1] for t in (fake, real, eps))
        flat, hat = _held((n, count), device, off, pad)
        _call("vfi_gp_mix", f.data_ptr(), f.stride(0), r.data_ptr(), r.stride(0), e.data_ptr(), e.stride(0), hat.data_ptr(),
              hat.stride(0), n, count, _lib.stream_ptr())
        assert_untouched(flat, hat, what="vfi_gp_mix")
        assert torch.equal(_bits(hat), _bits(want)), name
    if count == 4099:
        x = fake.view(n, 1, 1, count).to(device)
        assert torch.equal(_bits(ops.gp_mix(x, real.view_as(x).to(device), eps.view_as(x).to(device))), _bits(want.view_as(x)))


# ---- the penalty ----------------------------------------------------------------------------------------------------------
N_SIZES = [1, 3, 255, 256, 257, 768, 3072, 196608]
WEIGHT = 10.0


def _rows(b, n, g, zero_row=None, unit_row=None):
    x = torch.randn((b, n), generator=g, dtype=torch.float64)
    x *= ((0.5 + 0.4 * torch.arange(b, dtype=torch.float64)) / x.norm(dim=1)).view(-1, 1)      # norms 0.5, 0.9, 1.3, ...
    if zero_row is not None and zero_row < b:
        x[zero_row] = 0.0
    if unit_row is not None and unit_row < b:
        x[unit_row] /= x[unit_row].norm()                                                       # next to 1 after rounding
    return x.float()


def _forward(g_dev, device):
    b, n = g_dev.shape
    flat_n, norms = _held((b,), device, 0, 0)
    flat_v, value = _held((1,), device, 0, 0)
    _call("vfi_grad_penalty_forward", g_dev.data_ptr(), g_dev.stride(0), norms.data_ptr(), value.data_ptr(), b, n,
          WEIGHT, _lib.stream_ptr())
    assert_untouched(flat_n, norms, what="vfi_grad_penalty_forward norms")
    assert_untouched(flat_v, value, what="vfi_grad_penalty_forward value")
    return norms, value


@pytest.mark.parametrize("n", N_SIZES)
def test_grad_penalty_forward_against_float64(n, device):
    worst = [0.0, 0.0]
    for b in (1, 2, 3, 4, 9):
        g0 = _rows(b, n, torch.Generator().manual_seed(n * 13 + b))
        sq64 = g0.double().pow(2).sum(1)
        for name, off, pad in LAYOUTS:
            gd = _held((b, n), device, off, pad, g0)[1]
            norms, value = _forward(gd, device)
            got = norms.double().cpu()
            r_sq = float(((got * got - sq64).abs() / sq64).max())
            want_v = WEIGHT / b * float(((got - 1.0) ** 2).sum())
            r_v = abs(float(value) - want_v) / want_v
            worst = [max(worst[0], r_sq), max(worst[1], r_v)]
            assert bool(torch.isfinite(norms).all()) and r_sq <= 1e-5, (b, name, r_sq)
            assert r_v <= 16 * EPS24, (b, name, r_v)
            norms2, value2 = _forward(gd, device)
            assert torch.equal(norms, norms2) and torch.equal(value, value2), "two runs differ"
    print(f"grad_penalty_forward n={n}: worst norm^2 err {worst[0]:.2e} relative, value from its norms {worst[1] / EPS24:.2f} x 2^-24")


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 3072, 196608])
def test_grad_penalty_backward_against_float64(n, device):
    worst = 0.0
    for b in (1, 4, 9):
        g0 = _rows(b, n, torch.Generator().manual_seed(n * 17 + b), zero_row=1, unit_row=2)
        up = torch.tensor(0.37, device=device)
        for name, off, pad in LAYOUTS:
            gd = _held((b, n), device, off, pad, g0)[1]
            norms, _ = _forward(gd, device)
            flat, out = _held((b, n), device, off, pad)
            _call("vfi_grad_penalty_backward", gd.data_ptr(), gd.stride(0), norms.data_ptr(), up.data_ptr(),
                  out.data_ptr(), out.stride(0), b, n, WEIGHT, _lib.stream_ptr())
            assert_untouched(flat, out, what="vfi_grad_penalty_backward")
            nk = norms.double().cpu()
            coef = torch.where(nk == 0, torch.zeros_like(nk), float(up.double()) * WEIGHT * 2.0 * (nk - 1.0) / (b * nk.clamp_min(1e-300)))
            want = coef.view(-1, 1) * g0.double()
            ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
            ratio = float(((out.double().cpu() - want).abs() / ulp).max())
            worst = max(worst, ratio)
            assert bool(torch.isfinite(out).all()) and ratio <= 4.0, (b, name, ratio)
            if b > 1:
                assert float(nk[1]) == 0.0 and not bool(out[1].any()), "an all-zero row must give zeros"
            if b > 2:
                assert abs(float(nk[2]) - 1.0) <= 4 * 2.0 ** -23
    print(f"grad_penalty_backward n={n}: worst {worst:.2f} ulp")


def test_penalty_through_ops_and_autograd(device):
    from vfi_amd.adacof.losses import adversarial
    g0 = _rows(3, 3 * 16 * 16, torch.Generator().manual_seed(2)).view(3, 3, 16, 16)
    g = g0.to(device).requires_grad_(True)
    value = adversarial.gradient_penalty(g)
    assert type(value.grad_fn).__name__.startswith("_GradPenalty") and value.dim() == 0
    (value * 0.5).backward()
    g64 = g0.double().requires_grad_(True)
    want = 10 * g64.flatten(1).norm(2, dim=1).sub(1).pow(2).mean()
    (want * 0.5).backward()
    # the norms are 0.5, 0.9, 1.3: a 2^-23 relative error of a norm is at most 1.1e-6 of | norm - 1 | >= 0.1
    assert abs(value.item() - want.item()) <= 1e-5 * want.item()
    assert float((g.grad.double().cpu() - g64.grad).norm() / g64.grad.norm()) <= 1e-5
    v2, norms = ops.grad_penalty_forward(g.detach())
    assert torch.equal(v2, value.detach()) and norms.shape == (3,)
