"""vfi_mse_forward / vfi_mse_backward alone: the squared-error term on the two-stage fixed-order
reduction of csrc/vfi_grad_common.h.

Counts: 1, 3, 4, 255, 256, 257, 1024, 4099 and the first counts past one trip of the largest grid.  `reduce_blocks` caps the
grid at kMaxPartials = 1024 blocks of kThreads = 256, so one trip covers 1024 * 256 = 262144 items: floats on the 4-byte
path, float4s on the 16-byte path.  262145 (4-byte path, either alignment) and 4 * 262144 + 4 = 1048580 (16-byte path when
aligned) are each one item past it.  Every count runs 16-byte aligned and as a slice starting one float into a buffer (the
4-byte path), and every buffer -- inputs, gradients, the scalar -- ends inside NaN canaries that must survive.

Bounds.  Integer-valued data (differences in [-3, 3], sum of squares below 2^24): every product and partial sum is exact,
so the forward is float64's value rounded once when the count is a power of two (1 / count exact), and within 2 ulp
otherwise (the rounding of 1 / count to fp32, then of the product).  Uniform [0, 1) data: the project's bounds for the
Charbonnier node, which shares the reduction (tests/test_adacofnet_backward_gpu.py: 1e-6 relative forward, rtol 1e-5 /
atol 1e-9 backward)."""
import numpy as np
import pytest
import torch

from vfi_amd import _lib, ops
from vfi_amd._lib import VfiLibraryError

pytestmark = pytest.mark.gpu

ONE_TRIP = 1024 * 256                       # kMaxPartials * kThreads (csrc/vfi_grad_common.h: reduce_blocks)
COUNTS = [1, 3, 4, 255, 256, 257, 1024, 4099, ONE_TRIP + 1, 4 * ONE_TRIP + 4]
GUARD = 8                                   # canary floats on each side (a multiple of 4: alignment is the offset's alone)


class Guarded:
    """`count` floats at `offset` floats past a 16-byte boundary, between NaN canaries."""

    def __init__(self, count, offset, device, values=None):
        self.buf = torch.full((GUARD + offset + count + GUARD,), float("nan"), device=device)
        self.lo, self.hi = GUARD + offset, GUARD + offset + count
        self.view = self.buf[self.lo:self.hi]
        assert self.view.data_ptr() % 16 == 4 * offset
        if values is not None:
            self.view.copy_(values)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())


def _forward(a, b, device):
    """one vfi_mse_forward call on guarded operands -> (0-dim tensor, every canary intact)"""
    out = Guarded(1, 0, device)
    ws = Guarded(_lib.REDUCE_WORKSPACE_FLOATS, 0, device)
    _lib.call("vfi_mse_forward", a.view.data_ptr(), b.view.data_ptr(), a.view.numel(), ws.view.data_ptr(),
              out.view.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.view[0].clone(), all(t.intact() for t in (a, b, out, ws))


def _backward(a, b, up, need_a, need_b, offset, device):
    n = a.view.numel()
    ga = Guarded(n, offset, device) if need_a else None
    gb = Guarded(n, offset, device) if need_b else None
    _lib.call("vfi_mse_backward", a.view.data_ptr(), b.view.data_ptr(), up.data_ptr(), ga.view.data_ptr() if need_a else None,
              gb.view.data_ptr() if need_b else None, n, _lib.stream_ptr())
    torch.cuda.synchronize()
    ok = all(t.intact() for t in (a, b, ga, gb) if t is not None)
    return (ga.view.clone() if need_a else None), (gb.view.clone() if need_b else None), ok


def _ulp_distance(x, y):
    i = lambda v: int(np.float32(v).view(np.int32))
    return abs(i(x) - i(y))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("count", COUNTS)
def test_mse_entries(count, offset, device):
    g = torch.Generator().manual_seed(count * 2 + offset)
    # integer-valued data: exact sums
    ai = torch.randint(0, 4, (count,), generator=g).float()
    bi = torch.randint(0, 4, (count,), generator=g).float()
    assert float(((ai - bi).double() ** 2).sum()) < 2 ** 24
    a, b = Guarded(count, offset, device, ai), Guarded(count, offset, device, bi)
    got, ok = _forward(a, b, device)
    assert ok
    want64 = float(((ai.double() - bi.double()) ** 2).mean())
    want = float(np.float32(want64))
    ulps = _ulp_distance(float(got), want)
    print(f"count {count} offset {offset}: integer data {float(got)!r} vs {want!r}: {ulps} ulp")
    if count & (count - 1) == 0:
        assert float(got) == want
    else:
        assert ulps <= 2
    again, ok = _forward(a, b, device)
    assert ok and torch.equal(again, got)

    # uniform data against float64
    au, bu = torch.rand(count, generator=g), torch.rand(count, generator=g)
    a, b = Guarded(count, offset, device, au), Guarded(count, offset, device, bu)
    ad, bd = au.double().requires_grad_(True), bu.double().requires_grad_(True)
    want = ((ad - bd) ** 2).mean()
    (want * 0.7).backward()
    want = want.detach()
    got, ok = _forward(a, b, device)
    assert ok
    print(f"count {count} offset {offset}: uniform data rel err {abs(float(got) - float(want)) / float(want):.3e}")
    assert abs(float(got) - float(want)) <= 1e-6 * float(want)
    again, ok = _forward(a, b, device)
    assert ok and torch.equal(again, got)
    up = torch.tensor([0.7], device=device)
    first = None
    for need_a, need_b in ((True, True), (True, False), (False, True)):
        ga, gb, ok = _backward(a, b, up, need_a, need_b, offset, device)
        assert ok
        if need_a:
            assert torch.allclose(ga.cpu().double(), ad.grad, rtol=1e-5, atol=1e-9)
        if need_b:
            assert torch.allclose(gb.cpu().double(), bd.grad, rtol=1e-5, atol=1e-9)
        if first is None:
            first = (ga, gb)
            ga2, gb2, ok = _backward(a, b, up, True, True, offset, device)
            assert ok and torch.equal(ga2, ga) and torch.equal(gb2, gb)
        else:                                           # the same bits whichever outputs are asked for
            assert (not need_a or torch.equal(ga, first[0])) and (not need_b or torch.equal(gb, first[1]))
    # the wrappers: the same bits as the direct calls
    assert torch.equal(ops.mse_forward(a.view, b.view), got)
    wa, wb = ops.mse_backward(a.view, b.view, up[0], need_a=True, need_b=True)
    assert torch.equal(wa, first[0]) and torch.equal(wb, first[1])
    assert ops.mse_backward(a.view, b.view, up[0], need_a=True, need_b=False)[1] is None


def test_mse_on_the_two_halves_of_one_tensor(device):
    """b is a pointer into a's allocation: the VGG term's call"""
    g = torch.Generator().manual_seed(5)
    feat = torch.rand((4, 8, 3, 5), generator=g)
    d = feat.to(device)
    want = ((feat[:2].double() - feat[2:].double()) ** 2).mean()
    got = ops.mse_forward(d[:2], d[2:])
    assert abs(float(got) - float(want)) <= 1e-6 * float(want)
    ga, gb = ops.mse_backward(d[:2], d[2:], torch.tensor(1.0, device=device), need_a=True, need_b=False)
    assert gb is None
    assert torch.allclose(ga.cpu().double(), 2 * (feat[:2].double() - feat[2:].double()) / feat[:2].numel(), rtol=1e-5, atol=1e-9)
    assert torch.equal(d.cpu(), feat)


def test_mse_rejects_null_pointers_and_empty_counts(device):
    a, b = Guarded(16, 0, device, torch.ones(16)), Guarded(16, 0, device, torch.zeros(16))
    out, ws, ga = Guarded(1, 0, device), Guarded(_lib.REDUCE_WORKSPACE_FLOATS, 0, device), Guarded(16, 0, device)
    up = torch.ones(1, device=device)
    s = _lib.stream_ptr()
    A, B, O, W, G = (t.view.data_ptr() for t in (a, b, out, ws, ga))
    U = up.data_ptr()
    bad_forward = [(None, B, 16, W, O), (A, None, 16, W, O), (A, B, 16, None, O), (A, B, 16, W, None), (A, B, 0, W, O), (A, B, -4, W, O)]
    bad_backward = [(None, B, U, G, None, 16), (A, None, U, G, None, 16), (A, B, None, G, None, 16), (A, B, U, None, None, 16),
                    (A, B, U, G, None, 0), (A, B, U, G, None, -1)]
    for args in bad_forward:
        with pytest.raises(VfiLibraryError):
            _lib.call("vfi_mse_forward", *args, s)
    for args in bad_backward:
        with pytest.raises(VfiLibraryError):
            _lib.call("vfi_mse_backward", *args, s)
    torch.cuda.synchronize()
    assert all(t.intact() for t in (a, b, out, ws, ga))
    assert bool(torch.isnan(out.view).all()) and bool(torch.isnan(ga.view).all())       # nothing was launched
    with pytest.raises(VfiLibraryError):
        ops.mse_forward(a.view, b.view[:8])
