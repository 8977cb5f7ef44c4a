"""CPU checks of the closed forms behind FusionNet's HIP backward: float64 host models of the
reflect-padding fold of vfi_conv2d_backward_data, the max-pool routing of vfi_pool2_max_backward and the x2 bilinear
adjoint of vfi_resize_bilinear_backward, written the way the kernels compute them, against torch.autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def reflect_sources(y, n, p):
    """Padded indices whose reflect source is y (reflect_sources in vfi_conv_grad.hip)."""
    u = [y + p]
    if 1 <= y <= p:
        u.append(p - y)
    if n - 1 - p <= y <= n - 2:
        u.append(2 * (n - 1) - y + p)
    return u


def reflect_fold(d, p):
    n, c, hp, wp = d.shape
    h, w = hp - 2 * p, wp - 2 * p
    out = np.zeros((n, c, h, w))
    for y in range(h):
        for x in range(w):
            for u in reflect_sources(y, h, p):
                for v in reflect_sources(x, w, p):
                    out[:, :, y, x] += d[:, :, u, v]
    return out


def dgrad_model(dy, w, pad_mode):
    """vfi_conv2d_backward_data's route: zero-embed dy by p, zero-padded conv with W^T flipped, fold the padding."""
    k = w.shape[-1]
    p = (k - 1) // 2
    wt = torch.from_numpy(w).transpose(0, 1).flip(2, 3)
    if pad_mode == "zeros" or p == 0:
        return F.conv2d(torch.from_numpy(dy), wt, padding=p).numpy()
    e = np.pad(dy, ((0, 0), (0, 0), (p, p), (p, p)))
    d = F.conv2d(torch.from_numpy(e), wt, padding=p).numpy()
    return reflect_fold(d, p)


def conv(x, w, pad_mode):
    p = (w.shape[-1] - 1) // 2
    if p and pad_mode == "reflect":
        return F.conv2d(F.pad(x, (p,) * 4, mode="reflect"), w)
    return F.conv2d(x, w, padding=p)


def up2_sources(j, n):
    """(output index, weight) pairs reading source j of a x2, align_corners=False axis (up2_sources in the kernel)."""
    s = []
    if j >= 1:
        s.append((2 * j - 1, 0.25))
    s.append((2 * j, 1.0 if j == 0 else 0.75))
    s.append((2 * j + 1, 1.0 if j == n - 1 else 0.75))
    if j + 1 <= n - 1:
        s.append((2 * j + 2, 0.25))
    return s


def up2_adjoint(x, g, relu_input):
    n, c, h, w = x.shape
    out = np.zeros_like(x)
    for y in range(h):
        for xx in range(w):
            for oy, wy in up2_sources(y, h):
                for ox, wx in up2_sources(xx, w):
                    out[:, :, y, xx] += wy * wx * g[:, :, oy, ox]
    return out * (x > 0) if relu_input else out


def pool_route(s, gp, gskip):
    n, c, h, w = s.shape
    out = gskip.copy()
    for yo in range(h // 2):
        for xo in range(w // 2):
            win = s[:, :, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2].reshape(n, c, 4)
            arg = np.zeros((n, c), dtype=int)
            for k in range(1, 4):             # strict '>': the first maximal element in row-major order wins
                arg = np.where(win[:, :, k] > np.take_along_axis(win, arg[..., None], 2)[..., 0], k, arg)
            for k in range(4):
                out[:, :, 2 * yo + k // 2, 2 * xo + k % 2] += np.where(arg == k, gp[:, :, yo, xo], 0.0)
    return out * (s > 0)


@pytest.mark.parametrize("ks,pad_mode,h,w", [(5, "reflect", 3, 3), (5, "reflect", 4, 7), (5, "reflect", 9, 6),
                                             (3, "reflect", 2, 2), (3, "reflect", 2, 5), (3, "reflect", 7, 4),
                                             (1, "reflect", 3, 2), (5, "zeros", 3, 4), (3, "zeros", 1, 1),
                                             (1, "zeros", 2, 3)])
def test_input_gradient_route_matches_autograd(ks, pad_mode, h, w):
    rng = np.random.default_rng(ks * 100 + h * 10 + w)
    x = rng.standard_normal((2, 3, h, w))
    wt = rng.standard_normal((4, 3, ks, ks))
    g = rng.standard_normal((2, 4, h, w))
    xt = torch.from_numpy(x).requires_grad_(True)
    (conv(xt, torch.from_numpy(wt), pad_mode) * torch.from_numpy(g)).sum().backward()
    np.testing.assert_allclose(dgrad_model(g, wt, pad_mode), xt.grad.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("ks,pad_mode", [(5, "reflect"), (3, "reflect"), (1, "reflect"), (5, "zeros"), (3, "zeros")])
def test_adjoint_identity(ks, pad_mode):
    """<conv(x), g> == <x, dgrad(g)> for the reflect fold route (the defining property of the input gradient)."""
    rng = np.random.default_rng(ks)
    x = rng.standard_normal((2, 6, 11, 8))
    wt = rng.standard_normal((5, 6, ks, ks))
    g = rng.standard_normal((2, 5, 11, 8))
    lhs = float((conv(torch.from_numpy(x), torch.from_numpy(wt), pad_mode).numpy() * g).sum())
    rhs = float((x * dgrad_model(g, wt, pad_mode)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_reflect_sources_cover_every_padded_index_once():
    for n in range(2, 9):
        for p in (1, 2):
            if p >= n:
                continue
            hits = sorted(u for y in range(n) for u in reflect_sources(y, n, p))
            assert hits == list(range(n + 2 * p)), (n, p, hits)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 4), (2, 3), (5, 9), (8, 8)])
@pytest.mark.parametrize("relu_input", [True, False])
def test_bilinear_x2_adjoint_matches_autograd(h, w, relu_input):
    rng = np.random.default_rng(h * 10 + w)
    x = rng.standard_normal((2, 3, h, w))
    g = rng.standard_normal((2, 3, 2 * h, 2 * w))
    xt = torch.from_numpy(x).requires_grad_(True)
    src = torch.relu(xt) if relu_input else xt
    (F.interpolate(src, scale_factor=2, mode="bilinear", align_corners=False) * torch.from_numpy(g)).sum().backward()
    np.testing.assert_allclose(up2_adjoint(x, g, relu_input), xt.grad.numpy(), rtol=0, atol=1e-12)


def test_max_pool_routing_with_ties_matches_autograd():
    rng = np.random.default_rng(0)
    s = np.maximum(np.round(rng.standard_normal((2, 3, 6, 8)), 1), 0.0)
    s[0, 0, 0:2, 0:2] = 0.5                                  # four-way tie
    s[0, 1, 2:4, 4:6] = [[0.1, 0.9], [0.9, 0.9]]             # three-way tie, not at the first element
    s[1, 2, 4:6, 0:2] = [[0.0, 0.0], [0.3, 0.3]]             # tie in the second row
    s[1, 0, 0:2, 6:8] = 0.0                                  # no positive element: masked by the ReLU
    gp = rng.standard_normal((2, 3, 3, 4))
    gk = rng.standard_normal((2, 3, 6, 8))
    z = torch.from_numpy(s).requires_grad_(True)
    y = torch.relu(z)
    ((F.max_pool2d(y, 2, 2) * torch.from_numpy(gp)).sum() + (y * torch.from_numpy(gk)).sum()).backward()
    got = pool_route(s, gp, gk)
    np.testing.assert_allclose(got, z.grad.numpy(), rtol=0, atol=1e-12)
    assert got[0, 0, 0, 0] == gp[0, 0, 0, 0] + gk[0, 0, 0, 0] and got[0, 0, 1, 1] == gk[0, 0, 1, 1]
    assert got[0, 1, 2, 5] == gp[0, 1, 1, 2] + gk[0, 1, 2, 5]
