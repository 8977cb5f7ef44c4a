"""Float64 restatement of the pyramid's synthesis (oracle/pyramid_cpu.py: reconstruct + values_to_coeff) and its adjoint in
closed form: the references of the synthesis-gradient tests.  The mask tables are the oracle's PyramidSpec float32 tables
cast to double, so only the arithmetic is more precise.

Adjoint of img = Re(ifft2s(lo0 * R_0 + hi0 * fft2s(high))), R_k = embed(R_{k+1} * lomask_k) + sum_b (-i) P_s[k][b] fft2s(z_kb),
R_L = fft2s(low), for a gradient image g (fft2 un-normalised, ifft2 1/n):
  grad high = Re(ifft2s(fft2s(g) * hi0))
  grad z_kb = c_k * ifft2s(i * window_k(fft2s(g) * lo0 * prod_{j<k} lomask_j) * P_s[k][b]),  c_k = h_k w_k / (H W)
  grad low  = hL wL / (H W) * Re(ifft2s(window_L(fft2s(g) * lo0 * prod_j lomask_j)))
"""
import torch

from oracle.pyramid_cpu import _fft2s, _ifft2s


def _tables(spec):
    d = lambda t: t.double()
    return d(spec.lo0), d(spec.hi0), [d(m) for m in spec.himask], [d(m) for m in spec.lomask], [d(a) for a in spec.ang_s]


def reconstruct64(spec, coeff):
    """pyramid_cpu.reconstruct in float64: coeff = [hi (N,H,W), [nb x (N,h,w,2)] x L, lo (N,hL,wL)] -> (N,H,W)."""
    lo0, hi0, himask, lomask, ang_s = _tables(spec)
    n = coeff[0].shape[0]
    res = _fft2s(coeff[-1].double())
    for k in range(spec.nlev - 1, -1, -1):
        ys, xs = spec.crop(k)
        cur = torch.zeros((n, *spec.sizes[k]), dtype=torch.complex128)
        cur[:, ys, xs] = res * lomask[k]
        for b in range(spec.nbands):
            z = _fft2s(torch.view_as_complex(coeff[1 + k][b].double().contiguous())) * ang_s[k][b] * himask[k]
            cur = cur + z * (-1j)
        res = cur
    return _ifft2s(res * lo0 + _fft2s(coeff[0].double()) * hi0).real


def polar_to_coeff(high, phase, amp, low, nbands=4):
    """layout_cpu.values_to_coeff for per-image (N,1,..) / (N*nb,1,..) tensors (any dtype; keeps autograd)."""
    n = high.shape[0]
    coeff = [high.squeeze(1)]
    for p, a in zip(phase, amp):
        p = p.reshape(n, nbands, *p.shape[2:])
        a = a.reshape(n, nbands, *a.shape[2:])
        coeff.append([torch.stack((torch.cos(p[:, b]) * a[:, b], torch.sin(p[:, b]) * a[:, b]), -1) for b in range(nbands)])
    coeff.append(low.squeeze(1))
    return coeff


def adjoint64(spec, g):
    """Closed-form adjoint of reconstruct for the gradient image g (N,H,W) -> (grad hi (N,H,W),
    [[grad z_kb (N,h,w) complex128] x nb] x L, grad lo (N,hL,wL))."""
    lo0, hi0, himask, lomask, ang_s = _tables(spec)
    H, W = spec.H, spec.W
    G = _fft2s(g.double())
    ghi = _ifft2s(G * hi0).real
    lod = G * lo0
    bands = []
    for k in range(spec.nlev):
        h, w = spec.sizes[k]
        c = h * w / (H * W)
        bands.append([c * _ifft2s(1j * lod * ang_s[k][b] * himask[k]) for b in range(spec.nbands)])
        ys, xs = spec.crop(k)
        lod = lod[:, ys, xs] * lomask[k]
    hl, wl = spec.sizes[-1]
    return ghi, bands, hl * wl / (H * W) * _ifft2s(lod).real


def polar_grads(z_grad, phase, amp, nbands=4):
    """(d phase, d amplitude) of one level from its coefficient gradients [nb x (N,h,w) complex] and the forward's
    (N*nb,1,h,w) phase / amplitude: d A = Re G cos p + Im G sin p, d p = A (Im G cos p - Re G sin p)."""
    G = torch.stack(z_grad, 1).reshape(phase.shape)
    p, a = phase.double(), amp.double()
    return a * (G.imag * torch.cos(p) - G.real * torch.sin(p)), G.real * torch.cos(p) + G.imag * torch.sin(p)
