"""Float64 restatement of the pyramid's analysis (oracle/pyramid_cpu.py: build + coeff_to_values, with the phase scale of
Pyramid.filter) and its adjoint in closed form: the references of the analysis-gradient tests.  The mask tables are the
oracle's PyramidSpec float32 tables cast to double, so only the arithmetic is more precise.

Forward, for X = fft2s(x) (fft2 un-normalised, ifft2 1/n, the `s` variants in fft-shifted coordinates):
  z_kb = ifft2s(i * W_k * ang_a[k][b] * himask_k),  W_0 = X * lo0,  W_{k+1} = crop_k(W_k) * lomask_k
  high = Re ifft2s(X * hi0),  low = Re ifft2s(W_L),  A = |z|,  phi = s * atan2(Im z, Re z)
Adjoint, for upstream gradients (d high, G_kb = dL/dRe z + i dL/dIm z, d low); every mask is real, the adjoint of the crop
is the zero-padded embed, of ifft2 (1/n) fft2, of fft2 n * ifft2:
  R_L = fft2s(d low) / (hL wL)
  R_k = embed_k(R_{k+1} * lomask_k) + sum_b (-i) * ang_a[k][b] * himask_k * fft2s(G_kb) / (h_k w_k)
  grad x = H W * Re ifft2s(R_0 * lo0 + fft2s(d high) * hi0 / (H W))
Polar map: G = (dA + i * s * dphi / A) * exp(i * phi / s); where A == 0 the dphi term is dropped (torch's atan2 gives NaN
there: the kernels' convention, the mirror of `d phase = 0 at A = 0` of the synthesis gradient).
"""
import torch

from oracle.pyramid_cpu import _fft2s, _ifft2s


def _tables(spec):
    d = lambda t: t.double()
    return d(spec.lo0), d(spec.hi0), [d(m) for m in spec.himask], [d(m) for m in spec.lomask], [d(a) for a in spec.ang_a]


def build64(spec, im):
    """pyramid_cpu.build in float64 (keeps autograd): im (N,H,W) -> (high (N,H,W), [[z_kb (N,h,w) complex128] x nb] x L,
    low (N,hL,wL))."""
    lo0, hi0, himask, lomask, ang_a = _tables(spec)
    dft = _fft2s(im.double())
    lodft = dft * lo0
    bands = []
    for k in range(spec.nlev):
        bands.append([_ifft2s(1j * lodft * ang_a[k][b] * himask[k]) for b in range(spec.nbands)])
        ys, xs = spec.crop(k)
        lodft = lodft[:, ys, xs] * lomask[k]
    return _ifft2s(dft * hi0).real, bands, _ifft2s(lodft).real


def analyze64(spec, im, phase_scale=1.0):
    """Pyramid.filter in float64: (high (N,1,H,W), phase[k], amplitude[k] (N*nb,1,h,w) with index img*nb+band, low (N,1,hL,wL))."""
    high, bands, low = build64(spec, im)
    phase, amp = [], []
    for level in bands:
        z = torch.stack(level, 1).reshape(-1, 1, *level[0].shape[1:])
        phase.append(torch.atan2(z.imag, z.real) * phase_scale)
        amp.append(z.abs())
    return high.unsqueeze(1), phase, amp, low.unsqueeze(1)


def analysis_adjoint64(spec, dhigh, G, dlow):
    """Closed-form adjoint of build64: dhigh (N,H,W) or None, G = [[G_kb (N,h,w) complex] x nb or None] x L, dlow (N,hL,wL)
    or None -> grad x (N,H,W) float64."""
    lo0, hi0, himask, lomask, ang_a = _tables(spec)
    H, W = spec.H, spec.W
    n = next(t for t in [dhigh, dlow] + [g[0] for g in G if g is not None] if t is not None).shape[0]
    hl, wl = spec.sizes[-1]
    res = _fft2s(dlow.double()) / (hl * wl) if dlow is not None else torch.zeros((n, hl, wl), dtype=torch.complex128)
    for k in range(spec.nlev - 1, -1, -1):
        h, w = spec.sizes[k]
        ys, xs = spec.crop(k)
        cur = torch.zeros((n, h, w), dtype=torch.complex128)
        cur[:, ys, xs] = res * lomask[k]
        if G[k] is not None:
            for b in range(spec.nbands):
                cur = cur + (-1j) * ang_a[k][b] * himask[k] * _fft2s(G[k][b].to(torch.complex128)) / (h * w)
        res = cur
    out = res * lo0
    if dhigh is not None:
        out = out + _fft2s(dhigh.double()) * hi0 / (H * W)
    return H * W * _ifft2s(out).real


def polar_to_coeff_grad(dphi, damp, phi, amp, s=1.0):
    """Coefficient gradient G (complex128, shape of phi) of one level from the gradients of (phi, A) and the forward's own
    (phi, A): G = (dA + i s dphi / A) exp(i phi / s), without the dphi term where A == 0."""
    p, a = phi.double() / s, amp.double()
    tang = torch.where(a > 0, s * dphi.double() / torch.where(a > 0, a, torch.ones_like(a)), torch.zeros_like(a))
    return torch.complex(damp.double(), tang) * torch.complex(torch.cos(p), torch.sin(p))


def level_bands(G, n, nbands=4):
    """(N*nb,1,h,w) complex with index img*nb+band -> [nb x (N,h,w)] as analysis_adjoint64 takes a level."""
    g = G.reshape(n, nbands, *G.shape[2:])
    return [g[:, b] for b in range(nbands)]
