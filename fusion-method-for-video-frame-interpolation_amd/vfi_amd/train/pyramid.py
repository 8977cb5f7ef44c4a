"""Pyramid -- mirror of reference src/train/pyramid.py (`Pyramid(height, nbands, scale_factor, device)`,
`.filter(img[N,H,W]) -> DecompValues`, `.inv_filter(vals) -> [N,H,W]`, attrs .height/.nbands/.device/.pyr).

One library call per direction: `vfi_pyr_analyze` / `vfi_pyr_synthesize` (csrc/vfi_pyramid.hip) run the FFTs and
the fused mask / crop / shift / polar kernels; `coeff_to_values` / `values_to_coeff` (pyramid.py:48-112)
are fused in, so neither the coefficient lists nor the deepcopy (pyramid.py:49) exist.  Level geometry,
mask tables and FFT plans live in a plan cached per (H, W) instead of being rebuilt per frame
(reference src/fusion_net/interpolate_twoframe.py:124-129).

Extensions used by this package's own per-frame driver (not in the reference surface):
  * `filter(..., concat_frames=F)` writes the bands directly in PhaseNet's block-input layout
    (what separate_vals + get_concat_layers_inf + normalize_vals' phase/pi produce, src/train/utils.py:47-127);
  * entries of `vals.phase/amplitude` (or high_level / low_level) that are not tensors (the scalar 0 the
    reference itself uses for missing levels, src/phase_net/phase_net.py:91-93) are treated as zeros and
    their transforms are skipped.

`inv_filter` is differentiable with respect to high_level, phase, amplitude and low_level (the reference's PhaseNet
training backpropagates its L1 term through it, src/phase_net/architecture.py:69, src/train/loss.py:5-25): with grad mode
on and an input that requires grad it runs as the autograd node `Synthesis` (vfi_pyr_synthesize_backward).
`filter` in the per-image layout is differentiable with respect to img in the same way (the autograd node `Analysis`,
vfi_pyr_analyze_backward), so a loss in the pyramid domain (src/train/loss.py:5-25) can sit on a predicted image; so are
`band_filter` / `band_filter_pair` (self-adjoint radial filters: the backward is the same filter applied to the gradient).
"""
import ctypes
import math

import torch

from .. import _lib
from .._lib import VfiLibraryError
from ..steerable.SCFpyr_PyTorch import Analysis, BandFilter, SCFpyr_PyTorch, Synthesis, wants_grad
from ..values import DecompValues

__all__ = ["DecompValues", "Pyramid"]


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if torch.is_tensor(t) else None
    return arr


class Pyramid:
    """Steerable Pyramid Decomposition (reference src/train/pyramid.py:20-46)."""

    def __init__(self, height, nbands, scale_factor, device):
        self.height = height
        self.nbands = nbands
        self.scale_factor = scale_factor
        self.device = torch.device(device)
        self.pyr = SCFpyr_PyTorch(height=height, nbands=nbands, scale_factor=scale_factor, device=self.device)

    # -- analysis -------------------------------------------------------------------------------------
    def filter(self, img, concat_frames=None, phase_scale=1.0, level_mask=None, want_high=True, want_low=True, amp_max_eps=None,
               pred_channels=None):
        """Psi filter.  img (N,H,W) -> DecompValues in the per-image layout: high (N,1,H,W),
        phase/amplitude[k] (N*nbands,1,h_k,w_k) finest first with index img*nbands+band, low (N,1,hL,wL).

        concat_frames=F (N = F*C images ordered frame-major): PhaseNet layout instead -- phase/amplitude[k]
        are (C, F*nbands, h, w) views (channels [f0 b0..b3, f1 b0..b3]) of block-input buffers, lists ordered
        COARSEST first, high (C,F,H,W), low (C,F,hL,wL); see PhaseNet.normalize_vals.  The buffers are [feature 64 | prediction
        P | phase F*nbands | amp F*nbands]; pred_channels=(P of the coarsest level, P of the others), default (1, 8), is
        PhaseNet(num_img=F).pred_channels.  N = F*C is at most 16 images here (one slice of the plan: the amplitude maxima
        are reduced inside one launch); the per-image layout, inv_filter, band_filter and band_filter_pair take any N.

        The per-image layout is differentiable with respect to img (autograd node `Analysis`; the gradient of the phase is
        dropped where the amplitude is exactly 0, where torch.atan2 would give NaN).  The concat_frames layout is not:
        PhaseNet's inputs never need a gradient, and its outputs (the block-input buffers and amp_max included) are
        non-differentiable -- they never carry a grad_fn, whatever img requires."""
        if img.dim() != 3:
            raise VfiLibraryError("Pyramid.filter expects (N,H,W)")
        img = img.contiguous()
        n, h, w = img.shape
        if concat_frames is not None and n > 16:
            raise VfiLibraryError(f"Pyramid.filter(concat_frames={int(concat_frames)}): {n} images (frames x colours), a plan "
                                  "holds at most 16")
        plan = self.pyr.plan(h, w, n)
        nlev, nb = self.height - 2, self.nbands
        sizes = plan.sizes
        mask = (1 << nlev) - 1 if level_mask is None else int(level_mask)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=img.device)
        if concat_frames is None:
            layout = _PolarAnalysisLayout(plan, nlev, nb, phase_scale, mask, want_high, want_low)
            return layout.values(Analysis.apply(layout, img) if wants_grad([img]) else layout.forward(img))
        f = int(concat_frames)
        c = n // f
        if c * f != n:
            raise VfiLibraryError("concat_frames must divide the number of images")
        p_coarsest, p_band = (1, 8) if pred_channels is None else (int(pred_channels[0]), int(pred_channels[1]))
        if p_coarsest < 1 or p_band < 1:
            raise VfiLibraryError(f"pred_channels must be positive, got {pred_channels}")
        # block-input buffers [feature 64 | prediction P | phase f*nb | amp f*nb], P = p_coarsest at the coarsest level
        bufs, phase, amp, table = [], [], [], []
        for k in range(nlev):
            p_prev = p_coarsest if k == nlev - 1 else p_band
            ctot = 64 + p_prev + 2 * f * nb
            buf = new(c, ctot, *sizes[k])
            bufs.append(buf)
            phase.append(buf[:, 64 + p_prev:64 + p_prev + f * nb])
            amp.append(buf[:, 64 + p_prev + f * nb:])
            # image d = frame*c + colour -> batch colour, channel frame*nb (+ band); planes from the view's base
            table += [(d % c) * ctot + (d // c) * nb for d in range(n)]
        high = new(c, f, h, w) if want_high else 0
        low = new(c, f, *sizes[nlev]) if want_low else 0
        hi_tmp = new(n, h, w) if want_high else 0
        lo_tmp = new(n, *sizes[nlev]) if want_low else 0
        amp_max = None
        if amp_max_eps is not None:        # (levels finest first, colours): max amplitude + eps, for PhaseNet.normalize_vals
            amp_max = new(nlev, c)
        plan.analyze(img, hi_tmp, phase, amp, table, lo_tmp, phase_scale, mask, 0, amp_max=amp_max, groups=c,
                     eps=amp_max_eps if amp_max_eps is not None else 0.0)
        if want_high:
            high.copy_(hi_tmp.view(f, c, h, w).transpose(0, 1))
        if want_low:
            low.copy_(lo_tmp.view(f, c, *sizes[nlev]).transpose(0, 1))
        out = DecompValues(high, phase[::-1], amp[::-1], low)
        if amp_max is not None:
            return out, bufs[::-1], amp_max.flip(0).contiguous()      # coarsest first, like the lists
        return out, bufs[::-1]

    def band_filter(self, img, level_mask, keep_high=False, keep_low=False):
        """== inv_filter(keep(filter(img))) where `keep` zeroes every band level not in level_mask and the
        high / low residuals unless kept (get_last_value_levels / get_first_value_levels applied to UNMODIFIED
        values): a single radial frequency-domain gain (see vfi_pyr_plan_prepare_filter).  img (N,H,W)."""
        img = img.contiguous()
        n, h, w = img.shape
        plan = self.pyr.plan(h, w, n)
        if wants_grad([img]):
            return BandFilter.apply(plan, ((level_mask, keep_high, keep_low),), img)
        return plan.band_filter(img, level_mask, keep_high, keep_low)

    def band_filter_pair(self, img_a, spec_a, img_b, spec_b):
        """band_filter(img_a, **spec_a) + band_filter(img_b, **spec_b) (the sum of two unmodified level subsets of two
        image sets, e.g. the reference's "baseline" mix) with one inverse transform.  spec = dict(level_mask=...,
        keep_high=..., keep_low=...)."""
        img_a, img_b = img_a.contiguous(), img_b.contiguous()
        if img_a.shape != img_b.shape:
            raise VfiLibraryError("band_filter_pair: shape mismatch")
        n, h, w = img_a.shape
        tup = lambda d: (d["level_mask"], d.get("keep_high", False), d.get("keep_low", False))
        plan = self.pyr.plan(h, w, 2 * n)
        if wants_grad([img_a, img_b]):
            return BandFilter.apply(plan, (tup(spec_a), tup(spec_b)), img_a, img_b)
        return plan.band_filter_pair(img_a, tup(spec_a), img_b, tup(spec_b))

    # -- synthesis -------------------------------------------------------------------------------------
    def inv_filter(self, vals):
        """Psi^{-1} filter: per-image DecompValues -> (N,H,W)."""
        tensors = [t for t in list(vals.phase) + [vals.high_level, vals.low_level] if torch.is_tensor(t)]
        if not tensors:
            raise VfiLibraryError("inv_filter: all-zero values carry no shape")
        nlev, nb = self.height - 2, self.nbands
        if len(vals.phase) != nlev:
            raise VfiLibraryError(f"inv_filter: expected {nlev} band levels, got {len(vals.phase)}")
        if torch.is_tensor(vals.high_level):
            n, _, h, w = vals.high_level.shape
        else:
            k0 = next(k for k, p in enumerate(vals.phase) if torch.is_tensor(p))
            n = vals.phase[k0].shape[0] // nb
            h, w = self._full_size
        layout = _PolarLayout(self.pyr.plan(h, w, n), n, h, w, nlev, nb)
        inputs = [vals.high_level, *vals.phase, *vals.amplitude, vals.low_level]
        if wants_grad(inputs):
            return Synthesis.apply(layout, *inputs)
        return layout.forward(inputs)

    _full_size = None

    def set_full_size(self, h, w):
        """Only needed to invert values whose high_level was dropped (no tensor carries H, W)."""
        self._full_size = (h, w)


class _PolarAnalysisLayout:
    """filter's outputs in the per-image layout, flattened: [high (N,1,H,W)], phase[k], amplitude[k] ((N*nb,1,h,w)) of the
    levels in level_mask, finest first, [low (N,1,hL,wL)]."""

    def __init__(self, plan, nlev, nb, phase_scale, mask, want_high, want_low):
        self.plan, self.nlev, self.nb, self.phase_scale, self.mask = plan, nlev, nb, phase_scale, mask
        self.want_high, self.want_low = bool(want_high), bool(want_low)
        self.levels = [k for k in range(nlev) if (mask >> k) & 1]

    def forward(self, img):
        plan, nb, sizes = self.plan, self.nb, self.plan.sizes
        n, h, w = img.shape
        self.n = n                      # (one layout per call of filter)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=img.device)
        phase = [new(n * nb, 1, *sizes[k]) if (self.mask >> k) & 1 else 0 for k in range(self.nlev)]
        amp = [new(n * nb, 1, *sizes[k]) if (self.mask >> k) & 1 else 0 for k in range(self.nlev)]
        high = new(n, 1, h, w) if self.want_high else 0
        low = new(n, 1, *sizes[self.nlev]) if self.want_low else 0
        plan.analyze(img, high, phase, amp, None, low, self.phase_scale, self.mask, 0)
        return tuple([high] * self.want_high + [phase[k] for k in self.levels] + [amp[k] for k in self.levels] + [low] * self.want_low)

    def _split(self, flat):
        flat, m = list(flat), len(self.levels)
        high = flat.pop(0) if self.want_high else None
        low = flat.pop() if self.want_low else None
        return high, flat[:m], flat[m:2 * m], low

    def values(self, outputs):
        high, ph, am, low = self._split(outputs)
        phase, amp = [0] * self.nlev, [0] * self.nlev
        for i, k in enumerate(self.levels):
            phase[k], amp[k] = ph[i], am[i]
        return DecompValues(high if self.want_high else 0, phase, amp, low if self.want_low else 0)

    def saved(self, outputs):
        _, ph, am, _ = self._split(outputs)
        return (*ph, *am)

    def backward(self, saved, grads):
        plan, m = self.plan, len(self.levels)
        gh, gp, ga, gl = self._split(grads)
        ref = next(g for g in grads if g is not None)
        mask = 0
        dphi, damp, phase, amp = ([None] * self.nlev for _ in range(4))
        for i, k in enumerate(self.levels):
            if gp[i] is None and ga[i] is None:
                continue
            mask |= 1 << k
            phase[k], amp[k] = saved[i], saved[m + i]
            dphi[k] = gp[i] if gp[i] is not None else torch.zeros_like(phase[k])
            damp[k] = ga[i] if ga[i] is not None else torch.zeros_like(amp[k])
        grad_img = torch.empty((self.n, plan.h, plan.w), dtype=torch.float32, device=ref.device)
        plan.analyze_backward(gh.squeeze(1) if gh is not None else None, dphi, damp, phase, amp, None,
                              gl.squeeze(1) if gl is not None else None, self.phase_scale, mask, 0, grad_img)
        return grad_img


class _PolarLayout:
    """inv_filter's inputs, flattened: high (N,1,H,W), phase[0..L-1], amplitude[0..L-1] ((N*nb,1,h,w) finest first),
    low (N,1,hL,wL); any of them may be a non-tensor (zeros).  A level is synthesised when both its planes are tensors."""

    def __init__(self, plan, n, h, w, nlev, nb):
        self.plan, self.n, self.h, self.w, self.nlev, self.nb = plan, n, h, w, nlev, nb

    def _split(self, inputs):
        return inputs[0], inputs[1:1 + self.nlev], inputs[1 + self.nlev:1 + 2 * self.nlev], inputs[-1]

    def _levels(self, phase, amp):
        mask, ps, am = 0, [], []
        for k in range(self.nlev):
            p, a = phase[k], amp[k]
            if torch.is_tensor(p) and torch.is_tensor(a):
                if tuple(p.shape) != (self.n * self.nb, 1, *self.plan.sizes[k]):
                    raise VfiLibraryError(f"inv_filter: level {k} has shape {tuple(p.shape)}, expected "
                                          f"{(self.n * self.nb, 1, *self.plan.sizes[k])}")
                mask |= 1 << k
                ps.append(p.contiguous()); am.append(a.contiguous())
            else:
                ps.append(None); am.append(None)
        return mask, ps, am

    def forward(self, inputs):
        high, phase, amp, low = self._split(inputs)
        mask, phase, amp = self._levels(phase, amp)
        high = high.contiguous() if torch.is_tensor(high) else None
        low = low.contiguous() if torch.is_tensor(low) else None
        device = next(t for t in inputs if torch.is_tensor(t)).device
        img = torch.empty((self.n, self.h, self.w), dtype=torch.float32, device=device)
        self.plan.synthesize(high, phase, amp, None, low, mask, 0, img)
        return img

    def backward(self, grad, inputs, needs):
        L = self.nlev
        high, phase, amp, low = self._split(inputs)
        mask, phase, amp = self._levels(phase, amp)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=grad.device)
        gp, ga = [], []
        for k in range(L):
            if (mask >> k) & 1 and (needs[1 + k] or needs[1 + L + k]):
                gp.append(new(*phase[k].shape)); ga.append(new(*amp[k].shape))
            else:
                mask &= ~(1 << k)
                gp.append(None); ga.append(None)
        gh = new(self.n, 1, self.h, self.w) if needs[0] else None
        gl = new(self.n, 1, *self.plan.sizes[L]) if needs[-1] else None
        self.plan.synthesize_backward(grad, phase, amp, None, mask, 0, gh, gp, ga, gl)
        return [gh] + [g if nd else None for g, nd in zip(gp, needs[1:1 + L])] + \
            [g if nd else None for g, nd in zip(ga, needs[1 + L:1 + 2 * L])] + [gl]
