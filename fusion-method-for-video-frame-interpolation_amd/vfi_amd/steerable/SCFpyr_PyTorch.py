"""`SCFpyr_PyTorch(height, nbands, scale_factor, device)` with `.build(x[N,1,H,W]) -> coeff` and
`.reconstruct(coeff) -> [N,H,W]` -- the surface of the third-party class the reference constructs at
src/train/pyramid.py:28-33 and calls at :37,44.  Coefficient layout as the reference expects it:
coeff = [hi (N,H,W), [nbands x (N,h,w,2)] per level finest first, lo (N,hL,wL)] (pyramid.py:56-61).

Backed by one plan per (H, W) in libvfi_hip.so (level geometry, mask tables, the tables of the hand-written FFT
engines -- no FFT library is linked --, workspace).  N is not limited: a plan's workspace holds at most 16 images, and the
library walks a call of more images in slices of that many, so a whole training batch is one call.

`reconstruct` (and `vfi_amd.train.Pyramid.inv_filter`) is differentiable with respect to its inputs: when grad mode is on
and an input requires grad it runs as the autograd node `Synthesis`, whose backward is vfi_pyr_synthesize_backward.
`build` (and `vfi_amd.train.Pyramid.filter` in the per-image layout) is differentiable with respect to the image in the same
way: the autograd node `Analysis`, whose backward is vfi_pyr_analyze_backward.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import VfiLibraryError

BAND_MAJOR, COMPLEX_COEFF = 1, 2


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if torch.is_tensor(t) else None
    return arr


class Plan:
    """RAII handle of a vfi_pyr_plan."""

    def __init__(self, h, w, height, nbands, scale_factor, max_images, device):
        if torch.device(device).type != "cuda":
            raise VfiLibraryError("the pyramid needs a HIP device (vfi_amd has no CPU path)")
        self.h, self.w, self.height, self.nbands, self.max_images = h, w, height, nbands, max_images
        self.device = torch.device(device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.call("vfi_pyr_plan_create", h, w, height, nbands, float(scale_factor), max_images, ctypes.byref(self._h))
        self.sizes = []
        for k in range(height - 1):
            a, b = ctypes.c_int(), ctypes.c_int()
            _lib.call("vfi_pyr_plan_level_size", self._h, k, ctypes.byref(a), ctypes.byref(b))
            self.sizes.append((a.value, b.value))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().vfi_pyr_plan_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    PASSES = {"rows": 0, "ana_cols": 1, "syn_cols": 2}

    def pass_info(self, size_index, which):
        """How the plan runs one pass ("rows", "ana_cols", "syn_cols") of band level size_index, of the low residual
        (size_index == height-2) or of the frame (height-1): vfi_pyr_plan_query_pass as a dict.  M == 0: the generic engine."""
        info = (ctypes.c_int * 8)()
        _lib.call("vfi_pyr_plan_query_pass", self._h, int(size_index), self.PASSES[which], info)
        return dict(zip(("n", "bluestein", "m", "M", "tile", "bands", "tpitch_ana", "tpitch_syn"), info))

    def multi_levels(self, n, mask):
        """The levels of `mask` that an analysis of n images batches onto the generic engine (vfi_pyr_plan_multi_levels)."""
        out = ctypes.c_ulonglong()
        _lib.call("vfi_pyr_plan_multi_levels", self._h, int(n), int(mask), ctypes.byref(out))
        return out.value

    def _bytes(self, n, mask, high, low):
        """Algorithmic HBM bytes of one transform: image + kept band planes (phase, amp) + residuals."""
        px = self.h * self.w + (self.h * self.w if high else 0) + (self.sizes[-1][0] * self.sizes[-1][1] if low else 0)
        px += sum(2 * self.nbands * a * b for k, (a, b) in enumerate(self.sizes[:-1]) if (mask >> k) & 1)
        return 4.0 * n * px

    def analyze(self, img, high, phase, amp, table, low, phase_scale, mask, flags, amp_max=None, groups=1, eps=0.0):
        """amp_max: optional (levels, groups) float tensor that receives max amplitude + eps per level and image group
        (image d belongs to group d % groups): PhaseNet.normalize_vals' maxima, reduced by the kernel that writes them."""
        n = img.shape[0]
        tab = (ctypes.c_int * len(table))(*table) if table is not None else None
        head = (self._h, _lib.dptr(img, "img"), n, high.data_ptr() if torch.is_tensor(high) else None, _ptr_array(phase),
                _ptr_array(amp) if amp is not None else None, tab, low.data_ptr() if torch.is_tensor(low) else None,
                float(phase_scale), mask, flags)
        work = ("byte", self._bytes(n, mask, torch.is_tensor(high), torch.is_tensor(low)), "pyr_analyze")
        if amp_max is None:
            _lib.call("vfi_pyr_analyze", *head, _lib.stream_ptr(), work=work)
        else:
            _lib.call("vfi_pyr_analyze_max", *head, _lib.dptr(amp_max, "amp_max"), int(groups), float(eps), _lib.stream_ptr(), work=work)

    def band_filter(self, img, level_mask, keep_high, keep_low):
        """real(ifft2(fft2(img) * G)): analysis + synthesis of an unmodified level subset as ONE radial filter."""
        key = (int(level_mask), bool(keep_high), bool(keep_low))
        if not hasattr(self, "_filters"):
            self._filters = {}
        if key not in self._filters:
            fid = ctypes.c_int()
            _lib.call("vfi_pyr_plan_prepare_filter", self._h, key[0], int(key[1]), int(key[2]), ctypes.byref(fid))
            self._filters[key] = fid.value
        out = torch.empty_like(img)
        n = img.shape[0]
        _lib.call("vfi_pyr_apply_filter", self._h, self._filters[key], _lib.dptr(img, "img"), n, out.data_ptr(),
                  _lib.stream_ptr(), work=("byte", 8.0 * n * self.h * self.w, "pyr_band_filter"))
        return out

    def _filter_id(self, level_mask, keep_high, keep_low):
        key = (int(level_mask), bool(keep_high), bool(keep_low))
        if not hasattr(self, "_filters"):
            self._filters = {}
        if key not in self._filters:
            fid = ctypes.c_int()
            _lib.call("vfi_pyr_plan_prepare_filter", self._h, key[0], int(key[1]), int(key[2]), ctypes.byref(fid))
            self._filters[key] = fid.value
        return self._filters[key]

    def band_filter_pair(self, img_a, spec_a, img_b, spec_b):
        """band_filter(img_a, *spec_a) + band_filter(img_b, *spec_b) with one inverse transform; spec = (level_mask,
        keep_high, keep_low)."""
        fa, fb = self._filter_id(*spec_a), self._filter_id(*spec_b)
        out = torch.empty_like(img_a)
        n = img_a.shape[0]
        _lib.call("vfi_pyr_apply_filter_pair", self._h, fa, _lib.dptr(img_a, "img_a"), fb, _lib.dptr(img_b, "img_b"), n,
                  out.data_ptr(), _lib.stream_ptr(), work=("byte", 12.0 * n * self.h * self.w, "pyr_band_filter_pair"))
        return out

    def synthesize_backward(self, grad_img, phase, amp, table, mask, flags, grad_high, grad_phase, grad_amp, grad_low):
        """Gradients of `synthesize` for the loss gradient grad_img (N,H,W): arguments in synthesize's layout; grad_phase
        receives interleaved (re, im) gradients with COMPLEX_COEFF.  Builds the plan's adjoint tables on first use."""
        if not getattr(self, "_adjoint", False):
            with torch.cuda.device(self.device):
                _lib.call("vfi_pyr_plan_prepare_adjoint", self._h)
            self._adjoint = True
        n = grad_img.shape[0]
        tab = (ctypes.c_int * len(table))(*table) if table is not None else None
        polar = not flags & COMPLEX_COEFF
        reads = 4.0 * n * sum(2 * self.nbands * a * b for k, (a, b) in enumerate(self.sizes[:-1]) if (mask >> k) & 1) if polar else 0.0
        _lib.call("vfi_pyr_synthesize_backward", self._h, _lib.dptr(grad_img, "grad_img"), n,
                  _ptr_array(phase) if phase is not None else None, _ptr_array(amp) if amp is not None else None, tab, mask, flags,
                  grad_high.data_ptr() if torch.is_tensor(grad_high) else None, _ptr_array(grad_phase),
                  _ptr_array(grad_amp) if grad_amp is not None else None, grad_low.data_ptr() if torch.is_tensor(grad_low) else None,
                  _lib.stream_ptr(),
                  work=("byte", self._bytes(n, mask, torch.is_tensor(grad_high), torch.is_tensor(grad_low)) + reads,
                        "pyr_synthesize_backward"))

    def analyze_backward(self, grad_high, grad_phase, grad_amp, phase, amp, table, grad_low, phase_scale, mask, flags, grad_img):
        """Gradient of `analyze` with respect to img, written to grad_img (N,H,W): arguments in analyze's layout; phase / amp
        are the forward's outputs; grad_phase holds interleaved (re, im) coefficient gradients with COMPLEX_COEFF (phase, amp,
        grad_amp unused).  grad_high / grad_low None and clear mask bits are zero gradients.  Builds the plan's
        analysis-adjoint tables on first use."""
        if not getattr(self, "_analysis_adjoint", False):
            with torch.cuda.device(self.device):
                _lib.call("vfi_pyr_plan_prepare_analysis_adjoint", self._h)
            self._analysis_adjoint = True
        n = grad_img.shape[0]
        tab = (ctypes.c_int * len(table))(*table) if table is not None else None
        polar = not flags & COMPLEX_COEFF
        reads = 4.0 * n * sum(2 * self.nbands * a * b for k, (a, b) in enumerate(self.sizes[:-1]) if (mask >> k) & 1) if polar else 0.0
        opt = lambda t: _ptr_array(t) if t is not None else None
        _lib.call("vfi_pyr_analyze_backward", self._h, grad_high.data_ptr() if torch.is_tensor(grad_high) else None,
                  _ptr_array(grad_phase), opt(grad_amp), opt(phase), opt(amp), tab,
                  grad_low.data_ptr() if torch.is_tensor(grad_low) else None, float(phase_scale), mask, flags,
                  _lib.dptr(grad_img, "grad_img"), n, _lib.stream_ptr(),
                  work=("byte", self._bytes(n, mask, torch.is_tensor(grad_high), torch.is_tensor(grad_low)) + reads,
                        "pyr_analyze_backward"))

    def synthesize(self, high, phase, amp, table, low, mask, flags, img):
        n = img.shape[0]
        tab = (ctypes.c_int * len(table))(*table) if table is not None else None
        _lib.call("vfi_pyr_synthesize", self._h, high.data_ptr() if torch.is_tensor(high) else None,
                  _ptr_array(phase), _ptr_array(amp) if amp is not None else None, tab,
                  low.data_ptr() if torch.is_tensor(low) else None, mask, flags, img.data_ptr(), n, _lib.stream_ptr(),
                  work=("byte", self._bytes(n, mask, torch.is_tensor(high), torch.is_tensor(low)), "pyr_synthesize"))


class Synthesis(torch.autograd.Function):
    """The pyramid's synthesis as an autograd node.  `layout` maps the flat inputs to the library's arguments:
    layout.forward(inputs) -> image, layout.backward(grad, inputs, needs) -> one gradient (or None) per input.  Inputs that
    are not tensors (the scalar 0 the reference uses for a missing level) get None."""

    @staticmethod
    def forward(ctx, layout, *inputs):
        ctx.layout = layout
        ctx.is_tensor = [torch.is_tensor(t) for t in inputs]
        ctx.save_for_backward(*[t for t in inputs if torch.is_tensor(t)])
        return layout.forward(inputs)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        saved = iter(ctx.saved_tensors)
        inputs = [next(saved) if t else 0 for t in ctx.is_tensor]
        needs = [bool(nd and t) for nd, t in zip(ctx.needs_input_grad[1:], ctx.is_tensor)]
        if not any(needs):
            return (None,) * (1 + len(inputs))
        return (None,) + tuple(ctx.layout.backward(grad.contiguous(), inputs, needs))


class Analysis(torch.autograd.Function):
    """The pyramid's analysis as an autograd node.  `layout` maps the library's arguments to flat outputs:
    layout.forward(img) -> tuple of output tensors, layout.saved(outputs) -> the ones the backward reads,
    layout.backward(saved, grads) -> gradient image, where grads holds one gradient per output, None for an output that the
    loss does not depend on (that output's level is then dropped from the backward's level mask)."""

    @staticmethod
    def forward(ctx, layout, img):
        outputs = layout.forward(img)
        ctx.layout = layout
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*layout.saved(outputs))
        return outputs

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return None, ctx.layout.backward(ctx.saved_tensors, [g.contiguous() if g is not None else None for g in grads])


class BandFilter(torch.autograd.Function):
    """Plan.band_filter / band_filter_pair as autograd nodes.  The gain G is real and even, so real(ifft2(fft2(x) * G)) is
    self-adjoint: the gradient of each image set is the same filter id applied to the output's gradient."""

    @staticmethod
    def forward(ctx, plan, specs, *imgs):
        ctx.plan, ctx.specs = plan, specs
        if len(imgs) == 1:
            return plan.band_filter(imgs[0], *specs[0])
        return plan.band_filter_pair(imgs[0], specs[0], imgs[1], specs[1])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        grad = grad.contiguous()
        return (None, None) + tuple(ctx.plan.band_filter(grad, *spec) if need else None
                                    for spec, need in zip(ctx.specs, ctx.needs_input_grad[2:]))


def wants_grad(inputs):
    """Whether a transform over `inputs` has to be recorded for autograd."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in inputs)


class _ComplexLayout:
    """reconstruct's inputs, flattened: hi (N,H,W), nlev x nb band coefficients (N,h,w,2) finest first, lo (N,hL,wL)."""

    def __init__(self, plan, nlev, nb):
        self.plan, self.nlev, self.nb = plan, nlev, nb

    def forward(self, inputs):
        nb = self.nb
        hi, lo = inputs[0].contiguous(), inputs[-1].contiguous()
        n, h, w = hi.shape
        bands = [torch.stack([b.contiguous() for b in inputs[1 + k * nb:1 + (k + 1) * nb]], 0) for k in range(self.nlev)]   # (nb, N, h, w, 2)
        img = torch.empty((n, h, w), dtype=torch.float32, device=hi.device)
        self.plan.synthesize(hi, bands, None, None, lo, (1 << self.nlev) - 1, BAND_MAJOR | COMPLEX_COEFF, img)
        return img

    def backward(self, grad, inputs, needs):
        nb, plan = self.nb, self.plan
        n = grad.shape[0]
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=grad.device)
        mask, gb = 0, []
        for k in range(self.nlev):
            if any(needs[1 + k * nb:1 + (k + 1) * nb]):
                mask |= 1 << k
                gb.append(new(nb, n, *plan.sizes[k], 2))
            else:
                gb.append(0)
        gh = new(*grad.shape) if needs[0] else None
        gl = new(n, *plan.sizes[self.nlev]) if needs[-1] else None
        plan.synthesize_backward(grad, None, None, None, mask, BAND_MAJOR | COMPLEX_COEFF, gh, gb, None, gl)
        out = [gh]
        for k in range(self.nlev):
            out += [gb[k][b] if needs[1 + k * nb + b] else None for b in range(nb)]
        return out + [gl]


class _ComplexAnalysisLayout:
    """build's outputs, flattened: hi (N,H,W), nlev x band coefficients (nb,N,h,w,2) finest first, lo (N,hL,wL)."""

    def __init__(self, plan, nlev, nb):
        self.plan, self.nlev, self.nb = plan, nlev, nb

    def forward(self, img):
        plan, nlev, nb = self.plan, self.nlev, self.nb
        n, h, w = img.shape
        self.n = n                      # (one layout per call of build)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=img.device)
        bands = [new(nb, n, *plan.sizes[k], 2) for k in range(nlev)]
        hi, lo = new(n, h, w), new(n, *plan.sizes[nlev])
        plan.analyze(img, hi, bands, None, None, lo, 1.0, (1 << nlev) - 1, BAND_MAJOR | COMPLEX_COEFF)
        return (hi, *bands, lo)

    def saved(self, outputs):
        return ()

    def backward(self, saved, grads):
        plan, nlev = self.plan, self.nlev
        ref = next(g for g in grads if g is not None)
        mask = sum(1 << k for k in range(nlev) if grads[1 + k] is not None)
        grad_img = torch.empty((self.n, plan.h, plan.w), dtype=torch.float32, device=ref.device)
        plan.analyze_backward(grads[0], list(grads[1:1 + nlev]), None, None, None, None, grads[-1], 1.0, mask,
                              BAND_MAJOR | COMPLEX_COEFF, grad_img)
        return grad_img


class SCFpyr_PyTorch(object):
    def __init__(self, height=5, nbands=4, scale_factor=2, device=None):
        self.height = height
        self.nbands = nbands
        self.scale_factor = scale_factor
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self._plans = {}

    def plan(self, h, w, n):
        """The cached plan of (h, w) for calls of n images.  A plan's max_images (16 at most) is the number of images one
        slice of a call holds: the library walks a longer call in slices, so the plan is rebuilt only when
        min(max(n, 6), 16) grows."""
        key = (h, w)
        want = min(max(n, 6), 16)
        p = self._plans.get(key)
        if p is None or p.max_images < want:
            p = Plan(h, w, self.height, self.nbands, self.scale_factor, want, self.device)
            self._plans[key] = p
        return p

    def build(self, im_batch):
        if im_batch.dim() != 4 or im_batch.shape[1] != 1:
            raise VfiLibraryError("build expects (N,1,H,W)")
        img = im_batch.squeeze(1).contiguous()
        n, h, w = img.shape
        plan = self.plan(h, w, n)
        nlev, nb = self.height - 2, self.nbands
        layout = _ComplexAnalysisLayout(plan, nlev, nb)
        hi, *bands, lo = Analysis.apply(layout, img) if wants_grad([img]) else layout.forward(img)
        return [hi] + [[b[i] for i in range(nb)] for b in bands] + [lo]

    def reconstruct(self, coeff):
        nb = self.nbands
        if nb != len(coeff[1]):
            raise Exception("Unmatched number of orientations")
        n, h, w = coeff[0].shape
        layout = _ComplexLayout(self.plan(h, w, n), len(coeff) - 2, nb)
        inputs = [coeff[0]] + [b for level in coeff[1:-1] for b in level] + [coeff[-1]]
        if wants_grad(inputs):
            return Synthesis.apply(layout, *inputs)
        return layout.forward(inputs)
