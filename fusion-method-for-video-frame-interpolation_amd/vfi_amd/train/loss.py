"""PhaseNet's loss -- mirror of reference src/train/loss.py:5-26 (same name, signature and return values).

Per level the reference's double loop over the orientations equals nbands * mean |wrap(phase_t - phase_o)| over the whole
level (every orientation holds the same number of coefficients), wrap(d) = atan2(sin d, cos d).  For HIP fp32 tensors of
which one requires grad, each level's term and the L1 term run as one HIP autograd node (`vfi_l1_forward`: a two-stage
reduction in an order fixed by the element count; `vfi_l1_backward`: one streaming pass); any other arguments (CPU
tensors, float64, nothing requiring grad) take the reference's torch expression.
"""
import torch

from .. import ops


class _AbsMean(torch.autograd.Function):
    """scale * mean |w(a - b)|, w = wrap or the identity."""

    @staticmethod
    def forward(ctx, a, b, wrap, scale):
        a, b = a.contiguous(), b.contiguous()
        ctx.wrap, ctx.scale = wrap, scale
        ctx.save_for_backward(a, b)
        return ops.l1_forward(a, b, wrap, scale)

    @staticmethod
    def backward(ctx, upstream):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[:2]
        ga, gb = ops.l1_backward(a, b, upstream.contiguous(), ctx.wrap, ctx.scale, need_a=need_a, need_b=need_b)
        return ga, gb, None, None


def _on_hip(a, b):
    return (torch.is_grad_enabled() and a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32
            and a.shape == b.shape and (a.requires_grad or b.requires_grad))


def phase_term(phase_o, phase_t, nbands):
    """One level's term of the phase loss (loss.py:11-16): the sum over the orientations of the mean |delta_psi|."""
    if _on_hip(phase_t, phase_o):
        return _AbsMean.apply(phase_t, phase_o, True, float(nbands))
    d = phase_t - phase_o
    return nbands * torch.mean(torch.abs(torch.atan2(torch.sin(d), torch.cos(d))))


def l1_loss(output, target):
    """nn.L1Loss() (loss.py:8,20)."""
    if _on_hip(output, target):
        return _AbsMean.apply(output, target, False, 1.0)
    return torch.nn.functional.l1_loss(output, target)


def get_loss(vals_o, vals_t, output, target, pyr, weighting_factor=0.005):
    """PhaseNet special loss (loss.py:5-26) -> (total_loss, l_1_p, phase_loss_p)."""
    phase_loss = 0
    for phase_r, phase_g in zip(vals_o.phase, vals_t.phase):
        if phase_r.numel() % pyr.nbands:
            raise ValueError(f"get_loss: a level of {tuple(phase_r.shape)} does not hold {pyr.nbands} orientations per image")
        phase_loss = phase_loss + phase_term(phase_r, phase_g, pyr.nbands)
    l_1 = l1_loss(output, target)

    total_loss = l_1 + weighting_factor * phase_loss
    l_1_p = 100 * l_1.detach() / total_loss
    phase_loss_p = 100 * weighting_factor * phase_loss.detach() / total_loss
    return total_loss, l_1_p, phase_loss_p
