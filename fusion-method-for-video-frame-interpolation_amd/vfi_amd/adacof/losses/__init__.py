"""Loss of the AdaCoF trainer -- mirror of reference src/adacof/losses/__init__.py:6-72 (same class, same `weight*type`
grammar joined by `+`, same printed lines, same summation order).

`Loss(args)` reads `args.loss`; `forward(output, gt, input_frames)` takes the training dict of the network
({'frame1', 'g_Spatial', 'g_Occlusion'}), the target and the two input frames, and returns
`sum([w_0 * l_0(frame1, gt), ..., w_r * output[r], ...])` -- Python's `sum`, which starts from the int 0, terms first and
regularisers after them, each group in the order of the string.

`Module_MSELoss` / `Module_L1Loss` stand for the reference's `nn.MSELoss()` / `nn.L1Loss()`: one HIP autograd node each
(`vfi_mse_*`, `vfi_l1_*` with wrap off and scale 1: the fixed-order two-stage reduction of the Charbonnier node, one
streaming pass backward) when `utility._on_hip` holds, the plain torch expression otherwise.

Differences from the reference:

* `VGG` (losses/vgg.py) takes its weights from a file the user has -- `args.vgg_weights`, default the environment variable
  `VFI_VGG16_WEIGHTS` -- instead of downloading them; see vgg.py.
* The type `LPIPS` (not in the reference's grammar, e.g. `1*Charb+0.1*LPIPS`) is the mean over the batch of
  `vfi_amd.evaluation.lpips.LPIPS`, with `args.vgg_weights` as above and its head weights from `args.lpips_weights`,
  default `VFI_LPIPS_WEIGHTS`.  It is matched before the `VGG` substring test.
* The type `SSIM` (not in the reference's grammar either, e.g. `1*Charb+0.1*SSIM`) is
  `vfi_amd.evaluation.ssim.SSIMLoss(reduction='mean')`: the mean over the batch of 1 - SSIM, piq's defaults, no weights file.
* The types `GAN`, `WGAN` and `FI_GAN` build `adversarial.Adversarial(args, type)` (HIP discriminator),
  and `forward` hands `input_frames` to `FI_GAN`, as the reference does.  The classifier of the discriminator is sized by
  `args.patch_size`: an `args` without one raises NotImplementedError (the discriminator cannot be sized).  `WGAN_GP` (the
  critic without BatchNorm plus the gradient penalty) is built when `args.gradient_penalty` is true --
  the train script's `--gradient_penalty` -- and raises NotImplementedError without it; `T_WGAN_GP` always does (the temporal
  discriminator's Conv3d front end is not built, and the reference's own penalty branch cannot run it).  Any other unknown
  type raises ValueError; the reference fails there on an unbound name.
* The modules move to `cuda:<args.gpu_id>` (the reference: 'cuda', after `set_device(gpu_id)`), and stay where they are when
  there is no device, so the string can be parsed on a host.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..utility import Module_CharbonnierLoss, _on_hip

REGULARIZERS = ('g_Spatial', 'g_Occlusion', 'Lw', 'Ls')
VGG_WEIGHTS_ENV = 'VFI_VGG16_WEIGHTS'
LPIPS_WEIGHTS_ENV = 'VFI_LPIPS_WEIGHTS'


class _Mean(torch.autograd.Function):
    """mean(term(a - b)) as one node; term: 'mse' | 'l1'."""

    @staticmethod
    def forward(ctx, a, b, term):
        a, b = a.contiguous(), b.contiguous()
        ctx.term = term
        ctx.save_for_backward(a, b)
        return ops.mse_forward(a, b) if term == 'mse' else ops.l1_forward(a, b, wrap=False, scale=1.0)

    @staticmethod
    def backward(ctx, upstream):
        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[:2]
        if ctx.term == 'mse':
            ga, gb = ops.mse_backward(a, b, upstream.contiguous(), need_a=need_a, need_b=need_b)
        else:
            ga, gb = ops.l1_backward(a, b, upstream.contiguous(), wrap=False, scale=1.0, need_a=need_a, need_b=need_b)
        return ga, gb, None


def _mean(a, b, term):
    if a.shape != b.shape:
        a, b = torch.broadcast_tensors(a, b)
    if _on_hip(a, b):
        return _Mean.apply(a, b, term)
    return F.mse_loss(a, b) if term == 'mse' else F.l1_loss(a, b)


class Module_MSELoss(nn.Module):
    """mean((output - gt)^2): nn.MSELoss() (losses/__init__.py:17)."""

    def forward(self, output, gt):
        return _mean(output, gt, 'mse')


class Module_L1Loss(nn.Module):
    """mean(|output - gt|): nn.L1Loss() (losses/__init__.py:19)."""

    def forward(self, output, gt):
        return _mean(output, gt, 'l1')


class Loss(nn.modules.loss._Loss):
    def __init__(self, args):
        super(Loss, self).__init__()

        self.loss = []
        self.loss_module = nn.ModuleList()
        self.regularize = []

        for loss in args.loss.split('+'):
            weight, loss_type = loss.split('*')
            if loss_type == 'MSE':
                loss_function = Module_MSELoss()
            elif loss_type == 'L1':
                loss_function = Module_L1Loss()
            elif loss_type == 'Charb':
                loss_function = Module_CharbonnierLoss()
            elif loss_type == 'LPIPS':
                from ...evaluation.lpips import LPIPS
                loss_function = LPIPS(getattr(args, 'vgg_weights', None) or os.environ.get(VGG_WEIGHTS_ENV),
                                      getattr(args, 'lpips_weights', None) or os.environ.get(LPIPS_WEIGHTS_ENV),
                                      reduction='mean')
            elif loss_type == 'SSIM':
                from ...evaluation.ssim import SSIMLoss
                loss_function = SSIMLoss(reduction='mean')
            elif loss_type.find('VGG') >= 0:
                from .vgg import VGG
                loss_function = VGG(weights=getattr(args, 'vgg_weights', None) or os.environ.get(VGG_WEIGHTS_ENV))
            elif loss_type.find('GAN') >= 0:
                from .adversarial import TYPES, Adversarial, built_types
                built = built_types(args)       # TYPES, and WGAN_GP when args.gradient_penalty is true
                if loss_type not in built:
                    missing = "no temporal discriminator" if len(built) > len(TYPES) else "no gradient penalty, no temporal discriminator"
                    raise NotImplementedError(f"loss type {loss_type!r}: its discriminator is not built (only "
                                              f"{', '.join(built)}: {missing})")
                if getattr(args, 'patch_size', None) is None:
                    raise NotImplementedError(f"loss type {loss_type!r}: args has no patch_size, which sizes the "
                                              "discriminator's classifier")
                loss_function = Adversarial(args, loss_type)
            elif loss_type in REGULARIZERS:
                self.regularize.append({
                    'type': loss_type,
                    'weight': float(weight)}
                )
                continue
            else:
                raise ValueError(f"unknown loss type {loss_type!r} in {args.loss!r}")

            self.loss.append({
                'type': loss_type,
                'weight': float(weight),
                'function': loss_function}
            )

        for l in self.loss:
            if l['function'] is not None:
                print('{:.3f} * {}'.format(l['weight'], l['type']))
                self.loss_module.append(l['function'])

        for r in self.regularize:
            print('{:.3f} * {}'.format(r['weight'], r['type']))

        if torch.cuda.is_available():
            self.loss_module.to('cuda:{}'.format(getattr(args, 'gpu_id', torch.cuda.current_device())))

    def forward(self, output, gt, input_frames):
        losses = []
        for l in self.loss:
            if l['function'] is not None:
                if l['type'] == 'FI_GAN':
                    loss = l['function'](output['frame1'], gt, input_frames)
                else:
                    loss = l['function'](output['frame1'], gt)
                effective_loss = l['weight'] * loss
                losses.append(effective_loss)

        for r in self.regularize:
            effective_loss = r['weight'] * output[r['type']]
            losses.append(effective_loss)
        loss_sum = sum(losses)

        return loss_sum
