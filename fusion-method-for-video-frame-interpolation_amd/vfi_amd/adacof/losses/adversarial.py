"""Adversarial terms of the AdaCoF trainer -- mirror of reference src/adacof/losses/adversarial.py:10-97 for the types `GAN`,
`WGAN`, `FI_GAN` and, when `args.gradient_penalty` is true, `WGAN_GP`.

`Adversarial(args, gan_type)` owns a discriminator (discriminator.py), its optimiser and scheduler (`utility.make_optimizer` /
`make_scheduler` with the trainer's own `args`).  `forward(fake, real, input_frames=None)` first updates the discriminator
`gan_k` (= 1) times on `fake.detach()`:

* `GAN`:    BCE-with-logits(D(fake), 0) + BCE-with-logits(D(real), 1);
* `WGAN`:   mean(D(fake) - D(real)), and after the step every parameter is clamped to [-1, 1];
* `FI_GAN`: BCE-with-logits(D(frame0, fake), 0) + BCE-with-logits(D(fake, frame2), 1);
* `WGAN_GP`: mean(D(fake) - D(real)) + 10 mean_b((||grad D(hat_b)||_2 - 1)^2), hat = fake (1 - e) + real e with
  e = `torch.rand_like(fake)`; the discriminator has no BatchNorm, its optimiser is the reference's
  `Adam(betas=(0, 0.9), eps=1e-8, lr=1e-5)` whatever `args.optimizer` says, and nothing is clamped.  On fp32 device tensors
  hat is `ops.gp_mix` (the bits of that torch expression), the gradient `discriminator.input_gradient(hat)` and the penalty
  one autograd node over `ops.grad_penalty_forward` / `_backward`; elsewhere the torch expressions;

the fake and the real batch go through the discriminator in separate calls, each with its own batch statistics.  Then it
returns the generator's term from a third forward through the updated discriminator: BCE-with-logits(D(fake), 1),
-mean(D(fake)), or for `FI_GAN` mean(s01 log(s01 + 1e-12) + s12 log(s12 + 1e-12)) with s = sigmoid(D(.)).

`FI_GAN` evaluates its generator term on `fake.detach()`, as the reference does (adversarial.py:87-88): the term is a number
that sends NO gradient to the frame.  That is kept, not repaired; `fake.grad` is left untouched by it.

The loss arithmetic on the B logits is torch's; the discriminator runs the HIP node of discriminator.py.

Differences from the reference:

* `self.loss` (the mean discriminator loss of the call) stays a 0-d device tensor until it is read (`float(adv.loss)`); the
  reference calls `.item()` in every step.
* The generator's pass goes through `discriminator.frozen()`: it forms no discriminator weight gradients.  The reference
  accumulates them into `.grad` and zeroes them at the next call before any use.
* With a true `args.device_optimizer` the discriminator's optimiser is the `vfi_amd.optim` subclass of the same torch class
  (the fixed Adam of `WGAN_GP` too), and `WGAN` hands its clamp to that step (`step(clamp=(-1, 1))`: the parameters that
  took the step are clamped in the same pass, any parameter without a grad by the torch call) instead of looping over all.
* `WGAN_GP` is built only with `args.gradient_penalty` (the train script's `--gradient_penalty`); without it, and always for
  `T_WGAN_GP`, NotImplementedError (temporal discriminator: a Conv3d front end, and the reference's own penalty branch calls
  its three-argument discriminator with one).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ... import optim as device_optim
from .. import utility
from . import discriminator

TYPES = ('GAN', 'WGAN', 'FI_GAN')
GP_TYPES = ('WGAN_GP',)         # built when args.gradient_penalty is true
GP_WEIGHT = 10.0


def built_types(args):
    """The gan types `Adversarial(args, .)` builds."""
    return TYPES + (GP_TYPES if getattr(args, 'gradient_penalty', False) else ())


class _GradPenalty(torch.autograd.Function):
    """weight * mean_b (||g_b||_2 - 1)^2 of g (B, ...) as one node."""

    @staticmethod
    def forward(ctx, g, weight):
        g = g.contiguous()
        value, norms = ops.grad_penalty_forward(g, weight)
        ctx.weight = weight
        ctx.save_for_backward(g, norms)
        return value

    @staticmethod
    def backward(ctx, upstream):
        g, norms = ctx.saved_tensors
        return ops.grad_penalty_backward(g, norms, upstream.contiguous(), ctx.weight), None


def gradient_penalty(gradients, weight=GP_WEIGHT):
    """Reference adversarial.py:65-67: weight * mean((||gradients_b||_2 - 1)^2)."""
    if utility._on_hip(gradients):
        return _GradPenalty.apply(gradients, float(weight))
    gradient_norm = gradients.view(gradients.size(0), -1).norm(2, dim=1)
    return weight * gradient_norm.sub(1).pow(2).mean()


def interpolate(fake, real, epsilon):
    """Reference adversarial.py:58: fake (1 - epsilon) + real epsilon."""
    if all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in (fake, real, epsilon)):
        return ops.gp_mix(fake.contiguous(), real.contiguous(), epsilon)
    return fake.mul(1 - epsilon) + real.mul(epsilon)


class Adversarial(nn.Module):
    def __init__(self, args, gan_type):
        super(Adversarial, self).__init__()
        if gan_type not in built_types(args):
            raise NotImplementedError(f"Adversarial: gan_type {gan_type!r}: only {', '.join(built_types(args))} have a discriminator built")
        self.gan_type = gan_type
        self.gan_k = 1
        self.device_optimizer = bool(getattr(args, 'device_optimizer', False))
        if gan_type == 'FI_GAN':
            self.discriminator = discriminator.FI_Discriminator(args)
        else:
            self.discriminator = discriminator.Discriminator(args, gan_type)
        if gan_type in GP_TYPES:
            adam = device_optim.Adam if self.device_optimizer else torch.optim.Adam
            self.optimizer = adam(self.discriminator.parameters(), betas=(0.0, 0.9), eps=1e-8, lr=1e-5)
        else:
            self.optimizer = utility.make_optimizer(args, self.discriminator)
        self.scheduler = utility.make_scheduler(args, self.optimizer)
        self.loss = 0

    def forward(self, fake, real, input_frames=None):
        fake_detach = fake.detach()

        self.loss = 0
        for _ in range(self.gan_k):
            self.optimizer.zero_grad()
            if self.gan_type == 'FI_GAN':
                d_01 = self.discriminator(input_frames[0], fake_detach)
                d_12 = self.discriminator(fake_detach, input_frames[1])
            else:
                d_fake = self.discriminator(fake_detach)
                d_real = self.discriminator(real)

            if self.gan_type == 'GAN':
                label_fake = torch.zeros_like(d_fake)
                label_real = torch.ones_like(d_real)
                loss_d = F.binary_cross_entropy_with_logits(d_fake, label_fake) + F.binary_cross_entropy_with_logits(d_real, label_real)
            elif self.gan_type == 'FI_GAN':
                label_01 = torch.zeros_like(d_01)
                label_12 = torch.ones_like(d_12)
                loss_d = F.binary_cross_entropy_with_logits(d_01, label_01) + F.binary_cross_entropy_with_logits(d_12, label_12)
            else:
                loss_d = (d_fake - d_real).mean()
                if self.gan_type in GP_TYPES:
                    epsilon = torch.rand_like(fake)
                    hat = interpolate(fake_detach, real, epsilon)
                    gradients = self.discriminator.input_gradient(hat)
                    loss_d = loss_d + gradient_penalty(gradients, GP_WEIGHT)

            # Discriminator update
            self.loss = self.loss + loss_d.detach()
            loss_d.backward()
            if self.gan_type == 'WGAN' and self.device_optimizer:
                rest = [p for p in self.discriminator.parameters() if p.grad is None]
                self.optimizer.step(clamp=(-1, 1))      # clamped in the pass that writes the update
                for p in rest:                          # none today: every parameter has a grad
                    p.data.clamp_(-1, 1)
                continue
            self.optimizer.step()

            if self.gan_type == 'WGAN':
                for p in self.discriminator.parameters():
                    p.data.clamp_(-1, 1)

        self.loss = self.loss / self.gan_k

        with self.discriminator.frozen():
            if self.gan_type == 'GAN':
                d_fake_for_g = self.discriminator(fake)
                loss_g = F.binary_cross_entropy_with_logits(
                    d_fake_for_g, label_real
                )
            elif self.gan_type == 'FI_GAN':
                d_01_for_g = torch.sigmoid(self.discriminator(input_frames[0], fake_detach))
                d_12_for_g = torch.sigmoid(self.discriminator(fake_detach, input_frames[1]))
                loss_g = d_01_for_g * torch.log(d_01_for_g + 1e-12) + d_12_for_g * torch.log(d_12_for_g + 1e-12)
                loss_g = loss_g.mean()
            else:
                d_fake_for_g = self.discriminator(fake)
                loss_g = -d_fake_for_g.mean()

        # Generator loss
        return loss_g
