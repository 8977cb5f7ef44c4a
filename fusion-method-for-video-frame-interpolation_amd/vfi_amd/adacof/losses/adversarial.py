"""Adversarial terms of the AdaCoF trainer -- mirror of reference src/adacof/losses/adversarial.py:10-97 for the types `GAN`,
`WGAN` and `FI_GAN`.

`Adversarial(args, gan_type)` owns a discriminator (discriminator.py), its optimiser and scheduler (`utility.make_optimizer` /
`make_scheduler` with the trainer's own `args`).  `forward(fake, real, input_frames=None)` first updates the discriminator
`gan_k` (= 1) times on `fake.detach()`:

* `GAN`:    BCE-with-logits(D(fake), 0) + BCE-with-logits(D(real), 1);
* `WGAN`:   mean(D(fake) - D(real)), and after the step every parameter is clamped to [-1, 1];
* `FI_GAN`: BCE-with-logits(D(frame0, fake), 0) + BCE-with-logits(D(fake, frame2), 1);

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
* `WGAN_GP` and `T_WGAN_GP` raise NotImplementedError (gradient penalty: a double backward through every kernel; temporal
  discriminator: a Conv3d front end, and the reference's own forward calls its three-argument discriminator with one).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import utility
from . import discriminator

TYPES = ('GAN', 'WGAN', 'FI_GAN')


class Adversarial(nn.Module):
    def __init__(self, args, gan_type):
        super(Adversarial, self).__init__()
        if gan_type not in TYPES:
            raise NotImplementedError(f"Adversarial: gan_type {gan_type!r}: only {', '.join(TYPES)} have a discriminator built")
        self.gan_type = gan_type
        self.gan_k = 1
        if gan_type == 'FI_GAN':
            self.discriminator = discriminator.FI_Discriminator(args)
        else:
            self.discriminator = discriminator.Discriminator(args, gan_type)
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

            # Discriminator update
            self.loss = self.loss + loss_d.detach()
            loss_d.backward()
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
