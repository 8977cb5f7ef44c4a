"""Train script of the AdaCoF network -- mirror of reference src/adacof/train.py:12-82:
`python -m vfi_amd.adacof.train --train <vimeo_triplet> --test_input <middlebury input> --gt <middlebury gt> ...`.

The reference's flags and defaults, plus `--vgg_weights` (a torchvision vgg16 state dict for a `VGG` term of `--loss`;
default: the environment variable VFI_VGG16_WEIGHTS), `--lpips_weights` (the head weights of an `LPIPS` term, which reads
`--vgg_weights` too; default: VFI_LPIPS_WEIGHTS), `--workers` (decoding threads of TripletLoader) and `--gradient_penalty`
(builds the `WGAN_GP` type of `--loss`, e.g. `--gradient_penalty --loss 1*Charb+0.005*WGAN_GP`; without it that type raises).
`--train_clips DIR` (with `--clip_stride`, `--matrix`, `--range`) trains from the `*.y4m` clips of DIR instead of `--train`,
with `--patch_size` as the crop (train/clipreader.py).

Differences from the reference:

* The batches come from `TripletLoader(dataset, rgb=True, lab=False)` instead of a `DataLoader(num_workers=0)`: the same
  dataset and the same draws of crop, flips and swap, prepared on the device.  `Trainer` takes either.
* `--model` names a module of `vfi_amd.adacof.models` (`adacofnet`); a dotted path is taken as it is.
* `--load` reads the checkpoint on the host (`map_location='cpu'`); `Model.load` copies it to the device.
"""
import argparse
import datetime
import os

import torch

from . import losses
from ..train import clipreader
from .models import Model
from .TestModule import Middlebury_other
from .trainer import Trainer

parser = argparse.ArgumentParser(description='AdaCoF-Pytorch')

# parameters
# Model Selection
parser.add_argument('--model', type=str, default='adacofnet')

# Hardware Setting
parser.add_argument('--gpu_id', type=int, default=0)

# Directory Setting
parser.add_argument('--train', type=str, default='./db/vimeo_triplet')
parser.add_argument('--out_dir', type=str, default='./output_adacof_train')
parser.add_argument('--load', type=str, default=None)
parser.add_argument('--test_input', type=str, default='./test_input/middlebury_others/input')
parser.add_argument('--gt', type=str, default='./test_input/middlebury_others/gt')
clipreader.add_arguments(parser)       # --train_clips PATH [--clip_stride N --matrix M --range R]: train from .y4m clips

# Learning Options
parser.add_argument('--epochs', type=int, default=50, help='Max Epochs')
parser.add_argument('--batch_size', type=int, default=4, help='Batch size')
parser.add_argument('--loss', type=str, default='1*Charb+0.01*g_Spatial+0.005*g_Occlusion', help='loss function configuration')
parser.add_argument('--patch_size', type=int, default=256, help='Patch size')
parser.add_argument('--vgg_weights', type=str, default=os.environ.get(losses.VGG_WEIGHTS_ENV),
                    help='torchvision vgg16 state dict for a VGG term (default: $VFI_VGG16_WEIGHTS)')
parser.add_argument('--lpips_weights', type=str, default=os.environ.get(losses.LPIPS_WEIGHTS_ENV),
                    help='LPIPS head weights for an LPIPS term (default: $VFI_LPIPS_WEIGHTS)')
parser.add_argument('--workers', type=int, default=4, help='decoding threads')
parser.add_argument('--gradient_penalty', action='store_true', help='build the WGAN_GP loss type (critic without BatchNorm + gradient penalty)')

# Optimization specifications
parser.add_argument('--lr', type=float, default=0.001, help='learning rate')
parser.add_argument('--lr_decay', type=int, default=20, help='learning rate decay per N epochs')
parser.add_argument('--decay_type', type=str, default='step', help='learning rate decay type')
parser.add_argument('--gamma', type=float, default=0.5, help='learning rate decay factor for step decay')
parser.add_argument('--optimizer', default='ADAMax', choices=('SGD', 'ADAM', 'RMSprop', 'ADAMax'), help='optimizer to use (SGD | ADAM | RMSprop | ADAMax)')
parser.add_argument('--weight_decay', type=float, default=0, help='weight decay')
parser.add_argument('--device_optimizer', action='store_true', help='optimiser steps (the discriminators\' too) in one HIP pass (vfi_amd.optim)')

# Options for AdaCoF
parser.add_argument('--kernel_size', type=int, default=5)
parser.add_argument('--dilation', type=int, default=1)


def main(argv=None):
    args = parser.parse_args(argv)
    torch.cuda.set_device(args.gpu_id)
    device = torch.device(f'cuda:{args.gpu_id}')
    if '.' not in args.model:
        args.model = 'vfi_amd.adacof.models.' + args.model

    dataset, train_loader = clipreader.training_input(args, (args.patch_size, args.patch_size), device, rgb=True, lab=False)
    TestDB = Middlebury_other(args.test_input, args.gt, device=device)
    model = Model(args)
    loss = losses.Loss(args)

    start_epoch = 0
    if args.load is not None:
        checkpoint = torch.load(args.load, map_location='cpu')
        model.load(checkpoint['state_dict'])
        start_epoch = checkpoint['epoch']

    my_trainer = Trainer(args, train_loader, TestDB, model, loss, start_epoch)

    now = datetime.datetime.now().strftime('%Y-%m-%d-%H:%M:%S')
    with open(args.out_dir + '/config.txt', 'a') as f:
        f.write(now + '\n\n')
        for arg in vars(args):
            f.write('{}: {}\n'.format(arg, getattr(args, arg)))
        f.write('\n')

    while not my_trainer.terminate():
        my_trainer.train()
        my_trainer.test()

    my_trainer.close()


if __name__ == "__main__":
    main()
