"""Train script of FusionNet -- mirror of reference src/fusion_net/train.py:22-145:
`python -m vfi_amd.fusion_net.train --train <vimeo_triplet> ...`.

The reference's flags and defaults, plus `--out_dir` (default: the reference's `./output_fusion_net_3_no_uncertainty_map`),
`--crop H W` (256 256), `--height` (12), `--workers`, `--phasenet_checkpoint`, `--adacof_checkpoint` (defaults: the
reference's paths), `--test_paths A B C`, and `--lpips_weight` (0) with `--vgg_weights` / `--lpips_weights` (defaults: the
environment variables VFI_VGG16_WEIGHTS / VFI_LPIPS_WEIGHTS) for the perceptual term of trainer.py, and `--ssim_weight` (0) for
its structural term (evaluation/ssim.py; no weights file).  `--train_clips DIR` (with `--clip_stride`, `--matrix`, `--range`)
trains from the `*.y4m` clips of DIR instead of `--train` (train/clipreader.py).  `--save` is accepted and raises NotImplementedError (trainer.py).

The network is `FusionNet(kernel, pad, dil)` with its default three uncertainty maps, which `Trainer.predict` feeds it; the
reference's script builds `FusionNet(uncertainty_maps=0)` (train.py:79), whose first convolution has three input channels
fewer than its own forward concatenates."""
import argparse
import os
import random

import numpy as np
import torch

from ..phase_net.phase_net import PhaseNet
from ..train import clipreader
from ..train.pyramid import Pyramid
from ..train.train import finish, write_config
from ..train.trainer import ADACOF_CHECKPOINT, load_adacof
from .fusion_net import FusionNet
from .trainer import Trainer

parser = argparse.ArgumentParser(description='FusionNet-Pytorch')

# Hardware Setting
parser.add_argument('--gpu_id', type=int, default=1)

# Directory Setting
parser.add_argument('--train', type=str, default='./Trainset/vimeo/vimeo_triplet')
parser.add_argument('--load', type=str, default=None)
parser.add_argument('--out_dir', type=str, default=None)
clipreader.add_arguments(parser)       # --train_clips PATH [--clip_stride N --matrix M --range R]: train from .y4m clips

# Learning Options
parser.add_argument('--epochs', type=int, default=1, help='max epochs')
parser.add_argument('--batch_size', type=int, default=16, help='batch size')
parser.add_argument('--seed', type=int, default=0, help='seed')
parser.add_argument('--crop', type=int, nargs=2, default=(256, 256), metavar=('H', 'W'), help='random crop')
parser.add_argument('--height', type=int, default=12, help='height of the pyramid')
parser.add_argument('--workers', type=int, default=4, help='decoding threads')

# Optimization specifications
parser.add_argument('--lr', type=float, default=1e-4, help='learning rate')
parser.add_argument('--lr_decay', type=int, default=0, help='learning rate decay per N epochs')
parser.add_argument('--weight_decay', type=float, default=0, help='weight decay')
parser.add_argument('--device_optimizer', action='store_true', help='optimiser step in one HIP pass (vfi_amd.optim.Adam)')

# Save Residuals
parser.add_argument('--save', type=bool, default=False, help='Save Residuals or not')

# Fusion model settings
parser.add_argument('--dilation', type=int, default=3, help='Dilation size for kernel')
parser.add_argument('--kernel', type=int, default=3, help='Kernel size')
parser.add_argument('--pad', type=int, default=3, help='Padding for kernel size')

parser.add_argument('--phasenet_checkpoint', type=str, default='src/phase_net/phase_net.pt')
parser.add_argument('--adacof_checkpoint', type=str, default=ADACOF_CHECKPOINT)
parser.add_argument('--test_paths', type=str, nargs=3, default=None, metavar=('A', 'B', 'C'))

# Perceptual term: loss = l1 + lpips_weight * mean LPIPS(clip(prediction), target)
parser.add_argument('--lpips_weight', type=float, default=0.0, help='weight of the LPIPS term (0: none)')
parser.add_argument('--vgg_weights', type=str, default=os.environ.get('VFI_VGG16_WEIGHTS'),
                    help='torchvision vgg16 state dict (default: $VFI_VGG16_WEIGHTS)')
parser.add_argument('--lpips_weights', type=str, default=os.environ.get('VFI_LPIPS_WEIGHTS'),
                    help='LPIPS head weights (default: $VFI_LPIPS_WEIGHTS)')

# Structural term: loss += ssim_weight * mean (1 - SSIM(clip(prediction), target)); needs no weights file
parser.add_argument('--ssim_weight', type=float, default=0.0, help='weight of the SSIM term (0: none)')


def main(argv=None):
    args = parser.parse_args(argv)
    if args.save:
        raise NotImplementedError("--save: the dump of FusionNet's residual sums is not built")
    torch.cuda.set_device(args.gpu_id)
    out_dir = args.out_dir or "./output_fusion_net_3_no_uncertainty_map"

    # RNG init
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    device = torch.device(f'cuda:{args.gpu_id}')
    dataset, train_loader = clipreader.training_input(args, tuple(args.crop), device)

    pyr = Pyramid(height=args.height, nbands=4, scale_factor=np.sqrt(2), device=device)
    fusion_net = FusionNet(kernel=args.kernel, pad=args.pad, dil=args.dilation).to(device)

    phase_net = PhaseNet(pyr, device, num_img=2)
    phase_net.eval()
    phase_net.load_state_dict(torch.load(args.phasenet_checkpoint, map_location='cpu'))
    adacof_model = load_adacof(args.gpu_id, args.adacof_checkpoint)

    start_epoch = 0
    if args.load is not None:
        fusion_net.load_state_dict(torch.load(args.load, map_location='cpu'))

    my_trainer = Trainer(args, train_loader, fusion_net, phase_net, adacof_model, my_pyr=pyr, lr=args.lr,
                         weight_decay=args.weight_decay, start_epoch=start_epoch, out_dir=out_dir)
    write_config(out_dir, args)

    while not my_trainer.terminate():
        my_trainer.train()
        torch.save(fusion_net.state_dict(), out_dir + f'/checkpoint/model_{my_trainer.current_epoch}.pt')

    finish(my_trainer)


if __name__ == "__main__":
    main()
