"""Train script of PhaseNet and the pyramid-domain fusion PhaseNets -- mirror of reference src/train/train.py:20-137:
`python -m vfi_amd.train.train --train <vimeo_triplet> [--mode phase|fusion] ...`.

The reference's flags and defaults, plus `--out_dir` (default: the reference's `./output_<mode>_net...`), `--crop H W`
(256 256), `--height` (12, the pyramid's), `--workers` (decoding threads of TripletLoader), `--fixed_stats` (fine-tune on the
checkpoint's BatchNorm statistics instead of training on the batch's), `--adacof_checkpoint`, `--adacof_config` (accepted for
the reference's sake; the fusion variant of AdaCoFNet takes no config file) and `--test_paths A B C` (frame 1, target,
frame 2 of the picture `Trainer.test` writes every 100 batches).  `--train_clips DIR` (with `--clip_stride`, `--matrix`,
`--range`) trains from the `*.y4m` clips of DIR instead of `--train` (clipreader.py).  No plots; see trainer.py for the other differences."""
import argparse
import datetime
import os
import random

import numpy as np
import torch

from ..phase_net.architecture import PhaseNet
from . import clipreader
from .pyramid import Pyramid
from .trainer import ADACOF_CHECKPOINT, Trainer

parser = argparse.ArgumentParser(description='PhaseNet-Pytorch')

# Hardware Setting
parser.add_argument('--gpu_id', type=int, default=0)

# Directory Setting
parser.add_argument('--train', type=str, default='./Trainset/vimeo/vimeo_triplet')
parser.add_argument('--load', type=str, default=None)
parser.add_argument('--out_dir', type=str, default=None)
clipreader.add_arguments(parser)       # --train_clips PATH [--clip_stride N --matrix M --range R]: train from .y4m clips

# Learning Options
parser.add_argument('--epochs', type=int, default=1, help='max epochs')
parser.add_argument('--batch_size', type=int, default=8, help='batch size')
parser.add_argument('--seed', type=int, default=0, help='seed')
parser.add_argument('--m', type=int, default=None, help='layers to train from 0 to m')
parser.add_argument('--m_update', type=int, default=500, help='number of batches after updating m')
parser.add_argument('--crop', type=int, nargs=2, default=(256, 256), metavar=('H', 'W'), help='random crop')
parser.add_argument('--height', type=int, default=12, help='height of the pyramid')
parser.add_argument('--workers', type=int, default=4, help='decoding threads')
parser.add_argument('--fixed_stats', action='store_true', help='BatchNorm on the running statistics (fine-tuning)')

# Optimization specifications
parser.add_argument('--lr', type=float, default=1e-3, help='learning rate')
parser.add_argument('--lr_decay', type=int, default=0, help='learning rate decay per N epochs')
parser.add_argument('--weight_decay', type=float, default=0, help='weight decay')
parser.add_argument('--device_optimizer', action='store_true', help='optimiser step in one HIP pass (vfi_amd.optim.Adam)')

# Method Settings
parser.add_argument('--mode', type=str, default='phase', help='phase, fusion')
parser.add_argument('--high_level', type=bool, default=False, help='replace high-level with adacof output or not')
parser.add_argument('--model', type=int, default=0, help='Define which fusion model')
parser.add_argument('--adacof_checkpoint', type=str, default=ADACOF_CHECKPOINT)
parser.add_argument('--adacof_config', type=str, default='src/adacof/checkpoint/kernelsize_5/config.txt')
parser.add_argument('--test_paths', type=str, nargs=3, default=None, metavar=('A', 'B', 'C'))


def write_config(out_dir, args):
    now = datetime.datetime.now().strftime('%Y-%m-%d-%H:%M:%S')
    with open(out_dir + '/config.txt', 'a') as f:
        f.write(now + '\n\n')
        for arg in vars(args):
            f.write('{}: {}\n'.format(arg, getattr(args, arg)))
        f.write('\n')


def finish(trainer):
    """train.py:119-124 without the plot: the running log goes, the whole history stays."""
    if os.path.exists(trainer.out_dir + '/log_train.txt'):
        os.remove(trainer.out_dir + '/log_train.txt')
    trainer.close()
    np.savetxt(trainer.out_dir + '/log.txt', np.asarray(trainer.loss_history))


def main(argv=None):
    args = parser.parse_args(argv)
    torch.cuda.set_device(args.gpu_id)
    hl_str = '_hl' if args.high_level else ''
    fusion_model = '_' + str(args.model) if args.model != 0 else ''
    out_dir = args.out_dir or f"./output_{args.mode}_net{hl_str}{fusion_model}"

    # RNG init
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    device = torch.device(f'cuda:{args.gpu_id}')
    needs_rgb = args.mode == 'fusion' or args.high_level
    dataset, train_loader = clipreader.training_input(args, tuple(args.crop), device, rgb=needs_rgb)

    pyr = Pyramid(height=args.height, nbands=4, scale_factor=np.sqrt(2), device=device)
    if args.mode == 'fusion':
        num = 4 if args.model == 0 else 3
    else:
        num = 2
    model = PhaseNet(args.height, device, num_img=num)
    m = 10 if args.m is None else args.m

    start_epoch = 0
    if args.load is not None:
        model.load_state_dict(torch.load(args.load, map_location='cpu'))

    my_trainer = Trainer(args, train_loader, model, pyr=pyr, lr=args.lr, weight_decay=args.weight_decay,
                         start_epoch=start_epoch, out_dir=out_dir, m=m, m_update=args.m_update)
    write_config(out_dir, args)

    while not my_trainer.terminate():
        my_trainer.train()
        torch.save(model.state_dict(), out_dir + f'/checkpoint/model_{my_trainer.current_epoch}.pt')

    finish(my_trainer)


if __name__ == "__main__":
    main()
