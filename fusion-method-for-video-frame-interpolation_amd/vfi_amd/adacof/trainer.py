"""Trainer of the AdaCoF network -- mirror of reference src/adacof/trainer.py:7-67.

`Trainer(args, train_loader, test_loader, my_model, my_loss, start_epoch=0)` with `train()`, `test()`, `terminate()` and
`close()`.  It makes `args.out_dir/{result, checkpoint, log.txt}`, runs the initial test in the constructor, prints every 100
batches in the reference's format, steps the scheduler once per epoch and saves `{'epoch', 'state_dict'}` as
`checkpoint/model_epoch%03d.pth` before each test.

`train_loader` is the reference's stock `DataLoader` over `DBreader_Vimeo90k` (three (B, 3, h, w) CPU tensors per batch,
uploaded here as `to_variable` does), or a `TripletLoader(..., rgb=True, lab=False)`, whose batches are already on the device
(decode ahead, crop, flips and swap in one launch: DESIGN.md section 22).

Differences from the reference:

* `loss_history` (the floats of every step so far) is kept, as the other trainers keep it; the loss goes to the host only
  where it is printed and when the history is read (train/trainer.py: LossHistory).
* The tensors are uploaded to the model's device, not to the current one.
"""
import os

import torch

from ..train.trainer import LossHistory
from . import utility

LOG_EVERY = 100


class Trainer:
    def __init__(self, args, train_loader, test_loader, my_model, my_loss, start_epoch=0):
        self.args = args
        self.train_loader = train_loader
        self.max_step = self.train_loader.__len__()
        self.test_loader = test_loader
        self.model = my_model
        self.loss = my_loss
        self.current_epoch = start_epoch
        self.device = next(self.model.parameters()).device

        self.optimizer = utility.make_optimizer(args, self.model)
        self.scheduler = utility.make_scheduler(args, self.optimizer)

        if not os.path.exists(args.out_dir):
            os.makedirs(args.out_dir)
        self.result_dir = args.out_dir + '/result'
        self.ckpt_dir = args.out_dir + '/checkpoint'

        if not os.path.exists(self.result_dir):
            os.makedirs(self.result_dir)
        if not os.path.exists(self.ckpt_dir):
            os.makedirs(self.ckpt_dir)

        self.logfile = open(args.out_dir + '/log.txt', 'w')
        self._losses = LossHistory()

        # Initial Test
        self.model.eval()
        self.test_loader.Test(self.model, self.result_dir, self.current_epoch, self.logfile, str(self.current_epoch).zfill(3) + '.png')

    @property
    def loss_history(self):
        return self._losses.flush()

    def _unpack(self, batch):
        """-> frame0, frame1 (the target), frame2: (B, 3, h, w) on the device"""
        if hasattr(batch, 'rgb'):
            if batch.rgb is None:
                raise ValueError("Trainer: the TripletLoader must be made with rgb=True")
            return batch.rgb_frame1, batch.rgb_target, batch.rgb_frame2
        frame0, frame1, frame2 = batch
        return frame0.to(self.device), frame1.to(self.device), frame2.to(self.device)

    def train(self):
        # Train
        self.model.train()
        for batch_idx, batch in enumerate(self.train_loader):
            frame0, frame1, frame2 = self._unpack(batch)

            self.optimizer.zero_grad()

            output = self.model(frame0, frame2)
            loss = self.loss(output, frame1, [frame0, frame2])
            loss.backward()
            self.optimizer.step()
            self._losses.append(loss)

            if batch_idx % LOG_EVERY == 0:
                print('{:<13s}{:<14s}{:<6s}{:<16s}{:<12s}{:<20.16f}'.format('Train Epoch: ', '[' + str(self.current_epoch) + '/' + str(self.args.epochs) + ']', 'Step: ', '[' + str(batch_idx) + '/' + str(self.max_step) + ']', 'train loss: ', loss.item()))
        self.current_epoch += 1
        self.scheduler.step()

    def test(self):
        # Test
        torch.save({'epoch': self.current_epoch, 'state_dict': self.model.get_state_dict()}, self.ckpt_dir + '/model_epoch' + str(self.current_epoch).zfill(3) + '.pth')
        self.model.eval()
        self.test_loader.Test(self.model, self.result_dir, self.current_epoch, self.logfile, str(self.current_epoch).zfill(3) + '.png')
        self.logfile.write('\n')

    def terminate(self):
        return self.current_epoch >= self.args.epochs

    def close(self):
        self.logfile.close()
