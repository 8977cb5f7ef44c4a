"""Trainer of FusionNet -- mirror of reference src/fusion_net/trainer.py:25-345.

`Trainer(args, train_loader, fusion_net, phase_net, adacof_model, my_pyr, lr, weight_decay, start_epoch, out_dir)`; only
`fusion_net` is trained (Adam on its parameters); PhaseNet and AdaCoF produce its inputs under no_grad through
`train_batch.fusion_net_inputs`, which is the reference's `predict` up to the call of the network.  The loss is
`l1(target_rgb, clip(final, 0, 1))` (trainer.py:246-254), plus `args.lpips_weight * mean LPIPS(clip(final, 0, 1), target_rgb)`
when that weight is not 0 (evaluation/lpips.py, built from `args.vgg_weights` and `args.lpips_weights`; the reference imports
LPIPS at trainer.py:13 and trains with L1 alone); at 0 nothing is built and the step is the reference's.  Likewise
`args.ssim_weight * SSIMLoss(clip(final, 0, 1), target_rgb)` (evaluation/ssim.py: the mean of 1 - SSIM over the batch; piq's
SSIMLoss is imported on the same line of the reference), added after the LPIPS term; at 0 nothing is built.  `train_loader`
yields `datareader.TripletBatch`es, or the reference's triples of (B, 3, h, w) CPU tensors.

Differences from the reference:

* `test()` keeps FusionNet's mode as it found it (the reference leaves it in `train()`), reads its three images with PIL and
  returns silently when `paths` is None or a file is missing; `train()` passes `args.test_paths`.
* The running checkpoint, written every 50 batches with the log, is `model_<epoch>_<batch_idx // 50>.pt`; the reference
  divides by 100 there (trainer.py:273), so two consecutive ones share a name.
* No plots, no debug pictures.  The text logs are kept.
* `args.save` (the dump of the residual sums) raises NotImplementedError: the trainable forward keeps no residuals.
* The loss goes to the host only where it is logged and at the end of the epoch (train/trainer.py: LossHistory).
"""
import os

import numpy as np
import torch

from ..train.trainer import LossHistory, read_test_images, save_image
from ..train.utils import preprocess
from .train_batch import fusion_net_inputs

LOG_EVERY = 50


class Trainer:
    """Trainer for the fusion net"""

    def __init__(self, args, train_loader, fusion_net, phase_net, adacof_model, my_pyr, lr=0.001, weight_decay=0.0,
                 start_epoch=0, out_dir="."):
        if getattr(args, "save", False):
            raise NotImplementedError("--save: the dump of FusionNet's residual sums is not built")
        self.args = args
        self.train_loader = train_loader
        self.max_step = len(self.train_loader)
        self.pyr = my_pyr
        self.current_epoch = start_epoch
        self.device = my_pyr.device
        self.l1 = torch.nn.L1Loss()
        self.lpips_weight = float(getattr(args, "lpips_weight", 0) or 0)
        self.lpips = None
        if self.lpips_weight != 0:
            from ..evaluation.lpips import LPIPS
            self.lpips = LPIPS(getattr(args, "vgg_weights", None), getattr(args, "lpips_weights", None),
                               reduction="mean").to(self.device).eval()
        self.ssim_weight = float(getattr(args, "ssim_weight", 0) or 0)
        self.ssim = None
        if self.ssim_weight != 0:
            from ..evaluation.ssim import SSIMLoss
            self.ssim = SSIMLoss(reduction="mean")

        self.fusion_net = fusion_net
        self.phase_net = phase_net
        self.adacof_model = adacof_model
        self.fusion_net.train()

        self.out_dir = out_dir
        adam = torch.optim.Adam
        if getattr(args, "device_optimizer", False):      # the same class with its step on the device (vfi_amd/optim.py)
            from ..optim import Adam as adam
        self.optimizer = adam(self.fusion_net.parameters(), lr=lr, weight_decay=weight_decay)
        self.result_dir = self.out_dir + "/result"
        self.ckpt_dir = self.out_dir + "/checkpoint"
        self.create_folders()

        self.logfile = open(self.out_dir + "/log.txt", "w")
        self._losses = LossHistory()

    @property
    def loss_history(self):
        return self._losses.flush()

    def create_folders(self):
        """ Checks whether the folders for results and checkpoints already exists or creates them. """
        for d in (self.out_dir, self.result_dir, self.ckpt_dir):
            os.makedirs(d, exist_ok=True)

    def predict(self, lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target=None):
        """ Given batch of input images, predict the intermediate images: -> (final (3B, h, w), phase_pred (B, 3, h, w)). """
        base, ada_pred, phase_pred, other, maps = fusion_net_inputs(self.adacof_model, self.phase_net, self.pyr, lab_frame1,
                                                                    lab_frame2, rgb_frame1, rgb_frame2)
        final_pred = self.fusion_net(base, ada_pred, phase_pred, other, maps, variant=0)
        return final_pred.reshape(-1, final_pred.shape[2], final_pred.shape[3]), phase_pred

    def _unpack(self, batch):
        """-> lab_frame1, lab_frame2 (3B, h, w); rgb_frame1, rgb_frame2, the rgb target (B, 3, h, w)"""
        if hasattr(batch, "lab"):
            return batch.lab_frame1, batch.lab_frame2, batch.rgb_frame1, batch.rgb_frame2, batch.rgb_target
        triple = batch                                                                   # trainer.py:231-239
        return (preprocess(triple[0], self.device), preprocess(triple[2], self.device), triple[0].to(self.device),
                triple[2].to(self.device), triple[1].to(self.device))

    def train(self):
        """ Train the model for one epoch. """
        for batch_idx, batch in enumerate(self.train_loader):
            lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target = self._unpack(batch)
            prediction, _ = self.predict(lab_frame1, lab_frame2, rgb_frame1, rgb_frame2)

            prediction = torch.clip(prediction, 0, 1).reshape(target.shape).float()
            loss = self.l1(target.float(), prediction)
            if self.lpips is not None:
                loss = loss + self.lpips_weight * self.lpips(prediction, target.float())
            if self.ssim is not None:
                loss = loss + self.ssim_weight * self.ssim(prediction, target.float())

            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
            self._losses.append(loss)

            if batch_idx % LOG_EVERY == 0:
                self.test(idx=batch_idx // LOG_EVERY, paths=getattr(self.args, "test_paths", None), name="test")
                print('{:<13s}{:<14s}{:<6s}{:<16s}{:<12s}{:<20.16f}'.format(
                    'Train Epoch: ', '[' + str(self.current_epoch) + '/' + str(self.args.epochs) + ']', 'Step: ',
                    '[' + str(batch_idx) + '/' + str(self.max_step) + ']', 'train loss: ', float(loss.detach())))
                torch.save(self.fusion_net.state_dict(), self.out_dir + f'/checkpoint/model_{self.current_epoch}_{batch_idx // LOG_EVERY}.pt')
                np.savetxt(self.out_dir + '/log_train.txt', np.asarray(self.loss_history))

        self._losses.flush()
        self.current_epoch += 1

    def test(self, idx=None, paths=None, name=''):
        frames = read_test_images(paths)
        if frames is None:
            return
        frame1, _, frame2 = frames
        rgb_frame1 = frame1.unsqueeze(0).to(self.device)
        rgb_frame2 = frame2.unsqueeze(0).to(self.device)
        lab_frame1, lab_frame2 = preprocess(rgb_frame1, self.device), preprocess(rgb_frame2, self.device)

        was = self.fusion_net.training
        self.fusion_net.eval()
        try:
            with torch.no_grad():
                prediction, _ = self.predict(lab_frame1, lab_frame2, rgb_frame1, rgb_frame2)
        finally:
            self.fusion_net.train(was)

        if idx is not None:
            name = f'/result/{name}_{self.current_epoch}_{idx}.png'
        else:
            name = f'/result/{name}_{self.current_epoch}.png'
        save_image(prediction, self.out_dir + name)

    def terminate(self):
        return self.current_epoch >= self.args.epochs

    def close(self):
        self.logfile.close()
