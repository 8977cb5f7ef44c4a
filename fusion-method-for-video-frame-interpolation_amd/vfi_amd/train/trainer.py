"""Trainer of PhaseNet and of the pyramid-domain fusion PhaseNets -- mirror of reference src/train/trainer.py:22-219.

`Trainer(args, train_loader, model, pyr, lr, weight_decay, start_epoch, out_dir, m, m_update)`; `args` carries `mode`
('phase' | 'fusion'), `model` (0: four input images, 1: three), `high_level`, `epochs`, `gpu_id` and optionally
`fixed_stats`, `adacof_checkpoint`, `test_paths`.  `train_loader` yields `datareader.TripletBatch`es (`TripletLoader`), or the
reference's triples of (B, 3, h, w) CPU tensors (a stock `DataLoader` over `DBreader_Vimeo90k`), which then take the
reference's route: float upload and `preprocess`.

Differences from the reference:

* The model is called as `model(img_batch, m=self.m)`.  The reference's `self.model(img_batch)` (trainer.py:107) drops `m`;
  with the target in the batch that cannot run: architecture.py:41-47 would treat the target as an input frame and return
  `vals_target = None`.
* Training mode is `model.fine_tune(True, batch_stats=..., fusion=(args.mode == 'fusion'))`, set by the constructor.
  batch_stats defaults to True, because the reference trains in `train()` mode; `args.fixed_stats` selects the
  fixed-statistics fine-tuning of DESIGN.md section 16.  `model.train()` keeps raising.
* `test()` replaces the reference's `eval()` / `train()` pair by `fine_tune(False)` around the no_grad prediction and
  restores the previous setting, so the call moves no running statistics.  It reads its three images with PIL and returns
  silently when `paths` is None or a file is missing; the reference hard-codes `counter_examples/...`.  `train()` passes
  `args.test_paths`.
* No plots.  The text logs (`log_train.txt`, `log.txt`, `config.txt`) are kept.
* `args.high_level` keeps the reference's meaning: AdaCoF is loaded; the flag is not forwarded to the model.
* AdaCoF's checkpoint is `args.adacof_checkpoint` (default: the reference's path); a ready model can be passed instead
  (`adacof_model=`).
* The loss goes to the host only where it is logged (every 100 batches) and at the end of the epoch; until then the history
  is a list of device scalars (`LossHistory.pending`), so the loop does not synchronise every step.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from ..adacof.models import Model
from .fusion import fusion_img_batch
from .loss import get_loss
from .transform import lab2rgb_single
from .utils import preprocess

ADACOF_CHECKPOINT = "src/adacof/checkpoint/kernelsize_5/ckpt.pth"       # trainer.py:61-62
LOG_EVERY = 100


def load_adacof(gpu_id, checkpoint=None):
    """The fusion variant of AdaCoFNet with the reference's settings (trainer.py:52-63), in eval mode."""
    model = Model(SimpleNamespace(gpu_id=gpu_id, model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1))
    model.eval()
    state = torch.load(checkpoint or ADACOF_CHECKPOINT, map_location=torch.device("cpu"))
    model.load(state["state_dict"])
    return model


def read_test_images(paths):
    """Three (3, H, W) float rgb tensors in [0, 1] (trainer.py:173-185), or None when `paths` is None or a file is missing."""
    if paths is None or len(paths) != 3 or not all(os.path.isfile(p) for p in paths):
        return None
    return [torch.from_numpy(np.array(Image.open(p).convert("RGB"))).permute(2, 0, 1).contiguous().float() / 255 for p in paths]


def save_image(img, path):
    """(3, H, W) in [0, 1] -> PNG, as ToPILImage: * 255, truncated to uint8."""
    arr = img.detach().cpu().mul(255).byte().permute(1, 2, 0).numpy()
    Image.fromarray(arr).save(path)


class LossHistory:
    """`history`: floats on the host; `pending`: device scalars of the steps since the last `flush`."""

    def __init__(self):
        self.history, self.pending = [], []

    def append(self, loss):
        self.pending.append(loss.detach())

    def flush(self):
        if self.pending:
            self.history += torch.stack(self.pending).cpu().tolist()
            self.pending = []
        return self.history


class Trainer:
    """Trainer for fusion and phase net"""

    def __init__(self, args, train_loader, model, pyr, lr=0.001, weight_decay=0.0, start_epoch=0, out_dir=".", m=0,
                 m_update=100, adacof_model=None):
        self.args = args
        self.train_loader = train_loader
        self.max_step = len(self.train_loader)
        self.model = model
        self.pyr = pyr
        self.current_epoch = start_epoch
        self.device = pyr.device
        self.m = m
        self.m_update = m_update
        self.out_dir = out_dir
        self.fusion = args.mode == "fusion"
        if args.mode not in ("phase", "fusion"):
            raise ValueError(f"Trainer: mode {args.mode!r} is neither 'phase' nor 'fusion'")
        self.model.fine_tune(True, batch_stats=not getattr(args, "fixed_stats", False), fusion=self.fusion)

        adam = torch.optim.Adam
        if getattr(args, "device_optimizer", False):      # the same class with its step on the device (vfi_amd/optim.py)
            from ..optim import Adam as adam
        self.optimizer = adam(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        self.result_dir = self.out_dir + "/result"
        self.ckpt_dir = self.out_dir + "/checkpoint"
        self.create_folders()

        self.logfile = open(self.out_dir + "/log.txt", "w")
        self._losses = LossHistory()

        self.adacof_model = adacof_model
        if adacof_model is None and (self.fusion or args.high_level):
            self.adacof_model = load_adacof(args.gpu_id, getattr(args, "adacof_checkpoint", None))

    @property
    def loss_history(self):
        return self._losses.flush()

    def create_folders(self):
        """ Checks whether the folders for results and checkpoints already exists or creates them. """
        for d in (self.out_dir, self.result_dir, self.ckpt_dir):
            os.makedirs(d, exist_ok=True)

    def predict(self, lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target, img_batch=None):
        """ Given batch of input images, predict the intermediate images.  `img_batch`: the phase-mode batch when the caller
        already holds it in one piece (TripletBatch.img_batch_phase), instead of the `cat` of trainer.py:103. """
        if self.fusion:
            img_batch = fusion_img_batch(self.adacof_model, lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target,
                                         4 if self.args.model == 0 else 3)
        elif img_batch is None:
            img_batch = torch.cat((lab_frame1, lab_frame2, target), 0)
        return self.model(img_batch, m=self.m)

    def _unpack(self, batch):
        """-> lab_frame1, lab_frame2, target (3B, h, w); rgb_frame1, rgb_frame2 (B, 3, h, w); the phase img_batch or None"""
        if hasattr(batch, "lab"):
            whole = batch.img_batch_phase if batch.lab.is_contiguous() else None
            rgb1, rgb2 = (batch.rgb_frame1, batch.rgb_frame2) if batch.rgb is not None else (None, None)
            return batch.lab_frame1, batch.lab_frame2, batch.lab_target, rgb1, rgb2, whole
        triple = batch                                                                   # trainer.py:115-121
        return (preprocess(triple[0], self.device), preprocess(triple[2], self.device), preprocess(triple[1], self.device),
                triple[0].to(self.device), triple[2].to(self.device), None)

    def train(self):
        """ Train the model for one epoch. """
        for batch_idx, batch in enumerate(self.train_loader):
            lab_frame1, lab_frame2, target, rgb_frame1, rgb_frame2, img_batch = self._unpack(batch)
            prediction, vals_pred, vals_target = self.predict(lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target, img_batch)
            loss, p1, p2 = get_loss(vals_pred, vals_target, prediction, target, self.pyr)

            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
            self._losses.append(loss)

            if batch_idx % LOG_EVERY == 0:
                self.test(idx=batch_idx // LOG_EVERY, paths=getattr(self.args, "test_paths", None), name="test")
                print('{:<13s}{:<14s}{:<6s}{:<16s}{:<12s}{:<20.16f} Percentages: {:<4f}, {:<4f}'.format(
                    'Train Epoch: ', '[' + str(self.current_epoch) + '/' + str(self.args.epochs) + ']', 'Step: ',
                    '[' + str(batch_idx) + '/' + str(self.max_step) + ']', 'train loss: ', float(loss.detach()), float(p1), float(p2)))
                torch.save(self.model.state_dict(), self.out_dir + f'/checkpoint/model_{self.current_epoch}_{batch_idx // LOG_EVERY}.pt')
                np.savetxt(self.out_dir + '/log_train.txt', np.asarray(self.loss_history))

            # Hierarchical training update
            if batch_idx % self.m_update == 0 and batch_idx > 0 and self.m < 10:
                self.m += 1

        self._losses.flush()
        self.current_epoch += 1

    def test(self, idx=None, paths=None, name=''):
        frames = read_test_images(paths)
        if frames is None:
            return
        frame1, target, frame2 = frames
        rgb_frame1 = frame1.unsqueeze(0).to(self.device)
        rgb_frame2 = frame2.unsqueeze(0).to(self.device)
        lab_frame1, target, lab_frame2 = (preprocess(f.unsqueeze(0), self.device) for f in (frame1, target, frame2))

        core = self.model.core
        was = (core.fine_tuning, core.batch_stats)
        self.model.fine_tune(False)
        try:
            with torch.no_grad():
                prediction, _, _ = self.predict(lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target)
        finally:
            if was[0]:
                self.model.fine_tune(True, batch_stats=was[1], fusion=self.fusion)

        img = lab2rgb_single(prediction)
        if idx is not None:
            name = f'/result/{name}_{self.current_epoch}_{idx}.png'
        else:
            name = f'/result/{name}_{self.current_epoch}.png'
        save_image(img, self.out_dir + name)

    def terminate(self):
        return self.current_epoch >= self.args.epochs

    def close(self):
        self.logfile.close()
