"""Test sets of the AdaCoF trainer -- mirror of reference src/adacof/TestModule.py:10-138: `Middlebury_eval`,
`Middlebury_other`, `Davis`, `ucf` with the reference's `im_list`s, directory layout, `Test(...)` signatures and log lines.

The model runs in eval mode through the unchanged inference path.  PSNR is `-10 * log10(mean((gt - out)^2))` with the mean
from `ops.mse_forward` (the fixed-order HIP reduction).

Differences from the reference:

* No torchvision.  Frames are decoded with PIL, converted as `ToTensor` does (uint8 HWC -> float CHW / 255) and uploaded
  once, at construction; frames that are not RGB are converted.
* The PNG is written as torchvision's `save_image` writes it -- `mul(255).add(0.5).clamp(0, 255)` to uint8 (`quantize`) --
  quantised on the device.  `range=(0, 1)` has no effect there without `normalize=True`, and has none here.
* `Test` runs under `torch.no_grad()`; the constructors take `device=` (default: the current HIP device; the host when
  there is none, where PSNR is the reference's torch expression).
* `Davis.Test` / `ucf.Test` write the epoch line from `model.get_epoch()` only when the model has that method (the
  reference's `Model` has none either); otherwise the line is left out.
"""
import os
from math import log10

import numpy as np
import torch
from PIL import Image

from .. import ops


def read_frame(path, device=None):
    """(1, 3, H, W) float in [0, 1] on the device: `ToTensor()(Image.open(path)).unsqueeze(0)` and the upload."""
    img = Image.open(path)
    if img.mode != 'RGB':
        img = img.convert('RGB')
    t = torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    return t.to(device)


def quantize(frame):
    """uint8 (H, W, 3) of a (1, 3, H, W) or (3, H, W) frame, by save_image's rule"""
    if frame.dim() == 4:
        frame = frame[0]
    return frame.detach().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def imwrite(frame, path):
    Image.fromarray(quantize(frame).cpu().numpy()).save(path)


def psnr_of(gt, frame_out):
    if not gt.is_cuda:              # host tensors: the reference's expression (TestModule.py:53)
        return -10 * log10(torch.mean((gt - frame_out) * (gt - frame_out)).item())
    return -10 * log10(ops.mse_forward(gt.contiguous(), frame_out.contiguous()).item())


def _run(im_list, input0_list, input1_list, gt_list, model, output_dir, epoch, logfile, output_name):
    """The body the three scored sets share (TestModule.py:43-64, 80-101, 117-138)."""
    model.eval()
    av_psnr = 0
    if logfile is not None and epoch is not None:
        logfile.write('{:<7s}{:<3d}'.format('Epoch: ', epoch) + '\n')
    with torch.no_grad():
        for idx in range(len(im_list)):
            if not os.path.exists(output_dir + '/' + im_list[idx]):
                os.makedirs(output_dir + '/' + im_list[idx])
            frame_out = model(input0_list[idx], input1_list[idx])
            gt = gt_list[idx]
            psnr = psnr_of(gt, frame_out)
            av_psnr += psnr
            imwrite(frame_out, output_dir + '/' + im_list[idx] + '/' + output_name)
            msg = '{:<15s}{:<20.16f}'.format(im_list[idx] + ': ', psnr) + '\n'
            print(msg, end='')
            if logfile is not None:
                logfile.write(msg)
    av_psnr /= len(im_list)
    msg = '{:<15s}{:<20.16f}'.format('Average: ', av_psnr) + '\n'
    print(msg, end='')
    if logfile is not None:
        logfile.write(msg)


def _epoch_of(model):
    return model.get_epoch() if hasattr(model, 'get_epoch') else None


class Middlebury_eval:
    def __init__(self, input_dir='./evaluation', device=None):
        self.im_list = ['Backyard', 'Basketball', 'Dumptruck', 'Evergreen', 'Mequon', 'Schefflera', 'Teddy', 'Urban']

        self.input0_list = []
        self.input1_list = []
        for item in self.im_list:
            self.input0_list.append(read_frame(input_dir + '/input/' + item + '/frame10.png', device))
            self.input1_list.append(read_frame(input_dir + '/input/' + item + '/frame11.png', device))

    def Test(self, model, output_dir='./evaluation/output', output_name='frame10i11.png'):
        model.eval()
        with torch.no_grad():
            for idx in range(len(self.im_list)):
                if not os.path.exists(output_dir + '/' + self.im_list[idx]):
                    os.makedirs(output_dir + '/' + self.im_list[idx])
                frame_out = model(self.input0_list[idx], self.input1_list[idx])
                imwrite(frame_out, output_dir + '/' + self.im_list[idx] + '/' + output_name)


class Middlebury_other:
    def __init__(self, input_dir, gt_dir, device=None):
        self.im_list = ['Beanbags', 'Dimetrodon', 'DogDance', 'Grove2', 'Grove3', 'Hydrangea', 'MiniCooper', 'RubberWhale', 'Urban2', 'Urban3', 'Venus', 'Walking']

        self.input0_list = []
        self.input1_list = []
        self.gt_list = []
        for item in self.im_list:
            self.input0_list.append(read_frame(input_dir + '/' + item + '/frame10.png', device))
            self.input1_list.append(read_frame(input_dir + '/' + item + '/frame11.png', device))
            self.gt_list.append(read_frame(gt_dir + '/' + item + '/frame10i11.png', device))

    def Test(self, model, output_dir, current_epoch, logfile=None, output_name='output.png'):
        _run(self.im_list, self.input0_list, self.input1_list, self.gt_list, model, output_dir, current_epoch, logfile, output_name)


class Davis:
    def __init__(self, input_dir, gt_dir, device=None):
        self.im_list = ['bike-trial', 'boxing', 'burnout', 'choreography', 'demolition', 'dive-in', 'dolphins', 'e-bike', 'grass-chopper', 'hurdles', 'inflatable', 'juggle', 'kart-turn', 'kids-turning', 'lions', 'mbike-santa', 'monkeys', 'ocean-birds', 'pole-vault', 'running', 'selfie', 'skydive', 'speed-skating', 'swing-boy', 'tackle', 'turtle', 'varanus-tree', 'vietnam', 'wings-turn']

        self.input0_list = []
        self.input1_list = []
        self.gt_list = []
        for item in self.im_list:
            self.input0_list.append(read_frame(input_dir + '/' + item + '/frame10.png', device))
            self.input1_list.append(read_frame(input_dir + '/' + item + '/frame11.png', device))
            self.gt_list.append(read_frame(gt_dir + '/' + item + '/frame10i11.png', device))

    def Test(self, model, output_dir, logfile=None, output_name='output.png'):
        _run(self.im_list, self.input0_list, self.input1_list, self.gt_list, model, output_dir, _epoch_of(model), logfile, output_name)


class ucf:
    def __init__(self, input_dir, device=None):
        self.im_list = ['1', '2', '3', '4', '5', '6', '7', '8', '9', '10', '11', '12', '13', '14', '15', '16', '17', '18', '19', '20', '21']

        self.input0_list = []
        self.input1_list = []
        self.gt_list = []
        for item in self.im_list:
            self.input0_list.append(read_frame(input_dir + '/' + item + '/frame0.png', device))
            self.input1_list.append(read_frame(input_dir + '/' + item + '/frame2.png', device))
            self.gt_list.append(read_frame(input_dir + '/' + item + '/frame1.png', device))

    def Test(self, model, output_dir, logfile=None, output_name='output.png'):
        _run(self.im_list, self.input0_list, self.input1_list, self.gt_list, model, output_dir, _epoch_of(model), logfile, output_name)
