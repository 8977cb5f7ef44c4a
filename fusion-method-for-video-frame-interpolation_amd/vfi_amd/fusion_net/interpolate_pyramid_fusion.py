"""Pyramid-domain fusion -- counterpart of reference `src/fusion_net/interpolate_twoframe copy.py`:89-192 for its models 1 and 2
(also src/fusion_net/full_res_fusion_net.py:73-101): AdaCoF's outputs enter the steerable pyramid next to the two frames, and a
PhaseNet with more than two input images fuses them there.

  model 1 (`num_img=4`): the two frames and AdaCoF's two warped sides (frame_out1, frame_out2);
  model 2 (`num_img=3`): the two frames and AdaCoF's result (ada_pred).

(Model 3, the pixel-wise FusionNet, is `interpolate_twoframe.FusionInterpolator`.)

`PyramidFusionInterpolator.__call__` runs the whole sequence on the device:

  AdaCoF | rgb->Lab of every image | pyramid(4*3 or 3*3 Lab images, frame-major) written in PhaseNet's block-input layout |
  PhaseNet(num_img) | inverse pyramid | Lab->rgb

Differences from the reference's execution: the three colours run as one batch (the reference loops over them to save memory,
:156-186), the pyramid and the network are built once per frame size (:120-151), nothing leaves the device (:95-117), and the
frames are not padded to a square (:99-105; the pyramid takes any size, as in FusionInterpolator).

The reference's checkpoints of these models, `fusion_net1.pt` and `fusion_net2.pt` (:137,140), are not part of its snapshot.  The
class takes any state dict with the reference's key names (`PhaseNet(pyr, device, num_img).state_dict()`).
"""
import math

import numpy as np
import torch

from .. import ops
from ..phase_net.phase_net import PhaseNet
from ..train.pyramid import Pyramid
from ..train.utils import calc_pyr_height
from ..values import DecompValues

NUM_IMG = {1: 4, 2: 3}       # `interpolate_twoframe copy.py`:135-140


class PyramidFusionInterpolator:
    """Holds AdaCoF and the per-size pyramid + PhaseNet(num_img); `__call__(rgb1, rgb2)` -> dict of tensors.
    model: 1 or 2 (the reference's `args.model`)."""

    def __init__(self, adacof_model, model, phase_net_state=None, device=None):
        if model not in NUM_IMG:
            raise ValueError(f"model must be 1 (four images) or 2 (three images), got {model!r}; model 3 is FusionInterpolator")
        self.adacof = adacof_model
        self.model = model
        self.num_img = NUM_IMG[model]
        self.device = torch.device(device) if device is not None else next(adacof_model.parameters()).device
        self.phase_net_state = phase_net_state
        self._per_size = {}

    def _state(self, h, w):
        key = (h, w)
        if key not in self._per_size:
            height = calc_pyr_height(torch.empty(3, h, w, device="meta"))
            pyr = Pyramid(height=height, nbands=4, scale_factor=np.sqrt(2), device=self.device)   # :120-125
            pyr.set_full_size(h, w)
            net = PhaseNet(pyr, self.device, num_img=self.num_img)                                # :149-151
            if self.phase_net_state is not None:
                net.load_state_dict(self.phase_net_state)
            net.eval()
            self._per_size[key] = (pyr, net)
        return self._per_size[key]

    @torch.no_grad()
    def __call__(self, rgb_frame1, rgb_frame2, high_level=False):
        """rgb_frame1/2: (3,H,W) float32 in [0,1] on the device.  high_level: the prediction takes the high residual of
        AdaCoF's result (:128-132,182-183) instead of none."""
        h, w = rgb_frame1.shape[1:]
        pyr, net = self._state(h, w)
        f = self.num_img
        out1, out2, ada_pred, flow_var_map = self.adacof(rgb_frame1.unsqueeze(0), rgb_frame2.unsqueeze(0))   # :90-93
        # every Lab image in ONE (3*num_img,H,W) buffer, frame-major: the pyramid's input (:158-165)
        lab = torch.empty((3 * f, h, w), dtype=torch.float32, device=rgb_frame1.device)
        extra = (out1[0], out2[0]) if self.model == 1 else (ada_pred[0],)
        for i, img in enumerate((rgb_frame1, rgb_frame2, *extra)):
            ops.rgb2lab(img, out=lab[3 * i:3 * i + 3])                                          # :108-117
        vals, bufs, amp_max = pyr.filter(lab, concat_frames=f, phase_scale=1.0 / math.pi, amp_max_eps=net.eps,
                                         pred_channels=net.pred_channels)
        vals_pred = net(net.normalize_vals(vals, concat=bufs, amp_max=amp_max))                 # :166-180
        high = 0
        if high_level and self.model == 2:                   # AdaCoF's result is model 2's third image: (3,1,H,W) of (C,F,H,W)
            high = vals.high_level[:, 2:3].contiguous()
        elif high_level:
            high = pyr.filter(ops.rgb2lab(ada_pred[0]), want_low=False).high_level              # :128-132
        lab_pred = pyr.inv_filter(DecompValues(high, vals_pred.phase, vals_pred.amplitude, vals_pred.low_level))   # :182-185
        return {"fusion_pred": ops.lab2rgb(lab_pred).unsqueeze(0), "ada_pred": ada_pred, "flow_var_map": flow_var_map}
