"""FusionNet's training batch -- mirror of reference src/fusion_net/trainer.py:65-220 (`Trainer.predict` up to the call of
the network) for B samples at once.

`fusion_net_inputs` produces the five inputs of `FusionNet.forward` under no_grad; `fusion_net(base, ada_pred, phase_pred,
other, maps, variant=0)` is then the trainable forward, and `l1(target, clip(final, 0, 1)).backward()` the reference's step
(trainer.py:246-259).  It is `FusionInterpolator._run` (interpolate_twoframe.py) on batches, with the same operations: the
fused forms of the two uncertainty maps, AdaCoF #1-#3 as one batch of 3B and #4 on their results.  The PhaseNet branch takes
the reference's own route -- per-image `filter`, `separate_vals`, `get_concat_layers_inf`, `normalize_vals` -- because the
block-input layout of `filter(concat_frames=...)` is the per-frame layout and holds 16 images at most; the per-image calls
take any number (6B and 6B images through the two analyses, 3B through each synthesis).

The reference's quirks hold: `phase_pred` is `rgb_pred` without the exchanged high level (trainer.py:108-115), and the
uncertainty analyses run on rgb images (:118-123).
"""
import inspect

import torch

from .. import ops
from ..train.utils import get_concat_layers_inf, separate_vals
from ..values import DecompValues


def _adacof_kwargs(adacof_model):
    """The fusion variant skips the stores of the two sampled sides, which nothing here reads (FusionInterpolator.__init__)."""
    net = getattr(adacof_model, "model", adacof_model)
    return {"return_sides": False} if "return_sides" in inspect.signature(getattr(net, "forward", net)).parameters else {}


@torch.no_grad()
def fusion_net_inputs(adacof_model, phase_net, pyr, lab_frame1, lab_frame2, rgb_frame1, rgb_frame2):
    """lab_frame1, lab_frame2: (3B, H, W) Lab channel-images (`utils.preprocess`), sample-major; rgb_frame1, rgb_frame2:
    (B, 3, H, W) in [0, 1]; adacof_model(f1, f2) -> (side 1, side 2, result, mask); phase_net: the two-image
    `phase_net.PhaseNet` built on `pyr`.
    -> (base, ada_pred, phase_pred (B, 3, H, W) rgb; other (B, 6, H, W) = Lab frame 1 | Lab frame 2;
        maps (B, 3, H, W) = [ada_uncertainty, phase_uncertainty, flow_var_map], trainer.py:208-211).  Nothing carries a graph."""
    b, _, h, w = rgb_frame1.shape
    if tuple(lab_frame1.shape) != (3 * b, h, w) or lab_frame2.shape != lab_frame1.shape or rgb_frame2.shape != rgb_frame1.shape:
        raise ValueError(f"fusion_net_inputs: Lab channel-images {tuple(lab_frame1.shape)}, {tuple(lab_frame2.shape)} do not "
                         f"belong to rgb frames {tuple(rgb_frame1.shape)}, {tuple(rgb_frame2.shape)}")
    nlev = pyr.height - 2
    rgb_frame1, rgb_frame2 = rgb_frame1.float().contiguous(), rgb_frame2.float().contiguous()
    lab_frame1, lab_frame2 = lab_frame1.float(), lab_frame2.float()
    pyr.set_full_size(h, w)

    # PhaseNet branch (trainer.py:80-106): one analysis of all 6B channel-images
    vals_list = separate_vals(pyr.filter(torch.cat((lab_frame1, lab_frame2), 0)), 2)
    vals_pred = phase_net(phase_net.normalize_vals(get_concat_layers_inf(pyr, vals_list)))
    lab_pred = pyr.inv_filter(DecompValues(0, vals_pred.phase, vals_pred.amplitude, vals_pred.low_level))      # (the high level is zero)
    phase_pred = ops.lab2rgb(lab_pred.reshape(b, 3, h, w))                                  # :102-106, :115

    # AdaCoF #1 (rgb1, rgb2) (:69), #2 (rgb1, phase_pred) and #3 (phase_pred, rgb2) (:150-155): one batch of 3B
    kw = _adacof_kwargs(adacof_model)
    _, _, three, masks = adacof_model(torch.cat((rgb_frame1, rgb_frame1, phase_pred), 0),
                                      torch.cat((rgb_frame2, phase_pred, rgb_frame2), 0), **kw)
    three = three.float()
    ada_pred, flow_var_map = three[:b].contiguous(), masks[:b].float()                      # (B,3,H,W), (B,1,H,W)

    # phase uncertainty (:125-135): h_freq - h_freq_ph is one radial gain (finest band level + high residual) applied to
    # mean_c(ada_pred) - mean_c(rgb_pred)
    planes = torch.empty((3, b, h, w), dtype=torch.float32, device=rgb_frame1.device)       # [ada | phase | flow] uncertainty
    m = ops.channel_mean_diff(ada_pred, phase_pred, 1.0, False, signed=True)                # (B,H,W)
    hf = pyr.band_filter(m, level_mask=1, keep_high=True)
    ops.gaussian_filter(ops.absdiff(hf, None, 100.0, True), 5, out=planes[1])

    # ada uncertainty (:137-146): the 6 coarsest levels of one analysis of 6B rgb channel-images
    coarse = min(6, nlev)
    mask = ((1 << coarse) - 1) << (nlev - coarse)
    vb = pyr.filter(torch.cat((ada_pred.reshape(3 * b, h, w), phase_pred.reshape(3 * b, h, w)), 0), level_mask=mask, want_high=False)
    half = lambda t: (t[:t.shape[0] // 2], t[t.shape[0] // 2:])                             # ada planes | phase planes
    dp, da = [0] * nlev, [0] * nlev
    for k in range(nlev - coarse, nlev):
        dp[k] = ops.absdiff(*half(vb.phase[k])[::-1])                                       # subtract_values(vals_ph, vals_ada)
        da[k] = ops.absdiff(*half(vb.amplitude[k])[::-1])
    dlow = ops.absdiff(*half(vb.low_level)[::-1])
    freq = pyr.inv_filter(DecompValues(0, dp, da, dlow))                                    # (3B,H,W)
    fd = ops.channel_mean_diff(freq.reshape(b, 3, h, w), None, 30.0, False)                 # :141
    ops.absdiff(fd, ops.median_filter(fd, 50), 5.0, True, out=planes[0])                    # :142-145

    # base (:158): AdaCoF #4 on the two intermediate results
    base = adacof_model(three[b:2 * b].contiguous(), three[2 * b:].contiguous(), **kw)[2].float()

    planes[2].copy_(flow_var_map[:, 0])
    other = torch.cat((lab_frame1.reshape(b, 3, h, w), lab_frame2.reshape(b, 3, h, w)), 1)  # :208-209
    maps = planes.transpose(0, 1).contiguous()                                              # :210
    return base, ada_pred, phase_pred, other, maps
