"""The batch of the pyramid-domain fusion networks -- mirror of reference src/train/trainer.py:74-104 (`Trainer.predict` in
`--mode fusion`): AdaCoF runs under no_grad on the two rgb frames, its outputs go to Lab, become channel-images and are
concatenated next to the two Lab frames, the target last.  The result feeds
`architecture.PhaseNet(num_img=3 | 4).forward(img_batch, m=m)` after `fine_tune(fusion=True)`.

The trainer's `args.model` 0 / 1 are `PyramidFusionInterpolator`'s models 1 / 2; this function takes the number of input
images of the PhaseNet it feeds instead of either numbering: 4 = the two frames and AdaCoF's two warped sides, 3 = the two
frames and AdaCoF's result.
"""
import torch

from .. import ops


def _channel_images(rgb):
    lab = ops.rgb2lab(rgb.float())                                                        # trainer.py:82-84
    return lab.reshape(-1, lab.shape[2], lab.shape[3]).float()                            # :86-91


def fusion_img_batch(adacof_model, lab_frame1, lab_frame2, rgb_frame1, rgb_frame2, target, num_img):
    """lab_frame1, lab_frame2, target: (B*3, H, W) Lab channel-images (`utils.preprocess`); rgb_frame1, rgb_frame2: (B, 3, H, W)
    in [0, 1]; adacof_model(rgb_frame1, rgb_frame2) -> (warped frame 1, warped frame 2, result, ...).
    -> img_batch ((num_img + 1) * B * 3, H, W), frame-major: [frame 1 | frame 2 | AdaCoF's images | target] -- 5 values for four
    images, 4 for three.  No gradient reaches AdaCoF."""
    if num_img not in (3, 4):
        raise ValueError(f"fusion_img_batch: the fusion networks have 3 or 4 input images, not {num_img}")
    with torch.no_grad():
        ada_frame1, ada_frame2, ada_pred = adacof_model(rgb_frame1, rgb_frame2)[:3]      # :80-81
        if num_img == 4:
            extra = (_channel_images(ada_frame1), _channel_images(ada_frame2))            # :94-97
        else:
            extra = (_channel_images(ada_pred),)                                          # :98-101
    return torch.cat((lab_frame1, lab_frame2, *extra, target), 0)
