"""PhaseNet -- mirror of reference src/phase_net/phase_net.py (`PhaseNet(pyr, device, num_img)`; the fused path uses
num_img=2; two-call protocol `normalize_vals(vals)` then `forward(vals)`).

Execution on the MI355X (all arithmetic in libvfi_hip.so):
  * block = [conv k, BN(eval), ELU, conv k, ELU] -> 64 features; [1x1 conv, tanh] -> prediction
    (phase_net.py:190-200): three fp32-MFMA conv launches, BN folded into the first conv's weights,
    ELU / tanh in the conv epilogues; k = 1 for blocks 0-2, 3 (reflect) for 3-7 (phase_net.py:30-35);
  * the block input `cat(feature_r, phase, amp, prediction_r)` (phase_net.py:141) is never
    concatenated: each level owns one buffer laid out [feature 64 | prediction P | phase 8 | amp 8]
    (the first conv's input channels are permuted to match at pack time); the previous block writes
    feature and prediction into ONE tensor, so a single bilinear-resize launch fills the first 64+P
    channels, and normalize_vals writes phase/pi and amp/max straight into the last 16;
  * the per-level blend + de-normalisation (phase_net.py:155-168, :80-105) is one launch per level: the prediction map's
    launch -- and, below a level whose first conv is 3x3, also the launch that resizes into that level's buffer
    (vfi_phasenet_level_tail, two images only).
Maxima are returned/kept per call on the module (as the reference does, phase_net.py:53,59,70).

`num_img` = 3 and 4 are the reference's pyramid-domain fusion networks (phase_net.py:21-35, 119-121, 158-162; DESIGN.md section
18): the buffers are [feature 64 | prediction P | phase 4*num_img | amp 4*num_img] with P = `pred_channels`, the heads are
vfi_phasenet_predict_n / vfi_phasenet_emit_low_n.  They train after `fine_tune(fusion=True)`.

After `fine_tune()`, with grad mode on and a parameter of `layers` requiring grad, `forward` takes a second route,
`_forward_grad`: the same walk as an autograd graph with HIP backward kernels, BatchNorm on its running statistics (DESIGN.md
section 16).  After `fine_tune(batch_stats=True)` every forward takes that route, with BatchNorm on the batch's statistics
and the running statistics updated (training from scratch, section 17).  Every other call runs the code above, unchanged.
"""
import math
import os

import torch

from .. import _lib, ops
from ..nn_util import BatchNormParams, ConvParams, Indexed, PackedModule
from ..values import DecompValues, NormalizedValues


class PhaseNetBlock(torch.nn.Module):
    """The reference's block with its key names (phase_net.py:179-207, block.py:4-32).  PhaseNet.forward runs the blocks
    through its own permuted packs; `forward` here is the reference's `(f, c) = block(x)` on an input in the reference's
    channel order, differentiable with a HIP backward.  BatchNorm uses its running statistics: a new
    block is in eval mode, and a block switched to training mode refuses to run.  Batch statistics are asked for with
    `batch_statistics()` (or the network's `fine_tune(batch_stats=True)`), not with `train(True)`: the block stays in eval
    mode (`training` is False) and its flag `batch_stats` selects the route of DESIGN.md section 17."""

    def __init__(self, c_in, c_out, pred_out, kernel_size, device=None, dropout=0.5):
        super().__init__()
        k = kernel_size[0]
        self.feature_map = Indexed({0: ConvParams(c_in, c_out, k), 1: BatchNormParams(c_out),
                                    3: ConvParams(c_out, c_out, k)})
        self.prediction_map = Indexed({0: ConvParams(c_out, pred_out, 1)})
        self.batch_stats = False
        self.train(False)
        if device is not None:
            self.to(device)

    def batch_statistics(self, mode=True):
        """BatchNorm on the batch's statistics on or off (off in a new block), for a block used on its own.  With it on,
        every forward -- grad mode or not -- normalises with the mean and biased variance of its own input batch and moves
        `running_mean`, `running_var` and `num_batches_tracked` as nn.BatchNorm2d in training mode does.  The block stays
        in eval mode: `training` is False, and `train(True)` keeps refusing to run."""
        self.batch_stats = bool(mode)
        return self

    def forward(self, x):
        from .grad import block_forward
        return block_forward(self, x)


class PhaseNet(PackedModule):
    def __init__(self, pyr, device, num_img=2):
        super().__init__()
        if num_img not in (2, 3, 4):
            raise NotImplementedError("vfi_amd.PhaseNet implements the reference's networks of two, three and four input images")
        self.pyr = pyr
        self.device = torch.device(device)
        self.num_img = num_img
        self.eps = 1e-8
        # phase_net.py:23-35: three images predict one more low-level weight and four more amplitude weights per level
        p_low, p_band = self.pred_channels
        blocks = [PhaseNetBlock(num_img, 64, p_low, (1, 1)),
                  PhaseNetBlock(64 + p_low + 8 * num_img, 64, p_band, (1, 1)),
                  PhaseNetBlock(64 + p_band + 8 * num_img, 64, p_band, (1, 1))]
        blocks += [PhaseNetBlock(64 + p_band + 8 * num_img, 64, p_band, (3, 3)) for _ in range(5)]
        self.layers = torch.nn.ModuleList(blocks)
        self.max_amplitudes = None
        self.max_low_level = None
        self.fine_tuning = False
        self.batch_stats = False
        self.train(False)
        self.to(self.device)

    @property
    def pred_channels(self):
        """(low level's, a band level's) prediction channels: (2, 12) for three input images, else (1, 8) (phase_net.py:23-35);
        what Pyramid.filter(concat_frames=num_img, pred_channels=...) lays the block-input buffers out for."""
        return ops.phasenet_pred_channels(self.num_img)

    def fine_tune(self, mode=True, batch_stats=False, fusion=False):
        """Training on or off (off in a new module).  It is PhaseNet's counterpart of FusionNet's training mode: a new
        module's parameters require grad, so callers that never backpropagate keep results without a grad_fn unless they
        ask here.  `fine_tune()` is fixed-statistics fine-tuning: BatchNorm on the running statistics of the checkpoint.
        `fine_tune(batch_stats=True)` is the reference's training mode (src/train/train.py:90, trainer.py:107-134): it sets
        every block's `batch_stats` flag, and every forward from then on, grad mode or not, normalises with the batch's
        statistics and moves the running ones.  `fine_tune(False)` clears everything.  The module stays in eval mode throughout
        (`training` is False); `train(True)` keeps raising.

        The networks of three and four input images (the reference's `--mode fusion`, trainer.py:74-134) train after
        `fine_tune(fusion=True)`, on fixed or batch statistics.  The keyword exists because the bare call
        on such a network was defined, before their training was built, to raise NotImplementedError, and callers and tests
        rely on that answer -- as `train(True)` keeps raising and batch statistics are asked for by a keyword.  It has no
        effect on the network of two images."""
        if mode and self.num_img != 2 and not fusion:
            raise NotImplementedError("training of the fusion variants (num_img = 3, 4) is not built: PhaseNet.fine_tune needs num_img = 2 "
                                      "-- or the keyword fusion=True, which trains them")
        self.fine_tuning = bool(mode)
        self.batch_stats = self.fine_tuning and bool(batch_stats)
        for blk in self.layers:
            blk.batch_statistics(self.batch_stats)
        return self

    # -- weights ------------------------------------------------------------------------------------
    def _build_packed(self):
        out = []
        for i, blk in enumerate(self.layers):
            w = blk.feature_map[0].weight
            if i >= 1:
                # reference channel order [feature 64 | phase 4F | amp 4F | pred P] -> ours
                # [feature 64 | pred P | phase 4F | amp 4F], F = num_img
                pa = 64 + 8 * self.num_img
                p = w.shape[1] - pa
                perm = list(range(64)) + list(range(pa, pa + p)) + list(range(64, pa))
                w = w[:, perm]
            c1 = ops.PackedConv(w, blk.feature_map[0].bias, bn=blk.feature_map[1].fold_args())
            out.append((c1, self.pack(blk.feature_map[3]), self.pack(blk.prediction_map[0])))
        return out

    # -- normalisation (phase_net.py:42-78) -------------------------------------------------------------
    def normalize_vals(self, vals, concat=None, amp_max=None):
        """phase_net.py:42-78.  `concat` (from Pyramid.filter(concat_frames=num_img, phase_scale=1/pi, pred_channels=self.pred_channels)): the block-input
        buffers that already hold phase/pi and the raw amplitudes -- then only the maxima are computed and
        the amplitudes / low level are normalised in place (no copies)."""
        if concat is not None:
            return self._normalize_in_place(vals, concat, amp_max)
        nlev = len(vals.phase)
        b = vals.amplitude[0].shape[0]
        maxes, concat, phases, amps = [], [], [], []
        for idx in range(nlev):
            amp, ph = vals.amplitude[idx].contiguous(), vals.phase[idx].contiguous()
            mx = ops.batch_max(amp, self.eps)                                   # :55
            maxes.append(mx)
            p_prev = self.pred_channels[0 if idx == 0 else 1]
            _, c, h, w = amp.shape
            buf = ops.new((b, 64 + p_prev + 2 * c, h, w), amp)
            pv = buf[:, 64 + p_prev:64 + p_prev + c]
            av = buf[:, 64 + p_prev + c:64 + p_prev + 2 * c]
            ops.affine_slice(ph, pv, None, 1.0 / math.pi)                        # :64
            ops.affine_slice(amp, av, mx, 1.0)                                   # :61
            concat.append(buf); phases.append(pv); amps.append(av)
        low_in = vals.low_level.contiguous()
        self.max_amplitudes = maxes
        self.max_low_level = ops.batch_max(low_in, self.eps)                     # :69
        low = ops.affine_slice(low_in, torch.empty_like(low_in), self.max_low_level, 1.0)   # :70
        out = NormalizedValues(vals.high_level, phases, amps, low)
        out.concat = concat
        return out

    def _normalize_in_place(self, vals, concat, amp_max=None):
        """amp_max (levels coarsest first, colours): maxima + eps already reduced by Pyramid.filter(amp_max_eps=...)."""
        maxes = []
        for idx, amp in enumerate(vals.amplitude):          # views into concat[idx]
            mx = amp_max[idx] if amp_max is not None else ops.batch_max(amp, self.eps)
            maxes.append(mx)
            ops.affine_slice(amp, amp, mx, 1.0)
        self.max_amplitudes = maxes
        self.max_low_level = ops.batch_max(vals.low_level, self.eps)
        ops.affine_slice(vals.low_level, vals.low_level, self.max_low_level, 1.0)
        out = NormalizedValues(vals.high_level, list(vals.phase), list(vals.amplitude), vals.low_level)
        out.concat = concat
        return out

    def reverse_normalize(self, vals, m):
        """phase_net.py:80-105 on already-blended outputs (generic path; forward() fuses this)."""
        phases = [ops.affine_slice(p.contiguous(), torch.empty_like(p), None, math.pi) for p in vals.phase]
        amps = []
        for i in range(m):
            a = vals.amplitude[i]
            nb = self.pyr.nbands
            a4 = a.reshape(a.shape[0] // nb, nb, a.shape[2], a.shape[3]).contiguous()
            inv = 1.0 / self.max_amplitudes[i]
            amps.append(ops.affine_slice(a4, torch.empty_like(a4), inv, 1.0).reshape(a.shape))
        for _ in range(self.pyr.height - 2 - m):
            phases.append(0); amps.append(0)
        low = ops.affine_slice(vals.low_level.contiguous(), torch.empty_like(vals.low_level),
                               1.0 / self.max_low_level, 1.0)
        return DecompValues(vals.high_level, phases[::-1], amps[::-1], low)

    # -- forward (phase_net.py:107-177) ------------------------------------------------------------------
    def forward(self, vals, m=None):
        if m is None:
            m = self.pyr.height - 2
        if self.max_amplitudes is None:
            raise RuntimeError("call normalize_vals(vals) before forward(vals) (phase_net.py two-call protocol)")
        if self.fine_tuning and (self.batch_stats or (torch.is_grad_enabled() and any(p.requires_grad for p in self.layers.parameters()))):
            return self._forward_grad(vals, m)
        packed = self.packed()
        low_in = vals.low_level.contiguous()
        b, _, hl, wl = low_in.shape
        stream = _lib.stream_ptr()

        def block(i, x, fp, prev=None, head=True):
            c1, c2, cp = packed[i]
            mode = "reflect" if c1.ks == 3 else "zeros"
            if prev is not None:     # 3x3 block: the resize of (feature | prediction) is done by the conv's tile loader
                t = ops.conv2d_resized_prefix(x, prev, c1, mode, "elu")
            else:
                t = ops.conv2d(x, c1, mode, "elu")
            ops.conv2d(t, c2, mode, "elu", out=fp[:, :64])
            if head:                 # (the band levels' prediction map comes out of vfi_phasenet_predict with their outputs)
                ops.conv2d(fp[:, :64], cp, "zeros", "tanh", out=fp[:, 64:])
            return fp

        n_img = self.num_img
        p_low, p_band = self.pred_channels
        fp = block(0, low_in, ops.new((b, 64 + p_low, hl, wl), low_in))               # :113
        low = ops.new((b, 1, hl, wl), low_in)
        if n_img == 2:
            _lib.call("vfi_phasenet_emit_low", fp[:, 64:].data_ptr(), fp.stride(0), low_in.data_ptr(), low_in.stride(0),
                      self.max_low_level.data_ptr(), low.data_ptr(), b, hl * wl, stream)     # :115-116 + :96-98
        else:                                                                          # ... + :119-121 for three images
            if low_in.shape[1] != n_img:
                raise RuntimeError(f"PhaseNet(num_img={n_img}): the low level has {low_in.shape[1]} images")
            _lib.call("vfi_phasenet_emit_low_n", fp[:, 64:].data_ptr(), fp.stride(0), low_in.data_ptr(), low_in.stride(0),
                      self.max_low_level.data_ptr(), low.data_ptr(), b, hl * wl, n_img, stream)
        hs = vals.high_level.shape
        high = torch.zeros((hs[0], 1, hs[2], hs[3]), dtype=torch.float32, device=low_in.device)   # :127-128

        concat = getattr(vals, "concat", None)

        def level_input(idx):
            if concat is not None:
                return concat[idx]
            # values not produced by normalize_vals: fill the block input buffer here
            ph, am = vals.phase[idx], vals.amplitude[idx]
            _, c, h, w = ph.shape
            p_prev = p_low if idx == 0 else p_band
            x = ops.new((b, 64 + p_prev + 2 * c, h, w), low_in)
            ops.affine_slice(ph.contiguous(), x[:, 64 + p_prev:64 + p_prev + c])
            ops.affine_slice(am.contiguous(), x[:, 64 + p_prev + c:])
            return x

        def layer(idx):
            return idx + 1 if idx + 1 < len(self.layers) - 1 else len(self.layers) - 1     # :148

        # two images, and the next level's first conv is the 3x3 that reads a materialised resize: this level's head and that
        # resize are one launch (vfi_phasenet_level_tail) from ops.PHASENET_TAIL_MIN_PIXELS pixels on.  VFI_PHASENET_TAIL, read
        # per call, is an A/B aid: 0 restores the two launches everywhere, 1 takes the one launch at every size
        tail_env = os.environ.get("VFI_PHASENET_TAIL", "")
        tail_on = n_img == 2 and not ops.FUSED_RESIZE and tail_env != "0"
        tail_min = 0 if tail_env == "1" else ops.PHASENET_TAIL_MIN_PIXELS
        phases, amps = [], []
        x_next = None
        for idx in range(m):
            p_prev = p_low if idx == 0 else p_band
            _, c, h, w = vals.phase[idx].shape
            filled = x_next is not None      # the level below has already written [feature | prediction], resized, into x
            x = x_next if filled else level_input(idx)
            i = layer(idx)
            fused = packed[i][0].ks == 3 and (64 + p_prev) % 8 == 0
            if not fused and not filled:
                ops.resize_bilinear(fp, (h, w), align_corners=False, out=x[:, :64 + p_prev])   # :138-141
            tail = tail_on and idx + 1 < m and h * w >= tail_min and packed[layer(idx + 1)][0].ks == 3 and (64 + p_band) % 8 == 0
            fp = block(i, x, ops.new((b, 64 if tail else 64 + p_band, h, w), low_in), prev=fp if fused and not filled else None, head=False)
            amp_in = x[:, 64 + p_prev + c:]
            # prediction map (1x1, tanh) + this level's outputs in one pass over the 64 feature channels (:149-168)
            cp = packed[i][2]
            if cp.cout != p_band or cp.ks != 1:
                raise RuntimeError(f"PhaseNet: a band level's prediction map must be a 1x1 layer with {p_band} outputs (phase_net.py:23-35)")
            x_next = None
            if tail:                 # ... and the resize of (feature | prediction) into the next level's input, same pass
                x_next = level_input(idx + 1)
                p_out, a_out = ops.phasenet_level_tail(fp, cp, amp_in, self.max_amplitudes[idx], x_next[:, :64 + p_band])
            elif n_img == 2:
                p_out, a_out = ops.new((b * 4, 1, h, w), low_in), ops.new((b * 4, 1, h, w), low_in)
                _lib.call("vfi_phasenet_predict", fp.data_ptr(), fp.stride(0), cp.packed.data_ptr(), cp.bias.data_ptr(), amp_in.data_ptr(),
                          x.stride(0), self.max_amplitudes[idx].data_ptr(), fp[:, 64:].data_ptr(), fp.stride(0), p_out.data_ptr(),
                          a_out.data_ptr(), b, 64, h, w, stream,
                          work=("byte", 4.0 * b * (64 + 8 + 8 + 8) * h * w, "phasenet_predict_kernel") if _lib.PROFILE is not None else None)
            else:                # the fusion variants (section 18): 4 * num_img amplitude planes, 12 predictions for three images
                if c != 4 * n_img:
                    raise RuntimeError(f"PhaseNet(num_img={n_img}): level {idx} has {c} phase planes, expected {4 * n_img}")
                _, p_out, a_out = ops.phasenet_predict_n(fp[:, :64], cp, amp_in, self.max_amplitudes[idx], n_img, pred=fp[:, 64:])
            phases.append(p_out); amps.append(a_out)
        for _ in range(self.pyr.height - 2 - m):                                           # :91-93
            phases.append(0); amps.append(0)
        return DecompValues(high, phases[::-1], amps[::-1], low)

    def _forward_grad(self, vals, m):
        """The same walk as a graph of the nodes of vfi_amd/phase_net/grad.py, in the reference's
        channel order [feature | phase | amp | prediction]: fixed-statistics fine-tuning.  Taken only after fine_tune(), with grad
        mode on and a parameter of self.layers requiring grad -- or, after fine_tune(batch_stats=True), by every call (section 17:
        each block takes its batch's statistics; the shared last block takes fresh ones at every level it serves and moves its
        running statistics once per level, coarse to fine).  The normalised inputs and the maxima get no gradient.
        Three and four input images (after fine_tune(fusion=True), section 20): block 0 sees num_img planes and predicts
        pred_channels[0], a band level brings 4 * num_img phase and amplitude planes, and the heads are the _n entry points."""
        from . import grad as G
        n_img = self.num_img
        low_in = vals.low_level.detach().contiguous()
        if low_in.shape[1] != n_img:
            raise RuntimeError(f"PhaseNet(num_img={n_img}): the low level has {low_in.shape[1]} images")
        f, c = G.block_forward(self.layers[0], low_in)                                     # :113
        low = G.blend_low(c, low_in, self.max_low_level, n_img)                            # :115-121 + :96-98
        hs = vals.high_level.shape
        high = torch.zeros((hs[0], 1, hs[2], hs[3]), dtype=torch.float32, device=low_in.device)   # :127-128
        phases, amps = [], []
        for idx in range(m):
            ph, am = vals.phase[idx].detach(), vals.amplitude[idx].detach()
            i = idx + 1 if idx + 1 < len(self.layers) - 1 else len(self.layers) - 1        # :148
            blk = self.layers[i]
            if ph.shape[1] != 4 * n_img:
                raise RuntimeError(f"PhaseNet(num_img={n_img}): level {idx} has {ph.shape[1]} phase planes, expected {4 * n_img}")
            x = G.level_input(f, c, ph, am)                                                # :138-141
            f = G.block_features(blk, x)
            c, p_out, a_out = G.level_head(blk, f, am, self.max_amplitudes[idx], n_img)    # :149-168 + :80-90
            phases.append(p_out); amps.append(a_out)
        for _ in range(self.pyr.height - 2 - m):                                           # :91-93
            phases.append(0); amps.append(0)
        return DecompValues(high, phases[::-1], amps[::-1], low)
