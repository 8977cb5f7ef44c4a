"""FusionNet -- mirror of reference src/fusion_net/fusion_net.py (same constructor, state-dict keys
and forward signature), executed as libvfi_hip.so calls on the MI355X.

forward (fusion_net.py:46-77): cat(base, adacof, phase, other, maps) -> 3 x [conv, ReLU, skip, maxpool]
-> bottleneck -> 3 x [ReLU, bilinear x2, + skip, conv] -> tanh -> base|phase + res -> clamp(0,1).
Fusions: ReLU in the conv epilogue; `deconvolution(relu(x)) + s` is one resize launch; tanh + add +
clamp is one launch.  The checkpoint's unused `net.*` stack (fusion_net.py:11-20) is kept as
parameters only so `load_state_dict` stays strict.
"""
import torch

from .. import ops
from ..nn_util import ConvParams, Indexed, PackedModule


class FusionNet(PackedModule):
    def __init__(self, num_imgs=5, uncertainty_maps=3, kernel=3, pad=3, dil=3):
        super().__init__()
        cin = 3 * num_imgs + uncertainty_maps
        self.in_channels = cin
        # dead stack of the reference (fusion_net.py:11-20): parameters only
        self.net = Indexed({0: ConvParams(cin, 64, kernel), 2: ConvParams(64, 64, kernel),
                            4: ConvParams(64, 64, kernel), 6: ConvParams(64, 3, kernel)})
        self.encoder_layers = Indexed({0: ConvParams(cin, 32, 5), 1: ConvParams(32, 64, 5), 2: ConvParams(64, 128, 3)})
        self.bottleneck_layer = ConvParams(128, 128, 3)
        self.decoder_layers = Indexed({0: ConvParams(128, 64, 5), 1: ConvParams(64, 32, 5), 2: ConvParams(32, 3, 1)})
        self.residuals = []
        self.train(False)

    def _build_packed(self):
        return {"enc": [self.pack(self.encoder_layers[i]) for i in range(3)],
                "mid": self.pack(self.bottleneck_layer),
                "dec": [self.pack(self.decoder_layers[i]) for i in range(3)]}

    def _live_convs(self):
        """The 7 convolutions forward() runs, in execution order (the `net.*` stack is not among them)."""
        return [self.encoder_layers[i] for i in range(3)] + [self.bottleneck_layer] + [self.decoder_layers[i] for i in range(3)]

    def packed_transposed(self):
        """W.transpose(0,1).flip(2,3) packs of the live convolutions for their input gradients, built on the first backward
        after a parameter change and cached beside the forward packs (same key, same host wait as `packed()`)."""
        p = self.packed()
        if "T" not in p:
            with torch.no_grad():
                p["T"] = [ops.packed_transposed(c.weight) for c in self._live_convs()]
            dev = next(self.parameters()).device
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
        return p["T"]

    def train(self, mode=True):
        """FusionNet has no BatchNorm and no dropout: the mode changes no arithmetic.  Training mode only lets forward()
        record the autograd graph when parameters alone require grad (see forward)."""
        return torch.nn.Module.train(self, mode)

    def forward(self, base, adacof, phase, other, maps, save=False, variant=0):
        """With grad mode on and an input requiring grad -- or the module in training mode with a parameter requiring grad --
        the same kernels run as one autograd node (_FusionNetFunction) whose backward is HIP; otherwise the plain
        inference path runs (eval-mode callers that never backpropagate keep a result without a grad_fn)."""
        params = [t for c in self._live_convs() for t in (c.weight, c.bias)]
        inputs = [base, adacof, phase, other, maps]
        if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in inputs) or
                                        (self.training and any(t.requires_grad for t in params))):
            out = _FusionNetFunction.apply(self, variant, *inputs, *params)
        else:
            out = self._forward_impl(self.packed(), base, adacof, phase, other, maps, variant, None)
        if save:
            self.residuals.append(float((out - (phase if variant == 1 else base)).sum().item()))
        return out

    def _forward_impl(self, p, base, adacof, phase, other, maps, variant, keep):
        """The inference kernel sequence; `keep` (a dict or None) receives the tensors the backward needs -- tensors the
        forward produces anyway, so the result is bit-identical either way."""
        parts = [base, adacof, phase, other] + ([maps] if maps is not None else [])
        n, _, h, w = base.shape
        if h % 8 or w % 8:
            raise ops.VfiLibraryError(f"FusionNet needs H, W multiples of 8, got {h}x{w}")
        x = ops.new((n, self.in_channels, h, w), base)
        c0 = 0
        for t in parts:                                   # torch.cat of fusion_net.py:49
            ops.affine_slice(t.contiguous(), x[:, c0:c0 + t.shape[1]])
            c0 += t.shape[1]
        assert c0 == self.in_channels
        enc_in, skip = [x], []
        for i in range(3):                                # fusion_net.py:55-59
            s, x = ops.conv2d_pool2(x, p["enc"][i], True, "reflect", "relu")     # conv + ReLU, and its MaxPool2d(2)
            skip.append(s)
            enc_in.append(x)
        x = ops.conv2d(x, p["mid"], "reflect", None)      # :61
        dec_src, dec_in = [x], []
        for i, s in enumerate(skip[::-1]):                # :63-67
            x = ops.resize_bilinear(x, s.shape[2:], align_corners=False, relu_input=True, residual=s)
            dec_in.append(x)
            x = ops.conv2d(x, p["dec"][i], "reflect", None)
            dec_src.append(x)
        head_base = (phase if variant == 1 else base).contiguous()
        out = ops.tanh_residual_clamp(x, head_base)   # :69-77
        if keep is not None:
            keep.update(enc_in=enc_in, skip=skip, dec_src=dec_src, dec_in=dec_in, head_base=head_base,
                        widths=[t.shape[1] for t in parts])
        return out


class _FusionNetFunction(torch.autograd.Function):
    """FusionNet.forward as one autograd node.  Inputs: (net, variant, base, adacof, phase, other, maps, then weight and
    bias of the 7 live convolutions in execution order).  The backward walks the network in reverse with HIP kernels only:
    vfi_tanh_residual_clamp_backward for the head; per decoder level a weight gradient, an input gradient and
    vfi_resize_bilinear_backward (ReLU mask of the resize source; the skip's gradient is the resize output's); the
    bottleneck's two gradients; per encoder level vfi_pool2_max_backward (pool routing + skip, ReLU mask), a weight gradient
    and -- except at the first level when no input needs a gradient -- an input gradient, split over the input slices."""

    @staticmethod
    def forward(ctx, net, variant, base, adacof, phase, other, maps, *params):
        keep = {}
        out = net._forward_impl(net.packed(), base, adacof, phase, other, maps, variant, keep)
        ctx.net, ctx.variant, ctx.keep = net, variant, keep
        ctx.has_maps = maps is not None
        ctx.save_for_backward(*params)      # in-place changes between forward and backward raise, as for torch layers
        return out

    @staticmethod
    def backward(ctx, grad_out):
        net, k, variant = ctx.net, ctx.keep, ctx.variant
        ctx.saved_tensors                   # the version check of save_for_backward
        need = ctx.needs_input_grad
        need_in = need[2:7]                 # base, adacof, phase, other, maps
        pT = net.packed_transposed()
        convs = net._live_convs()
        g = grad_out.contiguous()
        head_slot = 2 if variant == 1 else 0    # the residual base is `phase` for variant 1, `base` otherwise
        gx, g_head_base = ops.tanh_residual_clamp_backward(k["dec_src"][3], k["head_base"], g,
                                                           need_base=bool(need[2 + head_slot]))
        pgrads = [None] * 14

        def layer(li, x, dy, want_dx):
            if need[7 + 2 * li] or need[8 + 2 * li]:
                dw, db = ops.conv2d_backward_weight(x, dy, convs[li].weight.shape[2], "reflect", bias=bool(need[8 + 2 * li]))
                pgrads[2 * li], pgrads[2 * li + 1] = dw, db
            return ops.conv2d_backward_data(dy, pT[li], "reflect") if want_dx else None

        # decoder (fusion_net.py:63-67): level i reads resize(relu(dec_src[i])) + skip[2-i]
        skip_grads = [None] * 3
        for i in (2, 1, 0):
            g_in = layer(4 + i, k["dec_in"][i], gx, True)
            skip_grads[2 - i] = g_in
            gx = ops.resize_bilinear_backward(k["dec_src"][i], g_in, relu_input=True)
        gx = layer(3, k["enc_in"][3], gx, True)            # bottleneck :61
        any_in = any(need_in)
        for i in (2, 1, 0):                                 # encoder :55-59
            gy = ops.pool2_max_backward(k["skip"][i], gx, skip_grads[i])
            gx = layer(i, k["enc_in"][i], gy, i > 0 or any_in)
        grads = [None] * 5
        if any_in:
            c0 = 0
            for slot, width in enumerate(k["widths"]):
                if need_in[slot]:
                    grads[slot] = gx[:, c0:c0 + width]
                c0 += width
        if g_head_base is not None:
            grads[head_slot] = g_head_base if grads[head_slot] is None else grads[head_slot] + g_head_base
        pgrads = [gp if need[7 + j] else None for j, gp in enumerate(pgrads)]
        ctx.keep = None
        return (None, None, *grads, *pgrads)
