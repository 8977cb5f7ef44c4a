"""Plain AdaCoF network -- mirror of reference src/adacof/models/adacofnet.py.

Eval mode returns frame1 through the inference path of the fusion variant (adacofnet.py:218-219).  Training mode returns
the reference's dict {'frame1', 'g_Spatial', 'g_Occlusion'} (adacofnet.py:202-217) from one autograd node whose backward is
HIP: the frames get no gradient (the reference's sampler returns zeros for it and moduleNormalize
only feeds the estimator), the parameters of `get_kernel` get theirs.
"""
import sys

import torch

from ... import ops
from ...fusion_net import fusion_adacofnet as _f
from ..cupy_module.adacof import adacof_fused, adacof_backward

CHARBONNIER_EPSILON = 0.001      # utility.py:67


def make_model(args):
    return AdaCoFNet(args).to(torch.device("cuda:{}".format(args.gpu_id)))


KernelEstimation = _f.KernelEstimation


class AdaCoFNet(_f.AdaCoFNet):
    def train(self, mode=True):
        """KernelEstimation has no BatchNorm and no dropout: the mode changes no arithmetic, only what forward returns."""
        return torch.nn.Module.train(self, mode)

    def forward(self, frame0, frame2):
        if not self.training:
            return super().forward(frame0, frame2)[2]      # adacofnet.py:216-219 (eval branch)
        if int(frame0.shape[2]) != int(frame2.shape[2]) or int(frame0.shape[3]) != int(frame2.shape[3]):
            sys.exit("Frame sizes do not match")           # adacofnet.py:175-176
        frame1, g_spatial, g_occlusion = _AdaCoFNetFunction.apply(self, frame0, frame2, *self.get_kernel.parameters())
        return {"frame1": frame1, "g_Spatial": g_spatial, "g_Occlusion": g_occlusion}


class _AdaCoFNetFunction(torch.autograd.Function):
    """AdaCoFNet.forward's training branch as one autograd node: (net, frame0, frame2, *get_kernel parameters) ->
    (frame1 cropped to the input size, g_Spatial, g_Occlusion).

    Forward: vfi_adacof_prepare (reflect pad to /32, planar), KernelEstimation.forward_train, the channel softmax, both
    samplings + blend in one vfi_adacof_fused launch (sides kept), vfi_adacof_smooth_forward.
    Backward: vfi_adacof_blend_backward (blend, crop, occlusion smoothness, sigmoid), vfi_adacof_backward per side on the
    replication-padded planar frames (vfi_replicate_pad), vfi_adacof_head_backward per side (spatial smoothness + softmax),
    then KernelEstimation.backward_train."""

    @staticmethod
    def forward(ctx, net, frame0, frame2, *params):
        est = net.get_kernel
        h0, w0 = int(frame0.shape[2]), int(frame0.shape[3])
        pad0, pad2, x6 = ops.adacof_prepare(frame0.detach().contiguous(), frame2.detach().contiguous(), rgbx=False)
        keep = {}
        w1, a1, b1, w2, a2, b2, occ = est.forward_train(x6, keep)
        ops.softmax_channels_(w1)
        ops.softmax_channels_(w2)
        t1, t2, frame1, _ = adacof_fused(pad0, pad2, w1, a1, b1, w2, a2, b2, occ, net.dilation, want_sides=True,
                                         want_mask=False)
        m, terms = ops.adacof_smooth_forward(w1, a1, b1, w2, a2, b2, occ, CHARBONNIER_EPSILON)
        if x6.shape[2] != h0 or x6.shape[3] != w0:
            frame1 = frame1[:, :, :h0, :w0].contiguous()    # adacofnet.py:197-200
        keep.update(pad0=pad0, pad2=pad2, maps=(w1, a1, b1, w2, a2, b2, occ), t1=t1, t2=t2, m=m)
        ctx.net, ctx.keep = net, keep
        ctx.save_for_backward(*params)      # in-place changes between forward and backward raise, as for torch layers
        return frame1, terms[0], terms[1]

    @staticmethod
    def backward(ctx, g_frame, g_spatial, g_occlusion):
        net, k = ctx.net, ctx.keep
        ctx.saved_tensors                   # the version check of save_for_backward
        est = net.get_kernel
        w1, a1, b1, w2, a2, b2, occ = k["maps"]
        g_t1, g_t2, g_z = ops.adacof_blend_backward(g_frame.contiguous(), k["t1"], k["t2"], occ,
                                                    g_occlusion.contiguous(), CHARBONNIER_EPSILON)
        heads = []
        for side, (pad, w, a, b, g_t) in enumerate(((k["pad0"], w1, a1, b1, g_t1), (k["pad2"], w2, a2, b2, g_t2))):
            frame = ops.replicate_pad(pad, net.kernel_pad)                       # adacofnet.py:193-194
            gw, ga, gb = adacof_backward(g_t, frame, w, a, b, net.dilation)
            heads += ops.adacof_head_backward(gw, ga, gb, w, a, b, k["m"][:, 2 * side:2 * side + 1],
                                              k["m"][:, 2 * side + 1:2 * side + 2], g_spatial.contiguous(),
                                              CHARBONNIER_EPSILON)
        names = [n for n, _ in est.named_parameters()]
        need = {n: bool(f) for n, f in zip(names, ctx.needs_input_grad[3:])}
        grads = est.backward_train(k, (*heads, g_z), need)
        ctx.keep = None
        return (None, None, None, *[grads.get(n) if need[n] else None for n in names])
