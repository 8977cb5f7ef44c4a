"""AdaCoF network, fusion variant -- mirror of reference src/fusion_net/fusion_adacofnet.py.

`make_model(args)` (fusion_adacofnet.py:10-11) is the plugin entry the reference's
`src.adacof.models.Model` resolves by dotted module path; `AdaCoFNet.forward(frame0, frame2)` returns
`(tensorAdaCoF1, tensorAdaCoF2, frame1, UncertaintyMask)` (fusion_adacofnet.py:172-240).

Execution on the MI355X:
  * prologue (reflect pad to /32, mean subtraction, concat): one launch (vfi_adacof_prepare);
  * KernelEstimation U-Net (fusion_adacofnet.py:109-155): fp32-MFMA convs with ReLU and the additive skip
    fused in the epilogue; the seven heads' first convs share their input and run as ONE 64->448 conv,
    their second/third convs read channel slices of its output in place;
  * both AdaCoF samplings + occlusion blend + flow-variance mask: one launch (vfi_adacof_fused); the
    ReplicationPad2d is folded into the sampler's clamp.
"""
import sys

import torch

from .. import _lib, ops
from ..adacof.cupy_module.adacof import FunctionAdaCoF, adacof_fused
from ..nn_util import ConvParams, Indexed, PackedModule

HEADS = ("moduleWeight1", "moduleAlpha1", "moduleBeta1", "moduleWeight2", "moduleAlpha2", "moduleBeta2",
         "moduleOcclusion")


def make_model(args):
    return AdaCoFNet(args).to(torch.device("cuda:{}".format(args.gpu_id)))


def _basic(cin, cout):
    return Indexed({0: ConvParams(cin, cout, 3), 2: ConvParams(cout, cout, 3), 4: ConvParams(cout, cout, 3)})


class KernelEstimation(PackedModule):
    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size
        k2 = kernel_size ** 2
        self.moduleConv1 = _basic(6, 32)
        self.moduleConv2 = _basic(32, 64)
        self.moduleConv3 = _basic(64, 128)
        self.moduleConv4 = _basic(128, 256)
        self.moduleConv5 = _basic(256, 512)
        self.moduleDeconv5 = _basic(512, 512)
        self.moduleUpsample5 = Indexed({1: ConvParams(512, 512, 3)})
        self.moduleDeconv4 = _basic(512, 256)
        self.moduleUpsample4 = Indexed({1: ConvParams(256, 256, 3)})
        self.moduleDeconv3 = _basic(256, 128)
        self.moduleUpsample3 = Indexed({1: ConvParams(128, 128, 3)})
        self.moduleDeconv2 = _basic(128, 64)
        self.moduleUpsample2 = Indexed({1: ConvParams(64, 64, 3)})
        for name in HEADS[:6]:
            setattr(self, name, Indexed({0: ConvParams(64, 64, 3), 2: ConvParams(64, 64, 3),
                                         4: ConvParams(64, k2, 3), 7: ConvParams(k2, k2, 3)}))
        self.moduleOcclusion = Indexed({0: ConvParams(64, 64, 3), 2: ConvParams(64, 64, 3),
                                        4: ConvParams(64, 64, 3), 7: ConvParams(64, 1, 3)})
        self.train(False)

    def _build_packed(self):
        p = {}
        for name in ("moduleConv1", "moduleConv2", "moduleConv3", "moduleConv4", "moduleConv5", "moduleDeconv5",
                     "moduleDeconv4", "moduleDeconv3", "moduleDeconv2"):
            m = getattr(self, name)
            p[name] = [self.pack(m[i]) for i in (0, 2, 4)]
        for name in ("moduleUpsample5", "moduleUpsample4", "moduleUpsample3", "moduleUpsample2"):
            p[name] = self.pack(getattr(self, name)[1])
        # the seven heads' first convs share their input: one 64 -> 7*64 filter bank
        w = torch.cat([getattr(self, h)[0].weight for h in HEADS], 0)
        b = torch.cat([getattr(self, h)[0].bias for h in HEADS], 0)
        p["heads0"] = ops.PackedConv(w, b)
        for h in HEADS:
            m = getattr(self, h)
            p[h] = [self.pack(m[2]), self.pack(m[4]), self.pack(m[7])]
        # occlusion tail Upsample -> Conv2d(64, 1, 3): channel reduction as a 1x1 conv (taps as output channels) at
        # low resolution, finished by vfi_upsample2x_tapsum (exact by linearity)
        w7 = self.moduleOcclusion[7].weight                              # (1, 64, 3, 3)
        p["occ_taps"] = ops.PackedConv(w7[0].permute(1, 2, 0).reshape(9, -1, 1, 1).contiguous(), None)
        p["occ_bias"] = float(self.moduleOcclusion[7].bias.item())
        return p

    def _basic(self, convs, x):
        for pc in convs:
            x = ops.conv2d(x, pc, "zeros", "relu")
        return x

    def _basic_pooled(self, convs, x):
        """Basic block followed by AvgPool2d(2): -> (block output, pooled output), the pooling fused into the last conv."""
        for pc in convs[:-1]:
            x = ops.conv2d(x, pc, "zeros", "relu")
        return ops.conv2d_pool2(x, convs[-1], False, "zeros", "relu")

    def _up(self, pc, x, skip):
        """Upsample(x2, align_corners=True) -> conv -> ReLU, + skip (fusion_adacofnet.py:28-33,128-146)."""
        return ops.conv2d(x, pc, "zeros", "relu", residual=skip, upsample2x=True)

    def forward_x6(self, x6, softmax=True):
        """softmax=False returns the Subnet_weight LOGITS (the sampler folds the softmax in).  In training mode with grad
        mode on and a parameter requiring grad, the same layers run as one autograd node whose backward is HIP
        (softmaxed weights only); otherwise the inference sequence below runs."""
        if softmax and self.wants_graph():
            return _KernelEstimationFunction.apply(self, x6, *self.parameters())
        p = self.packed()
        c1, q1 = self._basic_pooled(p["moduleConv1"], x6)          # (c1 itself is not a skip connection; q = AvgPool2d(c))
        c2, q2 = self._basic_pooled(p["moduleConv2"], q1)
        c3, q3 = self._basic_pooled(p["moduleConv3"], q2)
        c4, q4 = self._basic_pooled(p["moduleConv4"], q3)
        c5, q5 = self._basic_pooled(p["moduleConv5"], q4)
        x = self._basic(p["moduleDeconv5"], q5)
        x = self._up(p["moduleUpsample5"], x, c5)
        x = self._up(p["moduleUpsample4"], self._basic(p["moduleDeconv4"], x), c4)
        x = self._up(p["moduleUpsample3"], self._basic(p["moduleDeconv3"], x), c3)
        x = self._up(p["moduleUpsample2"], self._basic(p["moduleDeconv2"], x), c2)
        n, _, h, w = x.shape
        h0 = ops.conv2d(x, p["heads0"], "zeros", "relu")            # (N, 448, h, w)
        outs = []
        for i, name in enumerate(HEADS):
            c_mid, c_up, c_out = p[name]
            t = ops.conv2d(h0[:, 64 * i:64 * (i + 1)], c_mid, "zeros", "relu")
            t = ops.conv2d(t, c_up, "zeros", "relu")
            # Upsample(x2, align_corners=True) -> conv: one launch, the upsampled tensor is never written
            if name.startswith("moduleWeight"):
                t = ops.conv2d(t, c_out, "zeros", None, upsample2x=True)
                if softmax:
                    t = ops.softmax_channels_(t)
            elif name == "moduleOcclusion":
                taps = ops.conv2d(t, p["occ_taps"], "zeros", None)                  # (N, 9, h, w)
                t = ops.new((n, 1, 2 * h, 2 * w), t)
                _lib.call("vfi_upsample2x_tapsum", taps.data_ptr(), t.data_ptr(), n, h, w, p["occ_bias"], 4,
                          _lib.stream_ptr())
            else:
                t = ops.conv2d(t, c_out, "zeros", None, upsample2x=True)
            outs.append(t)
        return tuple(outs)

    def forward(self, rfield0, rfield2):
        """Reference signature (fusion_adacofnet.py:109): two mean-subtracted (N,3,H,W) frames."""
        return self.forward_x6(torch.cat([rfield0, rfield2], 1).contiguous())

    # ---- training ----------------------------------------------------------------------------
    def train(self, mode=True):
        """No BatchNorm, no dropout: the mode changes no arithmetic.  Training mode only lets forward / forward_x6 record
        the autograd graph (one node, HIP backward) when a parameter requires grad."""
        return torch.nn.Module.train(self, mode)

    def wants_graph(self):
        """FusionNet.forward's rule: grad mode on, module training, a parameter requiring grad."""
        return torch.is_grad_enabled() and self.training and any(t.requires_grad for t in self.parameters())

    def live_convs(self):
        """(name, ConvParams) of the 59 convolutions in state-dict order (all of them run)."""
        return [(k, m) for k, m in self.named_modules() if isinstance(m, ConvParams)]

    def packed_transposed(self):
        """W.transpose(0,1).flip(2,3) packs for the input gradients, keyed by module name (`heads0`: the 448 -> 64 pack of
        the seven heads' shared first convolution), cached beside the forward packs as FusionNet.packed_transposed does.
        The first layer's is never needed."""
        p = self.packed()
        if "T" not in p:
            with torch.no_grad():
                t = {k: ops.packed_transposed(m.weight) for k, m in self.live_convs()
                     if k != "moduleConv1.0" and not (k.endswith(".0") and k.split(".")[0] in HEADS)}
                t["heads0"] = ops.packed_transposed(torch.cat([getattr(self, h)[0].weight for h in HEADS], 0))
                p["T"] = t
            dev = next(self.parameters()).device
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
        return p["T"]

    def forward_train(self, x6, keep):
        """The layers of forward_x6 with everything the backward needs kept in `keep`: every ReLU output, the block
        inputs, the upsampled inputs of the upsample -> conv pairs, and relu(conv(up(x))) apart from the skip it is added
        to (the ReLU's mask cannot be recovered from the sum).  -> (W1 logits, A1, B1, W2 logits, A2, B2, sigmoid Occ)."""
        p = self.packed()

        def block(name, x, pooled):
            acts = [x]
            for pc in p[name][:-1]:
                acts.append(ops.conv2d(acts[-1], pc, "zeros", "relu"))
            if pooled:
                y, q = ops.conv2d_pool2(acts[-1], p[name][-1], False, "zeros", "relu")
                return acts + [y], q
            return acts + [ops.conv2d(acts[-1], p[name][-1], "zeros", "relu")], None

        enc, x = {}, x6
        for i in range(1, 6):
            enc[i], x = block(f"moduleConv{i}", x, True)
        dec, up = {}, {}
        for i in (5, 4, 3, 2):
            dec[i], _ = block(f"moduleDeconv{i}", x, False)
            d = dec[i][-1]
            u = ops.resize_bilinear(d, (2 * d.shape[2], 2 * d.shape[3]), align_corners=True)
            r = ops.conv2d(u, p[f"moduleUpsample{i}"], "zeros", "relu")
            up[i] = (u, r)
            x = ops.add(r, enc[i][-1])
        h0 = ops.conv2d(x, p["heads0"], "zeros", "relu")            # (N, 448, h, w)
        heads, outs = {}, []
        for i, name in enumerate(HEADS):
            c_mid, c_up, c_out = p[name]
            m = ops.conv2d(h0[:, 64 * i:64 * (i + 1)], c_mid, "zeros", "relu")
            t = ops.conv2d(m, c_up, "zeros", "relu")
            u = ops.resize_bilinear(t, (2 * t.shape[2], 2 * t.shape[3]), align_corners=True)
            heads[name] = (m, t, u)
            # the occlusion tail as upsample -> 64 -> 1 conv (the tap-sum form is an inference-only rewrite)
            outs.append(ops.conv2d(u, c_out, "zeros", "sigmoid" if name == "moduleOcclusion" else None))
        keep.update(enc=enc, dec=dec, up=up, x_heads=x, h0=h0, heads=heads)
        return tuple(outs)

    def backward_train(self, keep, g_outs, need):
        """HIP backward of forward_train.  g_outs: gradients of the seven head convolutions' outputs (for Occlusion: of
        the pre-sigmoid map); need: {parameter name: bool}.  -> {parameter name: gradient}.  Gradients are produced only
        where asked; the walk stops at the last layer that something below still needs, and the first layer's input
        gradient is never computed."""
        pT = self.packed_transposed()
        convs = dict(self.live_convs())
        grads = {}
        want = lambda k: need.get(k + ".weight", False) or need.get(k + ".bias", False)
        head_keys = {h: [f"{h}.{i}" for i in (0, 2, 4, 7)] for h in HEADS}
        trunk = any(want(k) for k in convs if k.split(".")[0] not in HEADS)

        def layer(k, x, dy, want_dx, out=None):
            if want(k):
                dw, db = ops.conv2d_backward_weight(x, dy, 3, "zeros", bias=need.get(k + ".bias", False))
                grads[k + ".weight"], grads[k + ".bias"] = dw, db
            return ops.conv2d_backward_data(dy, pT[k], "zeros", out=out) if want_dx else None

        x, h0 = keep["x_heads"], keep["h0"]
        active = [h for h in HEADS if trunk or any(want(k) for k in head_keys[h])]
        g448 = ops.new(tuple(h0.shape), h0) if active else None
        for name in active:
            i = HEADS.index(name)
            sl = slice(64 * i, 64 * (i + 1))
            m, t, u = keep["heads"][name]
            below = trunk or want(f"{name}.0")
            deeper = lambda k: below or any(want(q) for q in head_keys[name][:head_keys[name].index(k)])
            g = layer(f"{name}.7", u, g_outs[i].contiguous(), deeper(f"{name}.7"))
            if g is None:
                continue
            g = ops.upsample2x_backward(g, mask_src=t)
            g = layer(f"{name}.4", m, g, deeper(f"{name}.4"))
            if g is None:
                continue
            ops.relu_mask_(g, m)
            layer(f"{name}.2", h0[:, sl], g, below, out=g448[:, sl] if below else None)
            if below:
                ops.relu_mask_(g448[:, sl], h0[:, sl])
        if len(active) == len(HEADS) and all(want(f"{h}.0") for h in HEADS):
            # the shared first convolution stays one 64 -> 448 bank: one weight-gradient call, split over the parameters
            dw, db = ops.conv2d_backward_weight(x, g448, 3, "zeros", bias=True)
            for i, h in enumerate(HEADS):
                grads[f"{h}.0.weight"], grads[f"{h}.0.bias"] = dw[64 * i:64 * (i + 1)], db[64 * i:64 * (i + 1)]
        else:
            for h in active:
                if want(f"{h}.0"):
                    i = HEADS.index(h)
                    layer(f"{h}.0", x, g448[:, 64 * i:64 * (i + 1)], False)
        if not trunk:
            return grads
        g = ops.conv2d_backward_data(g448, pT["heads0"], "zeros")   # 448 -> 64: sums the seven heads' contributions

        def block_backward(name, acts, g, want_dx):
            """g: gradient of the block's last pre-activation (already masked) -> gradient of the block's input."""
            g = layer(f"{name}.4", acts[2], g, True)
            ops.relu_mask_(g, acts[2])
            g = layer(f"{name}.2", acts[1], g, True)
            ops.relu_mask_(g, acts[1])
            return layer(f"{name}.0", acts[0], g, want_dx)

        g_skip = {}
        for i in (2, 3, 4, 5):              # decoder, in reverse: x_i = relu(conv(up(d_i))) + c_i
            u, r = keep["up"][i]
            g_skip[i] = g                   # the skip's gradient is the sum's own
            gr = ops.relu_mask_(g, r, out=ops.new(tuple(g.shape), g))
            gu = layer(f"moduleUpsample{i}.1", u, gr, True)
            acts = keep["dec"][i]
            g = block_backward(f"moduleDeconv{i}", acts, ops.upsample2x_backward(gu, mask_src=acts[3]), True)
        for i in (5, 4, 3, 2, 1):           # encoder: c_i feeds AvgPool2d(2) and (i >= 2) the skip
            acts = keep["enc"][i]
            gc = ops.pool2_avg_backward(acts[3], g, g_skip.get(i))
            g = block_backward(f"moduleConv{i}", acts, gc, i > 1)
        return grads


class _KernelEstimationFunction(torch.autograd.Function):
    """KernelEstimation.forward_x6 as one autograd node: (net, x6, *parameters) -> the seven maps.  The backward turns
    the maps' gradients into those of the head convolutions' outputs (softmax backward through vfi_adacof_head_backward
    without smoothness terms, vfi_sigmoid_backward) and walks KernelEstimation.backward_train.  x6 gets no gradient."""

    @staticmethod
    def forward(ctx, net, x6, *params):
        keep = {}
        w1, a1, b1, w2, a2, b2, occ = net.forward_train(x6, keep)
        ops.softmax_channels_(w1)
        ops.softmax_channels_(w2)
        ctx.net, ctx.keep = net, keep
        # in-place changes between forward and backward raise, as for torch layers
        ctx.save_for_backward(*params, w1, a1, b1, w2, a2, b2, occ)
        return w1, a1, b1, w2, a2, b2, occ

    @staticmethod
    def backward(ctx, *g):
        net = ctx.net
        w1, a1, b1, w2, a2, b2, occ = ctx.saved_tensors[-7:]
        g = [t.contiguous() for t in g]
        gl1, ga1, gb1 = ops.adacof_head_backward(g[0], g[1], g[2], w1, a1, b1)
        gl2, ga2, gb2 = ops.adacof_head_backward(g[3], g[4], g[5], w2, a2, b2)
        gz = ops.sigmoid_backward(g[6], occ)
        names = [k for k, _ in net.named_parameters()]
        need = {k: bool(f) for k, f in zip(names, ctx.needs_input_grad[2:])}
        grads = net.backward_train(ctx.keep, (gl1, ga1, gb1, gl2, ga2, gb2, gz), need)
        ctx.keep = None
        return (None, None, *[grads.get(k) if need[k] else None for k in names])


class AdaCoFNet(torch.nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.kernel_size = args.kernel_size
        self.kernel_pad = int(((args.kernel_size - 1) * args.dilation) / 2.0)   # fusion_adacofnet.py:163
        self.dilation = args.dilation
        self.get_kernel = KernelEstimation(self.kernel_size)
        self.moduleAdaCoF = FunctionAdaCoF.apply
        self.train(False)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("vfi_amd implements the inference path only (eval mode)")
        return super().train(False)

    def forward(self, frame0, frame2, return_sides=True):
        """The reference returns both sampled sides (tensorAdaCoF1/2, fusion_adacofnet.py:240) although its fused caller
        drops them (src/fusion_net/interpolate_twoframe.py:156,229-237).  `return_sides=False` (a per-call argument, so
        callers sharing the module never see each other's choice) makes the sampler skip their 24 B/px of stores; forward
        then returns None in their place."""
        h0, w0 = int(frame0.shape[2]), int(frame0.shape[3])
        if h0 != int(frame2.shape[2]) or w0 != int(frame2.shape[3]):
            sys.exit("Frame sizes do not match")                                 # fusion_adacofnet.py:177-178
        pad0, pad2, x6 = ops.adacof_prepare(frame0.contiguous(), frame2.contiguous(), rgbx=True)
        w1, a1, b1, w2, a2, b2, occ = self.get_kernel.forward_x6(x6, softmax=False)
        t1, t2, frame1, mask = adacof_fused(pad0, pad2, w1, a1, b1, w2, a2, b2, occ, self.dilation, rgbx=True,
                                            weights_are_logits=True, want_sides=bool(return_sides))
        if x6.shape[2] != h0 or x6.shape[3] != w0:
            # the reference's width crop assigns tensorAdaCoF1 from tensorAdaCoF2 (fusion_adacofnet.py:225);
            # both are unused downstream -- we return the correctly cropped t1.
            t1, t2, frame1, mask = (t[:, :, :h0, :w0].contiguous() if t is not None else None for t in (t1, t2, frame1, mask))
        return t1, t2, frame1, mask
