"""The differentiable pieces one PhaseNet level is made of: `PhaseNetBlock.forward` as an autograd
node with a HIP backward, and differentiable wrappers of the level's resize and blends.  Each wrapper is a passthrough to
the existing op when grad mode is off or nothing requires grad, so inference callers see the same kernels and bits.

    f, c = blk(x)                                     # reference block.py:28-32
    x1 = torch.cat((resize_bilinear(f, size), phase, amp, resize_bilinear(c, size)), 1)      # phase_net.py:138-141
    phase_out, amp_out = blend_level(c1, amp, max_amp)                                       # phase_net.py:155-168, :80-90
    low_out = blend_low(c0, low, max_low)                                                    # phase_net.py:113-116, :96-98
"""
import torch

from .. import ops


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---- the block -------------------------------------------------------------------------------------------------------
def block_packs(blk):
    """(conv 1 with the BatchNorm's running statistics folded, conv 2, prediction map) as ops.PackedConv, cached on the
    block and keyed on the parameters' and buffers' version counters, so an optimiser step rebuilds them at the next call
    (section 12's rule).  x is in the reference's channel order: no permutation here."""
    fm, pm = blk.feature_map, blk.prediction_map
    tensors = [fm[0].weight, fm[0].bias, fm[1].weight, fm[1].bias, fm[1].running_mean, fm[1].running_var,
               fm[3].weight, fm[3].bias, pm[0].weight, pm[0].bias]
    key = tuple((id(t), t._version, t.device) for t in tensors)
    cache = blk.__dict__.get("_vfi_packs")
    if cache is None or cache["key"] != key:
        with torch.no_grad():
            cache = {"key": key,
                     "fwd": (ops.PackedConv(fm[0].weight, fm[0].bias, bn=fm[1].fold_args()),
                             ops.PackedConv(fm[3].weight, fm[3].bias), ops.PackedConv(pm[0].weight, pm[0].bias))}
        blk.__dict__["_vfi_packs"] = cache
        torch.cuda.current_stream(fm[0].weight.device).synchronize()      # as PackedModule.packed(): other streams may follow
    return cache


def _bn_scale(bn):
    return bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)


def block_packs_transposed(blk):
    """W.transpose(0,1).flip(2,3) packs of the three convolutions (conv 1: of the folded weights), built on the first
    backward after a parameter change and cached beside the forward packs."""
    cache = block_packs(blk)
    if "T" not in cache:
        fm, pm = blk.feature_map, blk.prediction_map
        with torch.no_grad():
            wf = fm[0].weight.detach() * _bn_scale(fm[1]).view(-1, 1, 1, 1)
            cache["T"] = (ops.packed_transposed(wf), ops.packed_transposed(fm[3].weight), ops.packed_transposed(pm[0].weight))
        torch.cuda.current_stream(fm[0].weight.device).synchronize()
    return cache["T"]


def block_launches(packs, x):
    """The block's three launches (BN folded, ELU / tanh in the epilogues, reflect padding for 3x3) -> (t, f, c), t the
    post-ELU output of conv 1."""
    c1, c2, cp = packs
    mode = "reflect" if c1.ks == 3 else "zeros"
    t = ops.conv2d(x, c1, mode, "elu")
    f = ops.conv2d(t, c2, mode, "elu")
    c = ops.conv2d(f, cp, "zeros", "tanh")
    return t, f, c


def block_forward(blk, x):
    """PhaseNetBlock.forward: (f, c) = (feature_map(x), prediction_map(f)) with BN on its running statistics."""
    if blk.training:
        raise NotImplementedError("PhaseNetBlock in training mode needs batch-statistics BatchNorm, which is not built; "
                                  "call .eval() to fine-tune on the running statistics")
    fm, pm = blk.feature_map, blk.prediction_map
    params = (fm[0].weight, fm[0].bias, fm[1].weight, fm[1].bias, fm[3].weight, fm[3].bias, pm[0].weight, pm[0].bias)
    if _wants_grad(x, *params):
        return _BlockFunction.apply(blk, x, *params)
    _, f, c = block_launches(block_packs(blk)["fwd"], x)
    return f, c


class _BlockFunction(torch.autograd.Function):
    """One PhaseNet block as one autograd node.  Inputs: (blk, x, then w1, b1, gamma, beta, w2, b2, wp, bp).  The forward
    runs exactly the inference launches and keeps t (post-ELU conv 1), f and c.  Backward: tanh backward -> 1x1 weight and
    data gradient -> + g_f -> ELU backward on f -> conv 2 weight and data gradient -> ELU backward on t -> conv 1 weight
    gradient (data gradient only when x needs one) -> the folded BatchNorm unfolded on parameter-sized tensors."""

    @staticmethod
    def forward(ctx, blk, x, *params):
        t, f, c = block_launches(block_packs(blk)["fwd"], x)
        ctx.blk, ctx.t = blk, t
        ctx.save_for_backward(x, f, c, *params)       # in-place changes between forward and backward raise
        ctx.set_materialize_grads(False)
        return f, c

    @staticmethod
    def backward(ctx, g_f, g_c):
        blk, t = ctx.blk, ctx.t
        x, f, c = ctx.saved_tensors[:3]
        need = ctx.needs_input_grad             # (blk, x, w1, b1, gamma, beta, w2, b2, wp, bp)
        fm = blk.feature_map
        ks = fm[0].weight.shape[2]
        mode = "reflect" if ks == 3 else "zeros"
        pT1, pT2, pTp = block_packs_transposed(blk)
        grads = [None] * 8
        first = any(need[2:6])                      # conv 1 or its BatchNorm
        below = first or need[1] or need[6] or need[7]      # anything under the prediction map
        g = g_f.contiguous() if g_f is not None else None
        if g_c is not None:
            gz = ops.act_backward_(g_c.contiguous(), c, "tanh", out=torch.empty_like(c))
            if need[8] or need[9]:
                grads[6], grads[7] = ops.conv2d_backward_weight(f, gz, 1, "zeros", bias=bool(need[9]))
            if below:
                g_head = ops.conv2d_backward_data(gz, pTp, "zeros")
                g = g_head if g is None else ops.add(g, g_head)
        elif g is not None and below:
            g = g.clone()
        if g is None or not below:
            ctx.t = None
            return (None, None, *[gp if need[2 + j] else None for j, gp in enumerate(grads)])
        ops.act_backward_(g, f, "elu")
        if need[6] or need[7]:
            grads[4], grads[5] = ops.conv2d_backward_weight(t, g, ks, mode, bias=bool(need[7]))
        gx = None
        if first or need[1]:
            g_t = ops.conv2d_backward_data(g, pT2, mode)
            ops.act_backward_(g_t, t, "elu")
            if first:
                g_wf, g_bf = ops.conv2d_backward_weight(x, g_t, ks, mode, bias=True)
                # y = conv(x, w s) + (b - mean) s + beta with s = gamma / sqrt(var + eps)
                bn = fm[1]
                inv = 1.0 / torch.sqrt(bn.running_var + bn.eps)
                s = bn.weight.detach() * inv
                w, b = fm[0].weight.detach(), fm[0].bias.detach()
                grads[0] = g_wf * s.view(-1, 1, 1, 1)
                grads[1] = g_bf * s
                grads[2] = ((g_wf * w).sum((1, 2, 3)) + g_bf * (b - bn.running_mean)) * inv
                grads[3] = g_bf
            if need[1]:
                gx = ops.conv2d_backward_data(g_t, pT1, mode)
        grads = [gp if need[2 + j] else None for j, gp in enumerate(grads)]
        ctx.t = None
        return (None, gx, *grads)


# ---- resize and blends -----------------------------------------------------------------------------------------------
class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.src = tuple(x.shape[2:])
        return ops.resize_bilinear(x, size, align_corners=False)

    @staticmethod
    def backward(ctx, g):
        return ops.resize_bilinear_adjoint(g.contiguous(), ctx.src), None


def resize_bilinear(x, size):
    """nn.Upsample(size, mode='bilinear') of phase_net.py:138-139 (align_corners=False, any size), differentiable."""
    size = (int(size[0]), int(size[1]))
    if _wants_grad(x):
        return _Resize.apply(x, size)
    return ops.resize_bilinear(x, size, align_corners=False)


class _BlendLevel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, amp_in, max_amp):
        ctx.save_for_backward(amp_in, max_amp)
        ctx.set_materialize_grads(False)
        return ops.phasenet_emit(pred, amp_in, max_amp)

    @staticmethod
    def backward(ctx, g_phase, g_amp):
        if g_phase is None and g_amp is None:
            return None, None, None
        amp_in, max_amp = ctx.saved_tensors
        c = lambda g: g.contiguous() if g is not None else None
        return ops.phasenet_emit_backward(c(g_phase), c(g_amp), amp_in, max_amp), None, None


def blend_level(pred, amp_in, max_amp):
    """One band level's de-normalised outputs from its prediction map (phase_net.py:155-168 + reverse_normalize :80-90):
    pred (N,8,H,W), amp_in (N,8,H,W) the normalised input amplitudes, max_amp (N,) -> (phase, amp), each (N*4,1,H,W).
    Differentiable in pred; amp_in and max_amp get no gradient."""
    if _wants_grad(pred):
        return _BlendLevel.apply(pred, amp_in.detach(), max_amp.detach())
    return ops.phasenet_emit(pred, amp_in, max_amp)


class _BlendLow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, low_in, max_low):
        ctx.save_for_backward(low_in, max_low)
        return ops.phasenet_emit_low(pred, low_in, max_low)

    @staticmethod
    def backward(ctx, g_low):
        low_in, max_low = ctx.saved_tensors
        return ops.phasenet_emit_low_backward(g_low.contiguous(), low_in, max_low), None, None


def blend_low(pred, low_in, max_low):
    """The low level's de-normalised output (phase_net.py:113-116 + :96-98): pred (N,1,H,W), low_in (N,2,H,W) normalised,
    max_low (N,) -> (N,1,H,W).  Differentiable in pred."""
    if _wants_grad(pred):
        return _BlendLow.apply(pred, low_in.detach(), max_low.detach())
    return ops.phasenet_emit_low(pred, low_in, max_low)
