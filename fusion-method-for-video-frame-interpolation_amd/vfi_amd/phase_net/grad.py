"""The differentiable pieces one PhaseNet level is made of (DESIGN.md sections 14 and 16): `PhaseNetBlock.forward` as an
autograd node with a HIP backward, the block's feature part and a band level's head as nodes of their own (what the
coarse-to-fine walk of `PhaseNet.forward` is built from), and differentiable wrappers of the level's resize and blends.
Each wrapper is a passthrough to the existing op when grad mode is off or nothing requires grad, so inference callers see
the same kernels and bits.

    f, c = blk(x)                                     # reference block.py:28-32
    x1 = torch.cat((resize_bilinear(f, size), phase, amp, resize_bilinear(c, size)), 1)      # phase_net.py:138-141
    phase_out, amp_out = blend_level(c1, amp, max_amp)                                       # phase_net.py:155-168, :80-90
    low_out = blend_low(c0, low, max_low)                                                    # phase_net.py:113-116, :96-98

The walk's own pieces, one band level (phase_net.py:138-168):
    x = level_input(f, c, phase, amp)                 # both resizes and the concatenation, written into one buffer
    f = block_features(blk, x)                        # conv 1 + folded BN + ELU + conv 2 + ELU
    c, phase_out, amp_out = level_head(blk, f, amp, max_amp)      # vfi_phasenet_predict / vfi_phasenet_predict_backward

A block whose `batch_stats` flag is set (PhaseNetBlock.batch_statistics, PhaseNet.fine_tune(batch_stats=True)) takes the
batch-statistics route of section 17 in the same nodes: conv 1 with its raw weights, vfi_bn_stats, vfi_bn_act_forward, conv 2,
and the running statistics updated at every forward, grad mode or not.  With the flag off nothing here changes.

`level_head`, `blend_level`, `blend_low` and `head_backward_composed` take `num_img` (default 2: the calls above).  For the
fusion networks of three and four input images (section 20) they go through the `_n` entry points and their adjoints, with
the level's amplitudes and the low level passed whole (4 * num_img and num_img planes).
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


BN_MOMENTUM = 0.1      # nn.BatchNorm2d's default, which block.py:17 takes


def block_packs_raw(blk):
    """The batch-statistics route's packs: (conv 1 with its RAW weights and bias, conv 2, prediction map), and under "T" their
    transposed packs once a backward asked for them.  A cache of its own beside block_packs', keyed on the six convolution
    tensors alone: this route rewrites the running statistics at every forward, and a key that held them would rebuild
    every pack (and wait for the stream) at every level."""
    fm, pm = blk.feature_map, blk.prediction_map
    tensors = [fm[0].weight, fm[0].bias, fm[3].weight, fm[3].bias, pm[0].weight, pm[0].bias]
    key = tuple((id(t), t._version, t.device) for t in tensors)
    cache = blk.__dict__.get("_vfi_packs_raw")
    if cache is None or cache["key"] != key:
        with torch.no_grad():
            cache = {"key": key, "fwd": tuple(ops.PackedConv(tensors[i], tensors[i + 1]) for i in (0, 2, 4))}
        blk.__dict__["_vfi_packs_raw"] = cache
        torch.cuda.current_stream(fm[0].weight.device).synchronize()
    return cache


def block_packs_raw_transposed(blk):
    cache = block_packs_raw(blk)
    if "T" not in cache:
        fm, pm = blk.feature_map, blk.prediction_map
        with torch.no_grad():
            cache["T"] = tuple(ops.packed_transposed(m.weight) for m in (fm[0], fm[3], pm[0]))
        torch.cuda.current_stream(fm[0].weight.device).synchronize()
    return cache["T"]


def _forward_packs(blk):
    return (block_packs_raw(blk) if blk.batch_stats else block_packs(blk))["fwd"]


def bn_feature_launches(blk, x):
    """The feature part on batch statistics (block.py:15-21 in training mode) -> (y, t, f, mean, var): conv 1 with its raw
    weights and no activation, the batch's statistics, normalise + ELU, conv 2; then the running statistics move as
    nn.BatchNorm2d's do (momentum 0.1, unbiased variance), in place, so that their version counters move too."""
    c1, c2 = block_packs_raw(blk)["fwd"][:2]
    bn = blk.feature_map[1]
    mode = "reflect" if c1.ks == 3 else "zeros"
    y = ops.conv2d(x, c1, mode, None)
    mean, var = ops.bn_stats(y)
    t = ops.bn_act_forward(y, mean, var, bn.weight, bn.bias, bn.eps, "elu")
    f = ops.conv2d(t, c2, mode, "elu")
    n = y.shape[0] * y.shape[2] * y.shape[3]
    with torch.no_grad():
        bn.running_mean.mul_(1.0 - BN_MOMENTUM).add_(mean, alpha=BN_MOMENTUM)
        bn.running_var.mul_(1.0 - BN_MOMENTUM).add_(var, alpha=BN_MOMENTUM * n / (n - 1))
        bn.num_batches_tracked.add_(1)
    return y, t, f, mean, var


def _feature_forward(blk, x):
    """-> (t, f, bn): bn = (y, mean, var) on the batch-statistics route, None on the running statistics."""
    if blk.batch_stats:
        y, t, f, mean, var = bn_feature_launches(blk, x)
        return t, f, (y, mean, var)
    t, f = feature_launches(block_packs(blk)["fwd"], x)
    return t, f, None


def block_launches(packs, x):
    """The block's three launches (BN folded, ELU / tanh in the epilogues, reflect padding for 3x3) -> (t, f, c), t the
    post-ELU output of conv 1."""
    t, f = feature_launches(packs, x)
    return t, f, ops.conv2d(f, packs[2], "zeros", "tanh")


def feature_launches(packs, x):
    """The feature part's two launches -> (t, f)."""
    c1, c2 = packs[:2]
    mode = "reflect" if c1.ks == 3 else "zeros"
    t = ops.conv2d(x, c1, mode, "elu")
    return t, ops.conv2d(t, c2, mode, "elu")


def _check_eval(blk):
    if blk.training:
        raise NotImplementedError("PhaseNetBlock in training mode needs batch-statistics BatchNorm, which is not built; "
                                  "call .eval() to fine-tune on the running statistics")


def _feature_params(blk):
    fm = blk.feature_map
    return (fm[0].weight, fm[0].bias, fm[1].weight, fm[1].bias, fm[3].weight, fm[3].bias)


def block_forward(blk, x):
    """PhaseNetBlock.forward: (f, c) = (feature_map(x), prediction_map(f)) with BN on its running statistics, or on the
    batch's when blk.batch_stats is set."""
    _check_eval(blk)
    pm = blk.prediction_map
    params = (*_feature_params(blk), pm[0].weight, pm[0].bias)
    if _wants_grad(x, *params):
        return _BlockFunction.apply(blk, x, *params)
    if blk.batch_stats:
        _, f, _ = _feature_forward(blk, x)
        return f, ops.conv2d(f, block_packs_raw(blk)["fwd"][2], "zeros", "tanh")
    _, f, c = block_launches(block_packs(blk)["fwd"], x)
    return f, c


class _BlockFunction(torch.autograd.Function):
    """One PhaseNet block as one autograd node.  Inputs: (blk, x, then w1, b1, gamma, beta, w2, b2, wp, bp).  The forward
    runs exactly the inference launches and keeps t (post-ELU conv 1), f and c.  Backward: tanh backward -> 1x1 weight and
    data gradient -> + g_f -> ELU backward on f -> conv 2 weight and data gradient -> ELU backward on t -> conv 1 weight
    gradient (data gradient only when x needs one) -> the folded BatchNorm unfolded on parameter-sized tensors.  On the
    batch-statistics route the node also keeps (y, mean, var), and _features_backward takes vfi_bn_act_backward."""

    @staticmethod
    def forward(ctx, blk, x, *params):
        if blk.batch_stats:
            t, f, ctx.bn = _feature_forward(blk, x)
            c = ops.conv2d(f, block_packs_raw(blk)["fwd"][2], "zeros", "tanh")
        else:
            t, f, c = block_launches(block_packs(blk)["fwd"], x)
            ctx.bn = None
        ctx.blk, ctx.t = blk, t
        ctx.save_for_backward(x, f, c, *params)       # in-place changes between forward and backward raise
        ctx.set_materialize_grads(False)
        return f, c

    @staticmethod
    def backward(ctx, g_f, g_c):
        blk, t = ctx.blk, ctx.t
        x, f, c = ctx.saved_tensors[:3]
        need = ctx.needs_input_grad             # (blk, x, w1, b1, gamma, beta, w2, b2, wp, bp)
        pTp = (block_packs_raw_transposed(blk) if ctx.bn is not None else block_packs_transposed(blk))[2]
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
            ctx.t = ctx.bn = None
            return (None, None, *[gp if need[2 + j] else None for j, gp in enumerate(grads)])
        gx, grads[:6] = _features_backward(blk, x, t, f, g, need[1:8], ctx.bn)
        grads = [gp if need[2 + j] else None for j, gp in enumerate(grads)]
        ctx.t = ctx.bn = None
        return (None, gx, *grads)


def _features_backward(blk, x, t, f, g, need, bn=None):
    """The walk below the head, shared by the block node and the feature node: g, the gradient of f, is the caller's own
    tensor and is overwritten (ELU backward in place).  need = (x, w1, b1, gamma, beta, w2, b2) -> (gx, six gradients).
    bn = (y, mean, var) of a batch-statistics forward: below g_t the BatchNorm's own adjoint (vfi_bn_act_backward, in place
    on g_t) gives g_y, g_gamma and g_beta, and conv 1's gradients come from g_y with the raw weights -- nothing to unfold."""
    fm = blk.feature_map
    ks = fm[0].weight.shape[2]
    mode = "reflect" if ks == 3 else "zeros"
    pT1, pT2, _ = block_packs_transposed(blk) if bn is None else block_packs_raw_transposed(blk)
    grads = [None] * 6
    first = any(need[1:5])                      # conv 1 or its BatchNorm
    ops.act_backward_(g, f, "elu")
    if need[5] or need[6]:
        grads[4], grads[5] = ops.conv2d_backward_weight(t, g, ks, mode, bias=bool(need[6]))
    gx = None
    if first or need[0]:
        g_t = ops.conv2d_backward_data(g, pT2, mode)
        if bn is not None:
            y, mean, var = bn
            conv1 = need[1] or need[2]
            g_y, grads[2], grads[3] = ops.bn_act_backward(g_t, t, y, mean, var, fm[1].weight, fm[1].eps, "elu",
                                                          need_data=bool(conv1 or need[0]), out=g_t)
            if conv1:
                grads[0], grads[1] = ops.conv2d_backward_weight(x, g_y, ks, mode, bias=bool(need[2]))
            if need[0]:
                gx = ops.conv2d_backward_data(g_y, pT1, mode)
            return gx, grads
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
        if need[0]:
            gx = ops.conv2d_backward_data(g_t, pT1, mode)
    return gx, grads


# ---- the walk's nodes: feature part, head, level input -----------------------------------------------------------------
def block_features(blk, x):
    """f = blk.feature_map(x) (conv 1 + BatchNorm on its running statistics, or the batch's when blk.batch_stats is set, + ELU
    + conv 2 + ELU), x in the reference's channel order; an autograd node when x or a feature parameter requires grad."""
    _check_eval(blk)
    params = _feature_params(blk)
    if _wants_grad(x, *params):
        return _FeatureFunction.apply(blk, x, *params)
    return _feature_forward(blk, x)[1]


class _FeatureFunction(torch.autograd.Function):
    """The block without its head.  Inputs: (blk, x, w1, b1, gamma, beta, w2, b2); keeps t (post-ELU conv 1) and f."""

    @staticmethod
    def forward(ctx, blk, x, *params):
        t, f, ctx.bn = _feature_forward(blk, x)
        ctx.blk, ctx.t = blk, t
        ctx.save_for_backward(x, f, *params)
        return f

    @staticmethod
    def backward(ctx, g_f):
        x, f = ctx.saved_tensors[:2]
        need = ctx.needs_input_grad             # (blk, x, w1, b1, gamma, beta, w2, b2)
        gx, grads = _features_backward(ctx.blk, x, ctx.t, f, g_f.contiguous().clone(), need[1:8], ctx.bn)
        ctx.t = ctx.bn = None
        return (None, gx, *[gp if need[2 + j] else None for j, gp in enumerate(grads)])


HEAD_ONE_PASS = True        # the head's backward: vfi_phasenet_predict_backward, or the five-launch composition (section 16)
HEAD_ONE_PASS_THREE = True  # ... and whether the twelve-output head of three input images follows it (section 20's measurement)


def head_backward_composed(f, c, amp_in, max_amp, weight, g_phase, g_amp, g_c, need_feat=True, need_weight=True, need_bias=True,
                           num_img=2):
    """The head's adjoint from the entry points of section 14: emit backward, (+ g_c), tanh backward, 1x1 weight gradient,
    1x1 data gradient.  Same contract as ops.phasenet_predict_backward (ops.phasenet_predict_n_backward for num_img = 3, 4:
    amp_in whole, the emit adjoint of section 20)."""
    if g_phase is None and g_amp is None:
        g = None
    elif num_img == 2:
        g = ops.phasenet_emit_backward(g_phase, g_amp, amp_in, max_amp)
    else:
        g = ops.phasenet_emit_n_backward(g_phase, g_amp, c, amp_in, max_amp, num_img)
    if g is None:
        g = g_c if g_c is not None else torch.zeros_like(c)
    elif g_c is not None:
        g = ops.add(g, g_c)
    gz = ops.act_backward_(g, c, "tanh", out=torch.empty_like(c))
    gw = gb = gf = None
    if need_weight or need_bias:
        gw, gb = ops.conv2d_backward_weight(f, gz, 1, "zeros", bias=bool(need_bias))
    if need_feat:
        gf = ops.conv2d_backward_data(gz, ops.packed_transposed(weight), "zeros")
    return gf, (gw if need_weight else None), gb


def level_head(blk, f, amp_in, max_amp, num_img=2):
    """(c, phase_out, amp_out) of one band level from its features (phase_net.py:149-168 + reverse_normalize :80-90):
    c = blk.prediction_map(f) (N,8,H,W), the de-normalised outputs (N*4,1,H,W).  One vfi_phasenet_predict call, as in
    inference; an autograd node with a one-pass backward when f or the head's parameters require grad.  num_img = 3, 4 (the
    fusion networks, section 20): amp_in whole (N,4*num_img,H,W), c (N,12,H,W) for three images, vfi_phasenet_predict_n and its
    adjoint."""
    _check_eval(blk)
    pm = blk.prediction_map[0]
    if _wants_grad(f, pm.weight, pm.bias):
        return _HeadFunction.apply(blk, f, amp_in.detach(), max_amp.detach(), pm.weight, pm.bias, num_img)
    return _head_launch(blk, f, amp_in, max_amp, num_img)


def _head_launch(blk, f, amp_in, max_amp, num_img):
    if num_img == 2:
        return ops.phasenet_predict(f, _forward_packs(blk)[2], amp_in, max_amp)
    return ops.phasenet_predict_n(f, _forward_packs(blk)[2], amp_in, max_amp, num_img)


class _HeadFunction(torch.autograd.Function):
    """Inputs: (blk, f, amp_in, max_amp, wp, bp, num_img) -> (c, phase, amp).  c also feeds the next finer level, whose
    resize adjoint arrives here as g_c."""

    @staticmethod
    def forward(ctx, blk, f, amp_in, max_amp, wp, bp, num_img=2):
        c, phase, amp = _head_launch(blk, f, amp_in, max_amp, num_img)
        ctx.num_img = num_img
        ctx.save_for_backward(f, c, amp_in, max_amp, wp)
        ctx.set_materialize_grads(False)
        return c, phase, amp

    @staticmethod
    def backward(ctx, g_c, g_phase, g_amp):
        need = ctx.needs_input_grad             # (blk, f, amp_in, max_amp, wp, bp, num_img)
        if (g_c is None and g_phase is None and g_amp is None) or not (need[1] or need[4] or need[5]):
            return (None,) * 7
        f, c, amp_in, max_amp, wp = ctx.saved_tensors
        cont = lambda g: g.contiguous() if g is not None else None
        num_img = ctx.num_img
        if not (HEAD_ONE_PASS and (HEAD_ONE_PASS_THREE or num_img != 3)):
            gf, gw, gb = head_backward_composed(f, c, amp_in, max_amp, wp, cont(g_phase), cont(g_amp), cont(g_c),
                                                need_feat=need[1], need_weight=need[4], need_bias=need[5], num_img=num_img)
        elif num_img == 2:
            gf, gw, gb = ops.phasenet_predict_backward(f, c, amp_in, max_amp, wp, cont(g_phase), cont(g_amp), cont(g_c),
                                                       need_feat=need[1], need_weight=need[4], need_bias=need[5])
        else:
            gf, gw, gb = ops.phasenet_predict_n_backward(f, c, amp_in, max_amp, wp, num_img, cont(g_phase), cont(g_amp), cont(g_c),
                                                         need_feat=need[1], need_weight=need[4], need_bias=need[5])
        return None, gf, None, None, gw, gb, None


def level_input(f, c, phase, amp):
    """A band level's block input in the reference's channel order (phase_net.py:138-141):
    cat(resize(f), phase, amp, resize(c)) at phase's size, written into one buffer -- no separate concatenation.
    Differentiable in f and c; phase and amp (the normalised analysis outputs) get no gradient."""
    if _wants_grad(f, c):
        return _LevelInput.apply(f, c, phase.detach(), amp.detach())
    return _level_input(f, c, phase, amp)


def _level_input(f, c, phase, amp):
    n, cf, _, _ = f.shape
    cc, cp, ca = c.shape[1], phase.shape[1], amp.shape[1]
    h, w = phase.shape[2:]
    x = ops.new((n, cf + cp + ca + cc, h, w), f)
    ops.resize_bilinear(f, (h, w), align_corners=False, out=x[:, :cf])
    ops.affine_slice(phase.contiguous(), x[:, cf:cf + cp])
    ops.affine_slice(amp.contiguous(), x[:, cf + cp:cf + cp + ca])
    ops.resize_bilinear(c, (h, w), align_corners=False, out=x[:, cf + cp + ca:])
    return x


class _LevelInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, c, phase, amp):
        ctx.src = tuple(f.shape[2:])
        ctx.split = (f.shape[1], f.shape[1] + phase.shape[1] + amp.shape[1])
        return _level_input(f, c, phase, amp)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        cf, c0 = ctx.split
        gf = ops.resize_bilinear_adjoint(g[:, :cf], ctx.src) if ctx.needs_input_grad[0] else None
        gc = ops.resize_bilinear_adjoint(g[:, c0:], ctx.src) if ctx.needs_input_grad[1] else None
        return gf, gc, None, None


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
    def forward(ctx, pred, amp_in, max_amp, num_img=2):
        ctx.num_img = num_img
        ctx.save_for_backward(pred, amp_in, max_amp)
        ctx.set_materialize_grads(False)
        if num_img == 2:
            return ops.phasenet_emit(pred, amp_in, max_amp)
        return ops.phasenet_emit_n(pred, amp_in, max_amp, num_img)

    @staticmethod
    def backward(ctx, g_phase, g_amp):
        if g_phase is None and g_amp is None:
            return None, None, None, None
        pred, amp_in, max_amp = ctx.saved_tensors
        c = lambda g: g.contiguous() if g is not None else None
        if ctx.num_img == 2:
            return ops.phasenet_emit_backward(c(g_phase), c(g_amp), amp_in, max_amp), None, None, None
        return ops.phasenet_emit_n_backward(c(g_phase), c(g_amp), pred, amp_in, max_amp, ctx.num_img), None, None, None


def blend_level(pred, amp_in, max_amp, num_img=2):
    """One band level's de-normalised outputs from its prediction map (phase_net.py:155-168 + reverse_normalize :80-90):
    pred (N,8,H,W), amp_in (N,8,H,W) the normalised input amplitudes, max_amp (N,) -> (phase, amp), each (N*4,1,H,W).
    num_img = 3, 4: amp_in whole (N,4*num_img,H,W), pred (N,12,H,W) for three images (vfi_phasenet_emit_n and its adjoint).
    Differentiable in pred; amp_in and max_amp get no gradient."""
    if _wants_grad(pred):
        return _BlendLevel.apply(pred, amp_in.detach(), max_amp.detach(), num_img)
    return ops.phasenet_emit(pred, amp_in, max_amp) if num_img == 2 else ops.phasenet_emit_n(pred, amp_in, max_amp, num_img)


class _BlendLow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, low_in, max_low, num_img=2):
        ctx.num_img = num_img
        ctx.save_for_backward(pred, low_in, max_low)
        if num_img == 2:
            return ops.phasenet_emit_low(pred, low_in, max_low)
        return ops.phasenet_emit_low_n(pred, low_in, max_low, num_img)

    @staticmethod
    def backward(ctx, g_low):
        pred, low_in, max_low = ctx.saved_tensors
        if ctx.num_img == 2:
            return ops.phasenet_emit_low_backward(g_low.contiguous(), low_in, max_low), None, None, None
        return ops.phasenet_emit_low_n_backward(g_low.contiguous(), pred, low_in, max_low, ctx.num_img), None, None, None


def blend_low(pred, low_in, max_low, num_img=2):
    """The low level's de-normalised output (phase_net.py:113-116 + :96-98): pred (N,1,H,W), low_in (N,2,H,W) normalised,
    max_low (N,) -> (N,1,H,W).  num_img = 3, 4: low_in (N,num_img,H,W), pred (N,2,H,W) for three images.  Differentiable in
    pred."""
    if _wants_grad(pred):
        return _BlendLow.apply(pred, low_in.detach(), max_low.detach(), num_img)
    return ops.phasenet_emit_low(pred, low_in, max_low) if num_img == 2 else ops.phasenet_emit_low_n(pred, low_in, max_low, num_img)
