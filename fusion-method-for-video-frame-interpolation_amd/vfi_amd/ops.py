"""Host-side wrappers of the generic device ops of libvfi_hip.so (include/vfi_hip.h).

Tensors are torch HIP tensors used purely as device-memory handles; every wrapper enqueues one
library call on torch's current stream.  Inputs / outputs may be CHANNEL SLICES of wider NCHW
tensors (`t[:, a:b]`): only the batch stride is free, the (C, H, W) block must be dense.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import VfiLibraryError

ACT = {None: 0, "none": 0, "relu": 1, "elu": 2, "tanh": 3, "sigmoid": 4}
PAD = {"zeros": 0, "zero": 0, "reflect": 1}


def _slice_ptr(t, name):
    """(device address, batch stride) of an NCHW tensor whose per-sample (C,H,W) block is dense."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise VfiLibraryError(f"{name} must be a tensor on a HIP device (vfi_amd has no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 4:
        raise VfiLibraryError(f"{name} must be a 4-d float32 tensor")
    _lib.check_device(t, name)
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    if not ((sw == 1 or w == 1) and (sh == w or h == 1) and (sc == h * w or c == 1)):
        raise VfiLibraryError(f"{name}: per-sample (C,H,W) block must be dense, strides {t.stride()}")
    if n == 1:
        sn = c * h * w
    return t.data_ptr(), sn


def new(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


class PackedConv:
    """Weights of one nn.Conv2d in the matrix-core layout ([Cin_pad][KS*KS][Cout_pad]) plus bias.

    `bn` = (weight, bias, running_mean, running_var, eps) folds an eval-mode BatchNorm2d that
    follows the conv (reference src/phase_net/phase_net.py:191-193) into weights and bias."""

    def __init__(self, weight, bias=None, bn=None, device=None):
        device = torch.device(device) if device is not None else weight.device
        if device.type != "cuda":
            raise VfiLibraryError("PackedConv needs a HIP device (vfi_amd has no CPU path)")
        weight = weight.detach().to(device=device, dtype=torch.float32).contiguous()
        self.cout, self.cin, kh, kw = weight.shape
        assert kh == kw, "square kernels only"
        self.ks = kh
        cout = self.cout
        b = (bias.detach().to(device=device, dtype=torch.float32) if bias is not None
             else torch.zeros(cout, device=device))
        scale = None
        if bn is not None:  # y = (conv + b - mean) * g / sqrt(var + eps) + beta
            g, beta, mean, var, eps = bn
            f = lambda t: t.detach().to(device=device, dtype=torch.float32)
            scale = (f(g) / torch.sqrt(f(var) + eps)).contiguous()
            b = (b - f(mean)) * scale + f(beta)
        self.bias = b.contiguous()
        n = _lib.lib().vfi_conv2d_packed_floats(cout, self.cin, self.ks)
        if n <= 0:
            raise VfiLibraryError(f"vfi_conv2d_packed_floats rejected {tuple(weight.shape)}")
        self.packed = torch.empty(n, dtype=torch.float32, device=device)
        _lib.call("vfi_conv2d_pack", weight.data_ptr(), scale.data_ptr() if scale is not None else None,
                  self.packed.data_ptr(), cout, self.cin, self.ks, _lib.stream_ptr())
        self._keep = (weight, scale)  # alive until the pack kernel has run (same stream ordering)


WINOGRAD = os.environ.get("VFI_CONV_WINOGRAD", "1") != "0"     # mirrors the library's switch (profiling labels only)
# 3x3 convs whose input is a bilinear resize: materialise the resize and use the Winograd kernel (default), or keep the
# direct kernels with the interpolating tile loader (VFI_CONV_FUSED_RESIZE=1; always when Winograd is off)
FUSED_RESIZE = (not WINOGRAD) or os.environ.get("VFI_CONV_FUSED_RESIZE", "0") == "1"
# (measured again in round 2 for the thin 25 -> 25 head convolutions alone: the fused loader loses there too,
# 77.5 vs 72.2 ms per frame)
def _winograd_work(n, cin, cout, h, w, residual=False, pooled=False, act="relu"):
    """Profiling label and the executed algorithm's own flop count of a 3x3 layer.  Which kernel runs is the library's
    decision (vfi_conv2d_algo): F(4x4,3x3) -- 36 multiply-adds per 4x4 outputs and channel pair -- or F(2x2,3x3) -- 16 per
    2x2 outputs."""
    algo = _lib.lib().vfi_conv2d_algo(n, cin, h, w, cout, 3, int(bool(residual)), int(bool(pooled)), ACT[act])
    if algo == 2:       # (the M = 32 kernel unless VFI_CONV_WINOGRAD4M=0: the library reads that switch at every call)
        name = "conv3x3_winograd4_kernel" if os.environ.get("VFI_CONV_WINOGRAD4M", "1") == "0" else "conv3x3_winograd4m_kernel"
        return ("flop", 2.0 * n * cin * cout * 36 * (h * w / 16.0), name)
    if algo == 1:
        return ("flop", 2.0 * n * cin * cout * 16 * (h * w / 4.0), "conv3x3_winograd_kernel")
    return ("flop", 2.0 * n * cin * cout * 9 * h * w, "conv2d_mfma_kernel<3,8,%d>" % (2 if ((cout + 31) // 32 * 32) % 64 == 0 else 1))


_WORKSPACES = {}
WORKSPACE_FLOATS = 48 * 1024 * 1024     # 192 MiB per (device, stream): split-K partial sums of the deep U-Net levels


def _workspace(device):
    """Split-K scratch, one per (device, stream) so frames in flight on different streams never share it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = torch.empty(WORKSPACE_FLOATS, dtype=torch.float32, device=device)
    return ws


def conv2d(x, pc, pad_mode="zeros", act=None, residual=None, out=None, upsample2x=False):
    """act(conv(x) + bias) (+ residual) -> out.  One vfi_conv2d launch.  upsample2x: x is the low-resolution
    input of an `Upsample(x2, bilinear, align_corners=True) -> conv` pair (the upsampled tensor is not
    materialised)."""
    n, cin, h, w = x.shape
    if cin != pc.cin:
        raise VfiLibraryError(f"conv2d: input has {cin} channels, weights expect {pc.cin}")
    if upsample2x and pc.ks == 3 and not FUSED_RESIZE:
        # the Winograd kernel reads its input by LDS-DMA and cannot interpolate on the fly: one streaming resize pass
        # (HBM-bound, a few % of the conv) + the Winograd conv beats the direct kernel with the fused loader
        x = resize_bilinear(x, (2 * h, 2 * w), align_corners=True)
        h, w, upsample2x = 2 * h, 2 * w, False
    if upsample2x:
        h, w = 2 * h, 2 * w
    if out is None:
        out = new((n, pc.cout, h, w), x)
    elif tuple(out.shape) != (n, pc.cout, h, w):
        raise VfiLibraryError(f"conv2d: out shape {tuple(out.shape)} != {(n, pc.cout, h, w)}")
    xp, xs = _slice_ptr(x, "x")
    yp, ys = _slice_ptr(out, "out")
    rp, rs = (None, 0)
    if residual is not None:
        if tuple(residual.shape) != tuple(out.shape):
            raise VfiLibraryError("conv2d: residual shape mismatch")
        rp, rs = _slice_ptr(residual, "residual")
    ws = _workspace(x.device)
    work = None
    if _lib.PROFILE is not None:
        if pc.ks == 3 and not upsample2x and WINOGRAD:
            work = _winograd_work(n, cin, pc.cout, h, w, residual is not None, False, act)
        else:
            label = (f"conv2d_mfma_kernel<{pc.ks},{4 if pc.ks == 5 else 8},{2 if ((pc.cout + 31) // 32 * 32) % 64 == 0 else 1}"
                     + (",ups>" if upsample2x else ">"))
            work = ("flop", 2.0 * n * cin * pc.cout * pc.ks * pc.ks * h * w, label)
            if pc.ks == 1:
                # a 1x1 layer (PhaseNet's 64 -> 8 prediction maps, the coarse 1x1 blocks, FusionNet's 32 -> 3 tail) does
                # 2*Cout flop per input byte: it is bound by reading the input once, not by the matrix cores
                if _lib.lib().vfi_conv2d_algo(n, cin, h, w, pc.cout, 1, int(residual is not None), 0, ACT[act]) == 3:
                    label = "conv1x1_stream_kernel"
                work = ("byte", 4.0 * n * (cin + pc.cout) * h * w, label)
    _lib.call("vfi_conv2d_upsample2x" if upsample2x else "vfi_conv2d", xp, xs, pc.packed.data_ptr(), pc.bias.data_ptr(), rp, rs, yp, ys,
              n, cin, h, w, pc.cout, pc.ks, PAD[pad_mode], ACT[act], ws.data_ptr(), ws.numel(), _lib.stream_ptr(), work=work)
    return out


def conv2d_pool2(x, pc, is_max, pad_mode="zeros", act="relu"):
    """(act(conv(x) + bias), pool2 of it): one vfi_conv2d_pool2 call (the pooled tensor comes out of the conv's epilogue
    for 3x3 ReLU layers)."""
    n, cin, h, w = x.shape
    if cin != pc.cin:
        raise VfiLibraryError(f"conv2d_pool2: input has {cin} channels, weights expect {pc.cin}")
    out, pooled = new((n, pc.cout, h, w), x), new((n, pc.cout, h // 2, w // 2), x)
    xp, xs = _slice_ptr(x, "x")
    ws = _workspace(x.device)
    work = None
    if _lib.PROFILE is not None:
        if pc.ks == 3 and WINOGRAD:
            work = _winograd_work(n, cin, pc.cout, h, w, False, True, act)
        else:
            work = ("flop", 2.0 * n * cin * pc.cout * pc.ks * pc.ks * h * w,
                    f"conv2d_mfma_kernel<{pc.ks},{4 if pc.ks == 5 else 8},{2 if ((pc.cout + 31) // 32 * 32) % 64 == 0 else 1}>")
    _lib.call("vfi_conv2d_pool2", xp, xs, pc.packed.data_ptr(), pc.bias.data_ptr(), out.data_ptr(), out.stride(0),
              pooled.data_ptr(), pooled.stride(0), int(bool(is_max)), n, cin, h, w, pc.cout, pc.ks, PAD[pad_mode], ACT[act],
              ws.data_ptr(), ws.numel(), _lib.stream_ptr(), work=work)
    return out, pooled


def conv2d_resized_prefix(x, x2, pc, pad_mode="reflect", act=None, out=None):
    """conv over [bilinear_resize(x2, align_corners=False) | x[:, C2:]] with C2 = x2.shape[1]; x is (N, Cin, H, W) whose
    first C2 channels are ignored (never written).  One launch, the resized maps are not materialised."""
    n, cin, h, w = x.shape
    n2, c2, hs, ws_ = x2.shape
    if cin != pc.cin or n2 != n:
        raise VfiLibraryError("conv2d_resized_prefix: shape mismatch")
    if pc.ks == 3 and not FUSED_RESIZE:      # see conv2d(upsample2x=True)
        resize_bilinear(x2, (h, w), align_corners=False, out=x[:, :c2])
        return conv2d(x, pc, pad_mode=pad_mode, act=act, out=out)
    if out is None:
        out = new((n, pc.cout, h, w), x)
    xp, xs = _slice_ptr(x, "x")
    x2p, x2s = _slice_ptr(x2, "x2")
    yp, ys = _slice_ptr(out, "out")
    ws = _workspace(x.device)
    work = None
    if _lib.PROFILE is not None:
        work = ("flop", 2.0 * n * cin * pc.cout * pc.ks * pc.ks * h * w, f"conv2d_mfma_kernel<{pc.ks},8,2,rsz>")
    _lib.call("vfi_conv2d_resized_prefix", xp, xs, x2p, x2s, c2, hs, ws_, pc.packed.data_ptr(), pc.bias.data_ptr(), yp, ys,
              n, cin, h, w, pc.cout, pc.ks, PAD[pad_mode], ACT[act], ws.data_ptr(), ws.numel(), _lib.stream_ptr(), work=work)
    return out


def adacof_prepare(frame0, frame2, rgbx=True):
    """-> (pad0, pad2, x6 (N,6,Hp,Wp)); Hp, Wp = sizes rounded up to multiples of 32.  pad0/pad2 are the
    reflect-padded raw frames: pixel-interleaved (N,Hp,Wp,4) when rgbx, else planar (N,3,Hp,Wp)."""
    n, c, h, w = frame0.shape
    if c != 3 or tuple(frame2.shape) != tuple(frame0.shape):
        raise VfiLibraryError("adacof_prepare: frames must both be (N,3,H,W)")
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    shape = (n, hp, wp, 4) if rgbx else (n, 3, hp, wp)
    pad0, pad2, x6 = new(shape, frame0), new(shape, frame0), new((n, 6, hp, wp), frame0)
    _lib.call("vfi_adacof_prepare", _lib.dptr(frame0, "frame0"), _lib.dptr(frame2, "frame2"), pad0.data_ptr(),
              pad2.data_ptr(), x6.data_ptr(), n, h, w, hp, wp, int(bool(rgbx)), _lib.stream_ptr())
    return pad0, pad2, x6


def pool2(x, is_max, out=None):
    n, c, h, w = x.shape
    if out is None:
        out = new((n, c, h // 2, w // 2), x)
    xp, xs = _slice_ptr(x, "x")
    yp, ys = _slice_ptr(out, "out")
    _lib.call("vfi_pool2", xp, xs, yp, ys, n, c, h, w, int(bool(is_max)), _lib.stream_ptr())
    return out


def resize_bilinear(x, size, align_corners, relu_input=False, residual=None, out=None):
    n, c, h, w = x.shape
    ho, wo = size
    if out is None:
        out = new((n, c, ho, wo), x)
    xp, xs = _slice_ptr(x, "x")
    yp, ys = _slice_ptr(out, "out")
    rp, rs = (None, 0) if residual is None else _slice_ptr(residual, "residual")
    _lib.call("vfi_resize_bilinear", xp, xs, rp, rs, yp, ys, n, c, h, w, ho, wo, int(bool(align_corners)),
              int(bool(relu_input)), _lib.stream_ptr())
    return out


# PhaseNet.forward takes vfi_phasenet_level_tail from this many pixels per plane on.  A tile of the one-pass kernel walks its 64
# channels in 18 dependent stages, about 45 us however small the level; the two launches it replaces need that long at
# 135 x 240 and are quicker below (profiles/r06_phasenet_tail.txt).
PHASENET_TAIL_MIN_PIXELS = 40000


def phasenet_level_tail(fp, cp, amp_in, max_amp, x_next):
    """A two-image band level's head and the next level's resize in one vfi_phasenet_level_tail call: fp[:, :64] the block's
    features, cp the packed 64 -> 8 prediction map, amp_in the level's 8 normalised amplitude planes, x_next the first 72
    channels of the next level's block input (a channel slice), which receive bilinear_resize([feature | prediction],
    align_corners=False).  -> (phase_out, amp_out), each (4 N, 1, h, w)."""
    n, _, h, w = fp.shape
    if cp.cin != 64 or cp.cout != 8 or cp.ks != 1 or fp.shape[1] < 64 or x_next.shape[:2] != (n, 72) or amp_in.shape != (n, 8, h, w):
        raise VfiLibraryError("phasenet_level_tail: shape mismatch")
    ho, wo = x_next.shape[2:]
    fpp, fps = _slice_ptr(fp[:, :64], "fp")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    xp, xs = _slice_ptr(x_next, "x_next")
    p_out, a_out = new((n * 4, 1, h, w), fp), new((n * 4, 1, h, w), fp)
    work = ("byte", 4.0 * n * ((64 + 8 + 8) * h * w + 72 * ho * wo), "phasenet_level_tail_kernel") if _lib.PROFILE is not None else None
    _lib.call("vfi_phasenet_level_tail", fpp, fps, cp.packed.data_ptr(), cp.bias.data_ptr(), ap, as_, _lib.dptr(max_amp, "max_amp"), xp, xs,
              p_out.data_ptr(), a_out.data_ptr(), n, h, w, ho, wo, _lib.stream_ptr(), work=work)
    return p_out, a_out


def softmax_channels_(x):
    n, c, h, w = x.shape
    xp, xs = _slice_ptr(x, "x")
    _lib.call("vfi_softmax_channels", xp, xs, xp, xs, n, c, h * w, _lib.stream_ptr())
    return x


def affine_slice(src, dst, div=None, mul=1.0):
    """dst[n] = src[n] / div[n] * mul over the per-sample (C,H,W) block (dst may be a channel slice)."""
    n = src.shape[0]
    count = src[0].numel()
    if dst.shape[0] != n or dst[0].numel() != count:
        raise VfiLibraryError("affine_slice: shape mismatch")
    sp, ss = _slice_ptr(src, "src")
    dp, ds = _slice_ptr(dst, "dst")
    _lib.call("vfi_affine_slice", sp, ss, dp, ds, n, count, _lib.dptr(div, "div") if div is not None else None,
              float(mul), _lib.stream_ptr())
    return dst


def batch_max(x, eps):
    """max over each sample's (C,H,W) block, + eps -> (N,) tensor."""
    n = x.shape[0]
    xp, xs = _slice_ptr(x, "x")
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = torch.empty(n, dtype=torch.int32, device=x.device)
    _lib.call("vfi_batch_max", xp, xs, n, x[0].numel(), float(eps), out.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    return out


def tanh_residual_clamp(x, base):
    out = torch.empty_like(x)
    _lib.call("vfi_tanh_residual_clamp", _lib.dptr(x, "x"), _lib.dptr(base, "base"), out.data_ptr(), x.numel(),
              _lib.stream_ptr())
    return out


def packed_transposed(weight):
    """PackedConv of W.transpose(0,1).flip(2,3) (no bias): the weights vfi_conv2d_backward_data convolves dY with."""
    return PackedConv(weight.detach().transpose(0, 1).flip(2, 3))


def conv2d_backward_weight(x, dy, ks, pad_mode="zeros", bias=True, max_splits=None):
    """(dW (Cout, Cin, KS, KS), dbias (Cout) or None) of a stride-1 conv2d layer with input x and output gradient dy.
    One vfi_conv2d_backward_weight call (split-K partial slabs in the per-stream workspace, fixed-order reduction).
    `max_splits` caps the split count (by the workspace size handed on): two calls over the same pixels with the same
    split count sum in the same order, whatever their Cout -- see conv2d_backward_weight_splits."""
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    if tuple(dy.shape) != (n, cout, h, w):
        raise VfiLibraryError(f"conv2d_backward_weight: dy {tuple(dy.shape)} does not match x {tuple(x.shape)}")
    dw = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=x.device)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if bias else None
    xp, xs = _slice_ptr(x, "x")
    gp, gs = _slice_ptr(dy, "dy")
    ws = _workspace(x.device)
    work = ("flop", 2.0 * n * cin * cout * ks * ks * h * w, f"conv_wgrad_kernel<{ks}>") if _lib.PROFILE is not None else None
    ws_floats = ws.numel()
    if max_splits is not None:
        ws_floats = min(ws_floats, max(int(max_splits), 1) * cout * (cin * ks * ks + 1))
    _lib.call("vfi_conv2d_backward_weight", xp, xs, gp, gs, dw.data_ptr(), db.data_ptr() if bias else None, n, cin, h, w,
              cout, ks, PAD[pad_mode], ws.data_ptr(), ws_floats, _lib.stream_ptr(), work=work)
    return dw, db


def conv2d_backward_weight_splits(n, cin, h, w, cout, ks):
    """Split count vfi_conv2d_backward_weight uses for this layer with the default workspace (the library's rule)."""
    return int(_lib.lib().vfi_conv2d_backward_weight_splits(n, cin, h, w, cout, ks, WORKSPACE_FLOATS))


BWD_DATA_SPLITK_FLOATS = 8 * 1024 * 1024     # handed on to vfi_conv2d's split-K beyond the embed / fold buffers


def conv2d_backward_data(dy, pct, pad_mode="zeros", out=None):
    """dX (N, Cin, H, W) of a stride-1 conv2d layer from its output gradient dy; `pct` = packed_transposed(weight).
    One vfi_conv2d_backward_data call; reflect padding takes a workspace of the padded extent, allocated here."""
    n, cout, h, w = dy.shape
    cin, ks = pct.cout, pct.ks
    if pct.cin != cout:
        raise VfiLibraryError(f"conv2d_backward_data: dy has {cout} channels, weights expect {pct.cin}")
    if out is None:
        out = new((n, cin, h, w), dy)
    elif tuple(out.shape) != (n, cin, h, w):
        raise VfiLibraryError(f"conv2d_backward_data: out shape {tuple(out.shape)} != {(n, cin, h, w)}")
    gp, gs = _slice_ptr(dy, "dy")          # (before the workspace: a CPU tensor has no stream to key one on)
    op, os_ = _slice_ptr(out, "out")
    need = _lib.lib().vfi_conv2d_backward_data_workspace_floats(n, cin, h, w, cout, ks, PAD[pad_mode])
    if need < 0:
        raise VfiLibraryError(f"conv2d_backward_data: unsupported layer {cout}->{cin} KS={ks}")
    ws = _workspace(dy.device) if need == 0 else torch.empty(need + BWD_DATA_SPLITK_FLOATS, dtype=torch.float32,
                                                             device=dy.device)
    work = None
    if _lib.PROFILE is not None:
        p = (ks - 1) // 2 if pad_mode == "reflect" else 0
        work = ("flop", 2.0 * n * cin * cout * ks * ks * (h + 2 * p) * (w + 2 * p), f"conv_dgrad<{ks}>")
    _lib.call("vfi_conv2d_backward_data", gp, gs, pct.packed.data_ptr(), op, os_, n, cin, h, w, cout, ks, PAD[pad_mode],
              ws.data_ptr(), ws.numel(), _lib.stream_ptr(), work=work)
    return out


def tanh_residual_clamp_backward(x, base, grad, need_x=True, need_base=True):
    """(grad_x, grad_base) of tanh_residual_clamp; an output not needed is None (not written)."""
    gx = torch.empty_like(x) if need_x else None
    gb = torch.empty_like(x) if need_base else None
    _lib.call("vfi_tanh_residual_clamp_backward", _lib.dptr(x, "x"), _lib.dptr(base, "base"), _lib.dptr(grad, "grad"),
              gx.data_ptr() if need_x else None, gb.data_ptr() if need_base else None, x.numel(), _lib.stream_ptr(),
              work=("byte", 20.0 * x.numel(), "tanh_residual_clamp_backward") if _lib.PROFILE is not None else None)
    return gx, gb


def pool2_max_backward(y, grad_pooled, grad_skip=None, out=None):
    """Gradient of y = relu(z) feeding MaxPool2d(2) and a skip: (max-pool routing of grad_pooled + grad_skip) * [y > 0]."""
    n, c, h, w = y.shape
    if out is None:
        out = new((n, c, h, w), y)
    yp, ys = _slice_ptr(y, "y")
    pp, ps = _slice_ptr(grad_pooled, "grad_pooled")
    kp, ks = (None, 0) if grad_skip is None else _slice_ptr(grad_skip, "grad_skip")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_pool2_max_backward", yp, ys, pp, ps, kp, ks, op, os_, n, c, h, w, _lib.stream_ptr(),
              work=("byte", 4.0 * n * c * h * w * (2.25 + (grad_skip is not None)), "pool2_max_backward")
              if _lib.PROFILE is not None else None)
    return out


def resize_bilinear_backward(x, grad, relu_input=True, out=None):
    """Gradient of x through resize_bilinear(x, 2x size, align_corners=False, relu_input) (gather form)."""
    n, c, h, w = x.shape
    if out is None:
        out = new((n, c, h, w), x)
    xp, xs = _slice_ptr(x, "x")
    gp, gs = _slice_ptr(grad, "grad")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_resize_bilinear_backward", xp, xs, gp, gs, op, os_, n, c, h, w, grad.shape[2], grad.shape[3],
              int(bool(relu_input)), _lib.stream_ptr(),
              work=("byte", 4.0 * n * c * h * w * 6, "resize_bilinear_backward") if _lib.PROFILE is not None else None)
    return out


# ---- glue of the AdaCoF network's backward ---------------------------------------------------
def _prof(kind, amount, label):
    return (kind, amount, label) if _lib.PROFILE is not None else None


def add(a, b):
    """a + b as a new dense tensor (operands may be channel slices)."""
    n = a.shape[0]
    count = a[0].numel()
    if tuple(a.shape) != tuple(b.shape):
        raise VfiLibraryError("add: shape mismatch")
    out = new(tuple(a.shape), a)
    ap, as_ = _slice_ptr(a, "a")
    bp, bs = _slice_ptr(b, "b")
    _lib.call("vfi_add", ap, as_, bp, bs, out.data_ptr(), count, n, count, _lib.stream_ptr(),
              work=_prof("byte", 12.0 * n * count, "add"))
    return out


def relu_mask_(grad, y, addend=None, out=None):
    """(grad + addend) * [y > 0], in place unless `out` is given; y is the ReLU's output."""
    n = grad.shape[0]
    count = grad[0].numel()
    if tuple(y.shape) != tuple(grad.shape) or (addend is not None and tuple(addend.shape) != tuple(grad.shape)):
        raise VfiLibraryError("relu_mask_: shape mismatch")
    gp, gs = _slice_ptr(grad, "grad")
    yp, ys = _slice_ptr(y, "y")
    ap, as_ = (None, 0) if addend is None else _slice_ptr(addend, "addend")
    op, os_ = (gp, gs) if out is None else _slice_ptr(out, "out")
    if out is not None and tuple(out.shape) != tuple(grad.shape):
        raise VfiLibraryError("relu_mask_: out shape mismatch")
    _lib.call("vfi_relu_mask", gp, gs, ap, as_, yp, ys, op, os_, n, count, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * count * (3 + (addend is not None)), "relu_mask"))
    return grad if out is None else out


def sigmoid_backward(grad, s):
    """grad * s * (1 - s) for s = sigmoid(z)."""
    gz = torch.empty_like(s)
    _lib.call("vfi_sigmoid_backward", _lib.dptr(grad, "grad"), _lib.dptr(s, "s"), gz.data_ptr(), s.numel(), _lib.stream_ptr(),
              work=_prof("byte", 12.0 * s.numel(), "sigmoid_backward"))
    return gz


def replicate_pad(x, pad):
    """ReplicationPad2d(pad) of an NCHW tensor (dense result)."""
    n, c, h, w = x.shape
    out = new((n, c, h + 2 * pad, w + 2 * pad), x)
    xp, xs = _slice_ptr(x, "x")
    _lib.call("vfi_replicate_pad", xp, xs, out.data_ptr(), n, c, h, w, int(pad), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * (x.numel() + out.numel()), "replicate_pad"))
    return out


def pool2_avg_backward(y, grad_pooled, grad_skip=None, out=None):
    """Gradient of y = relu(z) feeding AvgPool2d(2) and a skip: (grad_pooled / 4 over each window + grad_skip) * [y > 0]."""
    n, c, h, w = y.shape
    if tuple(grad_pooled.shape) != (n, c, h // 2, w // 2) or (grad_skip is not None and tuple(grad_skip.shape) != tuple(y.shape)):
        raise VfiLibraryError("pool2_avg_backward: shape mismatch")
    if out is None:
        out = new((n, c, h, w), y)
    yp, ys = _slice_ptr(y, "y")
    pp, ps = _slice_ptr(grad_pooled, "grad_pooled")
    kp, ks = (None, 0) if grad_skip is None else _slice_ptr(grad_skip, "grad_skip")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_pool2_avg_backward", yp, ys, pp, ps, kp, ks, op, os_, n, c, h, w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * h * w * (2.25 + (grad_skip is not None)), "pool2_avg_backward"))
    return out


def upsample2x_backward(grad, mask_src=None, out=None):
    """Adjoint of resize_bilinear(x, 2x size, align_corners=True); mask_src: the source when it is a ReLU's output."""
    n, c, ho, wo = grad.shape
    if ho % 2 or wo % 2:
        raise VfiLibraryError(f"upsample2x_backward: odd gradient size {ho}x{wo}")
    h, w = ho // 2, wo // 2
    if mask_src is not None and tuple(mask_src.shape) != (n, c, h, w):
        raise VfiLibraryError("upsample2x_backward: mask_src shape mismatch")
    if out is None:
        out = new((n, c, h, w), grad)
    gp, gs = _slice_ptr(grad, "grad")
    mp, ms = (None, 0) if mask_src is None else _slice_ptr(mask_src, "mask_src")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_upsample2x_backward", gp, gs, mp, ms, op, os_, n, c, h, w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * h * w * (5 + (mask_src is not None)), "upsample2x_backward"))
    return out


def _reduce_workspace(like):
    return torch.empty(_lib.REDUCE_WORKSPACE_FLOATS, dtype=torch.float32, device=like.device)


def adacof_smooth_forward(w1, a1, b1, w2, a2, b2, occ, epsilon=0.001):
    """-> (m (N,4,H,W) = [m_Alpha1, m_Beta1, m_Alpha2, m_Beta2], terms (2,) = [g_Spatial, g_Occlusion])."""
    n, ff, h, w = w1.shape
    f = int(round(ff ** 0.5))
    m = new((n, 4, h, w), w1)
    out = new((2,), w1)
    d = _lib.dptr
    _lib.call("vfi_adacof_smooth_forward", d(w1, "w1"), d(a1, "a1"), d(b1, "b1"), d(w2, "w2"), d(a2, "a2"), d(b2, "b2"),
              d(occ, "occ"), m.data_ptr(), _reduce_workspace(w1).data_ptr(), out.data_ptr(), n, f, h, w, float(epsilon),
              _lib.stream_ptr(), work=_prof("byte", 4.0 * n * h * w * (6 * ff + 4 + 2 * 5), "adacof_smooth_forward"))
    return m, out


def adacof_blend_backward(grad_frame, t1, t2, occ, up_occ=None, epsilon=0.001):
    """-> (grad_t1, grad_t2, grad_z) of frame1 = occ t1 + (1 - occ) t2 cropped to grad_frame's size, occ = sigmoid(z);
    up_occ: 0-dim device tensor, the upstream gradient of g_Occlusion."""
    n, c, h, w = t1.shape
    h0, w0 = grad_frame.shape[2:]
    g1, g2, gz = torch.empty_like(t1), torch.empty_like(t1), torch.empty_like(occ)
    d = _lib.dptr
    _lib.call("vfi_adacof_blend_backward", d(grad_frame, "grad_frame"), d(t1, "t1"), d(t2, "t2"), d(occ, "occ"),
              d(up_occ, "up_occ"), g1.data_ptr(), g2.data_ptr(), gz.data_ptr(), n, c, h, w, int(h0), int(w0), float(epsilon),
              _lib.stream_ptr(), work=_prof("byte", 4.0 * n * (c * (h0 * w0 + 4 * h * w) + 2 * h * w), "adacof_blend_backward"))
    return g1, g2, gz


def adacof_head_backward(gw, ga, gb, w, a, b, m_a=None, m_b=None, up_spatial=None, epsilon=0.001):
    """One side: (grad_logit, grad_alpha, grad_beta) from the sampler's gradients and g_Spatial's upstream gradient
    (0-dim device tensor, or None); m_a, m_b: that side's planes m[:, i:i+1] of adacof_smooth_forward."""
    n, ff, h, wd = w.shape
    f = int(round(ff ** 0.5))
    gl, gal, gbe = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    d = _lib.dptr
    map_, mbs = (None, 0) if m_a is None else _slice_ptr(m_a, "m_a")
    mbp, _ = (None, 0) if m_b is None else _slice_ptr(m_b, "m_b")
    _lib.call("vfi_adacof_head_backward", d(gw, "gw"), d(ga, "ga"), d(gb, "gb"), d(w, "w"), d(a, "a"), d(b, "b"), map_, mbp, mbs,
              d(up_spatial, "up_spatial"), gl.data_ptr(), gal.data_ptr(), gbe.data_ptr(), n, f, h, wd, float(epsilon),
              _lib.stream_ptr(), work=_prof("byte", 4.0 * n * h * wd * (9 * ff + 2), "adacof_head_backward"))
    return gl, gal, gbe


def charbonnier_forward(a, b=None, epsilon=0.001):
    """mean(sqrt((a - b)^2 + epsilon^2)) -> 0-dim tensor."""
    out = new((1,), a)
    _lib.call("vfi_charbonnier_forward", _lib.dptr(a, "a"), _lib.dptr(b, "b"), a.numel(), float(epsilon),
              _reduce_workspace(a).data_ptr(), out.data_ptr(), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * a.numel() * (1 + (b is not None)), "charbonnier_forward"))
    return out[0]


def charbonnier_backward(a, b, upstream, epsilon=0.001, need_a=True, need_b=False):
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(a) if need_b else None
    _lib.call("vfi_charbonnier_backward", _lib.dptr(a, "a"), _lib.dptr(b, "b"), _lib.dptr(upstream.reshape(1), "upstream"),
              _lib.dptr(ga), _lib.dptr(gb), a.numel(), float(epsilon), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * a.numel() * (1 + (b is not None) + need_a + need_b), "charbonnier_backward"))
    return ga, gb


def mse_forward(a, b):
    """mean((a - b)^2) -> 0-dim tensor (nn.MSELoss); a and b dense, of one element count, possibly parts of one tensor."""
    if a.numel() != b.numel():
        raise VfiLibraryError("mse_forward: shape mismatch")
    out = new((1,), a)
    _lib.call("vfi_mse_forward", _lib.dptr(a, "a"), _lib.dptr(b, "b"), a.numel(), _reduce_workspace(a).data_ptr(),
              out.data_ptr(), _lib.stream_ptr(), work=_prof("byte", 8.0 * a.numel(), "mse_forward"))
    return out[0]


def mse_backward(a, b, upstream, need_a=True, need_b=False):
    if a.numel() != b.numel():
        raise VfiLibraryError("mse_backward: shape mismatch")
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(b) if need_b else None
    _lib.call("vfi_mse_backward", _lib.dptr(a, "a"), _lib.dptr(b, "b"), _lib.dptr(upstream.reshape(1), "upstream"),
              _lib.dptr(ga), _lib.dptr(gb), a.numel(), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * a.numel() * (2 + need_a + need_b), "mse_backward"))
    return ga, gb


# ---- LPIPS -----------------------------------------------------------------------------------
def _map_ptr(t, name):
    """(address, batch stride, N, C, HW) of a feature map (N, C, H, W) or (N, C, HW) whose per-sample block is dense"""
    if isinstance(t, torch.Tensor) and t.dim() == 3:
        t = t.unsqueeze(-1)
    p, s = _slice_ptr(t, name)
    return p, s, t.shape[0], t.shape[1], t.shape[2] * t.shape[3]


def _vec(t, count, name):
    if t is not None and t.numel() != count:
        raise VfiLibraryError(f"{name} must hold {count} floats, got {tuple(t.shape)}")
    return _lib.dptr(t, name)


def lpips_head_forward(x, y, w, prior=None):
    """-> (N,) = prior + mean_p sum_c w_c (xh_c - yh_c)^2 of one tap, xh = x / (|x|_channels + 1e-10); x, y may be the two
    halves of one tensor."""
    xp, xs, n, c, hw = _map_ptr(x, "x")
    yp, ys = _map_ptr(y, "y")[:2]
    if tuple(x.shape) != tuple(y.shape):
        raise VfiLibraryError("lpips_head_forward: shape mismatch")
    out = new((n,), x)
    _lib.call("vfi_lpips_head_forward", xp, xs, yp, ys, _vec(w, c, "w"), _vec(prior, n, "prior"), out.data_ptr(),
              _reduce_workspace(x).data_ptr(), n, c, hw, _lib.stream_ptr(), work=_prof("byte", 8.0 * n * c * hw, "lpips_head_forward"))
    return out


def lpips_head_backward(x, y, w, upstream, above=None, relu_mask=True, out=None):
    """-> (above + upstream[n] * d head / dx) * [x > 0 when relu_mask], of x's shape; `out` may be `above` (in place)."""
    xp, xs, n, c, hw = _map_ptr(x, "x")
    yp, ys = _map_ptr(y, "y")[:2]
    if tuple(x.shape) != tuple(y.shape) or (above is not None and tuple(above.shape) != tuple(x.shape)):
        raise VfiLibraryError("lpips_head_backward: shape mismatch")
    if out is None:
        out = new(tuple(x.shape), x)
    elif tuple(out.shape) != tuple(x.shape):
        raise VfiLibraryError("lpips_head_backward: out shape mismatch")
    ap, as_ = (None, 0) if above is None else _map_ptr(above, "above")[:2]
    op, os_ = _map_ptr(out, "out")[:2]
    _lib.call("vfi_lpips_head_backward", xp, xs, yp, ys, _vec(w, c, "w"), _vec(upstream, n, "upstream"), ap, as_, op, os_, n, c,
              hw, int(bool(relu_mask)), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * hw * (3 + (above is not None)), "lpips_head_backward"))
    return out


def lpips_normalize(x, adjoint=False, out=None):
    """(x - mean_c) / std_c of (N, 3, H, W) images in [0, 1] (ImageNet statistics); adjoint: x / std_c."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise VfiLibraryError(f"lpips_normalize: (N, 3, H, W) expected, got {tuple(x.shape)}")
    if out is None:
        out = new(tuple(x.shape), x)
    xp, xs = _slice_ptr(x, "x")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_lpips_normalize", xp, xs, op, os_, x.shape[0], x.shape[2] * x.shape[3], int(bool(adjoint)), _lib.stream_ptr(),
              work=_prof("byte", 8.0 * x.numel(), "lpips_normalize"))
    return out


# ---- SSIM as a loss --------------------------------------------------------------------------
def ssim_loss_forward(x, y, kernel_size=11, sigma=1.5, c1=0.01 ** 2, c2=0.03 ** 2):
    """-> (N,) = 1 - mean SSIM of (N, C, H, W) images, one pass; x, y may be the two halves of one tensor."""
    xp, xs = _slice_ptr(x, "x")
    yp, ys = _slice_ptr(y, "y")
    if tuple(x.shape) != tuple(y.shape):
        raise VfiLibraryError("ssim_loss_forward: shape mismatch")
    n, c, h, w = x.shape
    out = new((n,), x)
    _lib.call("vfi_ssim_loss_forward", xp, xs, yp, ys, out.data_ptr(), _reduce_workspace(x).data_ptr(), n, c, h, w,
              int(kernel_size), float(sigma), float(c1), float(c2), _lib.stream_ptr(),
              work=_prof("byte", 8.0 * n * c * h * w, "ssim_loss_forward"))
    return out


def ssim_loss_backward(x, y, upstream, kernel_size=11, sigma=1.5, c1=0.01 ** 2, c2=0.03 ** 2, out=None):
    """-> upstream[n] * d ssim_loss_forward(x, y)[n] / dx, of x's shape; for y's gradient exchange x and y."""
    xp, xs = _slice_ptr(x, "x")
    yp, ys = _slice_ptr(y, "y")
    if tuple(x.shape) != tuple(y.shape):
        raise VfiLibraryError("ssim_loss_backward: shape mismatch")
    n, c, h, w = x.shape
    if out is None:
        out = new(tuple(x.shape), x)
    elif tuple(out.shape) != tuple(x.shape):
        raise VfiLibraryError("ssim_loss_backward: out shape mismatch")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_ssim_loss_backward", xp, xs, yp, ys, _vec(upstream, n, "upstream"), op, os_, n, c, h, w, int(kernel_size),
              float(sigma), float(c1), float(c2), _lib.stream_ptr(),
              work=_prof("byte", 12.0 * n * c * h * w, "ssim_loss_backward"))
    return out


def avg_pool(x, f):
    """F.avg_pool2d(kernel_size=f) of a dense (N, C, H, W) tensor (floor)."""
    n, c, h, w = x.shape
    out = new((n, c, h // f, w // f), x)
    _lib.call("vfi_avg_pool", _lib.dptr(x, "x"), out.data_ptr(), n * c, h, w, int(f), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * (x.numel() + out.numel()), "avg_pool"))
    return out


def avg_pool_backward(grad, size, f):
    """Adjoint of avg_pool for an input of spatial `size`: grad / f^2 over each window, 0 where the floor dropped pixels."""
    n, c, ho, wo = grad.shape
    h, w = size
    if (ho, wo) != (h // f, w // f):
        raise VfiLibraryError(f"avg_pool_backward: grad {tuple(grad.shape)} is not ({h}, {w}) pooled by {f}")
    out = new((n, c, h, w), grad)
    _lib.call("vfi_avg_pool_backward", _lib.dptr(grad, "grad"), out.data_ptr(), n * c, h, w, int(f), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * (grad.numel() + out.numel()), "avg_pool_backward"))
    return out


# ---- glue of a PhaseNet level's backward -----------------------------------------------------
def resize_bilinear_adjoint(grad, size, out=None):
    """Adjoint of resize_bilinear(x, grad's size, align_corners=False) for x of spatial `size` (any sizes; gather form)."""
    n, c, ho, wo = grad.shape
    h, w = size
    if out is None:
        out = new((n, c, h, w), grad)
    elif tuple(out.shape) != (n, c, h, w):
        raise VfiLibraryError(f"resize_bilinear_adjoint: out shape {tuple(out.shape)} != {(n, c, h, w)}")
    gp, gs = _slice_ptr(grad, "grad")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_resize_bilinear_adjoint", gp, gs, op, os_, n, c, int(h), int(w), ho, wo, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * (h * w + ho * wo), "resize_bilinear_adjoint"))
    return out


def act_backward_(grad, y, act, out=None):
    """grad * f'(y) from the activation's output y, act in 'elu' | 'tanh'; in place unless `out` is given."""
    n = grad.shape[0]
    count = grad[0].numel()
    if act not in ("elu", "tanh"):
        raise VfiLibraryError(f"act_backward_: no backward for activation {act!r}")
    if tuple(y.shape) != tuple(grad.shape) or (out is not None and tuple(out.shape) != tuple(grad.shape)):
        raise VfiLibraryError("act_backward_: shape mismatch")
    gp, gs = _slice_ptr(grad, "grad")
    yp, ys = _slice_ptr(y, "y")
    op, os_ = (gp, gs) if out is None else _slice_ptr(out, "out")
    _lib.call("vfi_act_backward", gp, gs, yp, ys, op, os_, n, count, ACT[act], _lib.stream_ptr(),
              work=_prof("byte", 12.0 * n * count, "act_backward"))
    return grad if out is None else out


def phasenet_emit(pred, amp_in, max_amp):
    """One band level's outputs (vfi_phasenet_emit): pred (N,8,H,W), amp_in (N,8,H,W) normalised amplitudes, max_amp (N,)
    -> (phase, amp), each (N*4,1,H,W) in the per-image layout colour*4+band."""
    n, c, h, w = pred.shape
    if c != 8 or tuple(amp_in.shape) != (n, 8, h, w) or max_amp.numel() != n:
        raise VfiLibraryError("phasenet_emit: pred and amp_in must be (N,8,H,W), max_amp (N,)")
    pp, ps = _slice_ptr(pred, "pred")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    phase, amp = new((n * 4, 1, h, w), pred), new((n * 4, 1, h, w), pred)
    _lib.call("vfi_phasenet_emit", pp, ps, ap, as_, _lib.dptr(max_amp, "max_amp"), phase.data_ptr(), amp.data_ptr(), n, h * w,
              _lib.stream_ptr())
    return phase, amp


def phasenet_emit_backward(grad_phase, grad_amp, amp_in, max_amp):
    """grad of phasenet_emit's pred (N,8,H,W) from the gradients of its outputs (either may be None = zero)."""
    n, _, h, w = amp_in.shape
    g = grad_phase if grad_phase is not None else grad_amp
    if g is None or g.numel() != n * 4 * h * w:
        raise VfiLibraryError("phasenet_emit_backward: gradient shape mismatch")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    out = new((n, 8, h, w), amp_in)
    _lib.call("vfi_phasenet_emit_backward", _lib.dptr(grad_phase, "grad_phase"), _lib.dptr(grad_amp, "grad_amp"), ap, as_,
              _lib.dptr(max_amp, "max_amp"), out.data_ptr(), out.stride(0), n, h * w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * h * w * 24, "phasenet_emit_backward"))
    return out


def phasenet_predict(feat, pc, amp_in, max_amp, pred=None):
    """A band level's head in one call (vfi_phasenet_predict): feat (N,64,H,W), pc the PackedConv of the 64 -> 8 1x1 prediction
    map, amp_in (N,8,H,W), max_amp (N,) -> (pred (N,8,H,W) post-tanh, phase, amp (N*4,1,H,W)).  Small or odd-sized levels run
    vfi_conv2d + vfi_phasenet_emit inside the library."""
    n, cin, h, w = feat.shape
    if pc.cout != 8 or pc.ks != 1 or pc.cin != cin or tuple(amp_in.shape) != (n, 8, h, w) or max_amp.numel() != n:
        raise VfiLibraryError("phasenet_predict: needs a 1x1 map with 8 outputs, amp_in (N,8,H,W) and max_amp (N,)")
    if pred is None:
        pred = new((n, 8, h, w), feat)
    elif tuple(pred.shape) != (n, 8, h, w):
        raise VfiLibraryError(f"phasenet_predict: pred shape {tuple(pred.shape)} != {(n, 8, h, w)}")
    fp, fs = _slice_ptr(feat, "feat")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    pp, ps = _slice_ptr(pred, "pred")
    phase, amp = new((n * 4, 1, h, w), feat), new((n * 4, 1, h, w), feat)
    _lib.call("vfi_phasenet_predict", fp, fs, pc.packed.data_ptr(), pc.bias.data_ptr(), ap, as_, _lib.dptr(max_amp, "max_amp"),
              pp, ps, phase.data_ptr(), amp.data_ptr(), n, cin, h, w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * (cin + 8 + 8 + 8) * h * w, "phasenet_predict_kernel"))
    return pred, phase, amp


def phasenet_predict_backward(feat, pred, amp_in, max_amp, weight, grad_phase=None, grad_amp=None, grad_pred_in=None,
                              need_feat=True, need_weight=True, need_bias=True, out=None):
    """Adjoint of phasenet_predict in one pass (vfi_phasenet_predict_backward): -> (grad_feat (N,64,H,W), grad_weight
    (8,64,1,1), grad_bias (8,)), None where not needed.  feat, pred, amp_in, grad_pred_in may be channel slices; weight is the
    prediction map's (8,64,1,1) parameter; grad_phase / grad_amp (N*4,1,H,W) dense; a missing upstream gradient is zero.
    `out`: where grad_feat goes (a channel slice is fine)."""
    n, cin, h, w = feat.shape
    if cin != 64 or tuple(pred.shape) != (n, 8, h, w) or tuple(weight.shape) != (8, 64, 1, 1):
        raise VfiLibraryError("phasenet_predict_backward: feat (N,64,H,W), pred (N,8,H,W), weight (8,64,1,1)")
    if not (need_feat or need_weight or need_bias):
        raise VfiLibraryError("phasenet_predict_backward: no output asked for")
    for g, name in ((grad_phase, "grad_phase"), (grad_amp, "grad_amp")):
        if g is not None and g.numel() != n * 4 * h * w:
            raise VfiLibraryError(f"phasenet_predict_backward: {name} shape mismatch")
    if grad_pred_in is not None and tuple(grad_pred_in.shape) != (n, 8, h, w):
        raise VfiLibraryError("phasenet_predict_backward: grad_pred_in shape mismatch")
    if grad_amp is not None and (tuple(amp_in.shape) != (n, 8, h, w) or max_amp.numel() != n):
        raise VfiLibraryError("phasenet_predict_backward: amp_in must be (N,8,H,W), max_amp (N,)")
    fp, fs = _slice_ptr(feat, "feat")
    pp, ps = _slice_ptr(pred, "pred")
    ap, as_ = (None, 0) if grad_amp is None else _slice_ptr(amp_in, "amp_in")
    ip, is_ = (None, 0) if grad_pred_in is None else _slice_ptr(grad_pred_in, "grad_pred_in")
    gf = None
    if need_feat:
        gf = new((n, 64, h, w), feat) if out is None else out
        if tuple(gf.shape) != (n, 64, h, w):
            raise VfiLibraryError(f"phasenet_predict_backward: out shape {tuple(gf.shape)} != {(n, 64, h, w)}")
    gp, gs = (None, 0) if gf is None else _slice_ptr(gf, "out")
    gw = new((8, 64, 1, 1), feat) if need_weight else None
    gb = new((8,), feat) if need_bias else None
    ws = torch.empty(_lib.PHASENET_HEAD_WORKSPACE_FLOATS, dtype=torch.float32, device=feat.device) if need_weight or need_bias else None
    planes = 8 + 64 * (need_weight or need_bias) + 64 * need_feat + 4 * (grad_phase is not None) + 12 * (grad_amp is not None) + \
        8 * (grad_pred_in is not None)
    _lib.call("vfi_phasenet_predict_backward", fp, fs, pp, ps, ap, as_, _lib.dptr(max_amp, "max_amp") if grad_amp is not None else None,
              _lib.dptr(weight.detach(), "weight"), _lib.dptr(grad_phase, "grad_phase"), _lib.dptr(grad_amp, "grad_amp"), ip, is_,
              gp, gs, _lib.dptr(gw), _lib.dptr(gb), _lib.dptr(ws), n, h * w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * h * w * planes, "phasenet_predict_backward"))
    return gf, gw, gb


# ---- batch-statistics BatchNorm of a PhaseNet block ----------------------------------------------
def _channel_vec(t, c, name):
    if t.numel() != c:
        raise VfiLibraryError(f"{name} must hold {c} floats, got {tuple(t.shape)}")
    return _lib.dptr(t.detach(), name)


def bn_stats(y):
    """Per-channel (mean, biased variance) of y (N,C,H,W; may be a channel slice) over samples and pixels (vfi_bn_stats):
    nn.BatchNorm2d's batch statistics.  One value per channel raises ValueError, as torch does."""
    n, c, h, w = y.shape
    if n * h * w < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
    yp, ys = _slice_ptr(y, "y")
    mean, var = new((c,), y), new((c,), y)
    _lib.call("vfi_bn_stats", yp, ys, n, c, h * w, mean.data_ptr(), var.data_ptr(), _reduce_workspace(y).data_ptr(),
              _lib.stream_ptr(), work=_prof("byte", 4.0 * n * c * h * w, "bn_stats"))
    return mean, var


def bn_act_forward(y, mean, var, gamma, beta, eps, act="elu", out=None):
    """act(gamma (y - mean) / sqrt(var + eps) + beta), act in None | 'elu' (vfi_bn_act_forward); y and out may be channel
    slices, out may be y."""
    n, c, h, w = y.shape
    if act not in (None, "none", "elu"):
        raise VfiLibraryError(f"bn_act_forward: activation {act!r} (none and elu only)")
    if out is None:
        out = new((n, c, h, w), y)
    elif tuple(out.shape) != (n, c, h, w):
        raise VfiLibraryError(f"bn_act_forward: out shape {tuple(out.shape)} != {(n, c, h, w)}")
    yp, ys = _slice_ptr(y, "y")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_bn_act_forward", yp, ys, _channel_vec(mean, c, "mean"), _channel_vec(var, c, "var"),
              _channel_vec(gamma, c, "gamma"), _channel_vec(beta, c, "beta"), float(eps), ACT[act], op, os_, n, c, h * w,
              _lib.stream_ptr(), work=_prof("byte", 8.0 * n * c * h * w, "bn_act_forward"))
    return out


def bn_act_backward(g_t, t, y, mean, var, gamma, eps, act="elu", need_data=True, out=None):
    """Adjoint of bn_stats + bn_act_forward (vfi_bn_act_backward) -> (g_y or None, g_gamma (C,), g_beta (C,)).  g_t, t, y may
    be channel slices; t is the forward's output (None without an activation).  `out`: where g_y goes, g_t itself is fine;
    need_data=False skips g_y."""
    n, c, h, w = g_t.shape
    if act not in (None, "none", "elu"):
        raise VfiLibraryError(f"bn_act_backward: activation {act!r} (none and elu only)")
    elu = act == "elu"
    if tuple(y.shape) != (n, c, h, w) or (elu and (t is None or tuple(t.shape) != (n, c, h, w))):
        raise VfiLibraryError("bn_act_backward: shape mismatch")
    gp, gs = _slice_ptr(g_t, "g_t")
    tp, ts = _slice_ptr(t, "t") if elu else (None, 0)
    yp, ys = _slice_ptr(y, "y")
    g_y = None
    if need_data:
        g_y = new((n, c, h, w), g_t) if out is None else out
        if tuple(g_y.shape) != (n, c, h, w):
            raise VfiLibraryError(f"bn_act_backward: out shape {tuple(g_y.shape)} != {(n, c, h, w)}")
    op, os_ = (None, 0) if g_y is None else _slice_ptr(g_y, "out")
    g_gamma, g_beta = new((c,), g_t), new((c,), g_t)
    _lib.call("vfi_bn_act_backward", gp, gs, tp, ts, yp, ys, _channel_vec(mean, c, "mean"), _channel_vec(var, c, "var"),
              _channel_vec(gamma, c, "gamma"), float(eps), ACT[act], op, os_, g_gamma.data_ptr(), g_beta.data_ptr(),
              _reduce_workspace(g_t).data_ptr(), n, c, h * w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * h * w * ((2 + elu) * (1 + need_data) + need_data), "bn_act_backward"))
    return g_y, g_gamma, g_beta


# ---- the AdaCoF trainer's discriminator -----------------------------------------------------------
def bn_leaky_forward(y, mean, var, gamma, beta, eps, slope, out=None):
    """leaky(gamma (y - mean) / sqrt(var + eps) + beta), leaky(z) = z if z > 0 else slope z (vfi_bn_leaky_forward); y and out
    may be channel slices, out may be y."""
    n, c, h, w = y.shape
    if out is None:
        out = new((n, c, h, w), y)
    elif tuple(out.shape) != (n, c, h, w):
        raise VfiLibraryError(f"bn_leaky_forward: out shape {tuple(out.shape)} != {(n, c, h, w)}")
    yp, ys = _slice_ptr(y, "y")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_bn_leaky_forward", yp, ys, _channel_vec(mean, c, "mean"), _channel_vec(var, c, "var"),
              _channel_vec(gamma, c, "gamma"), _channel_vec(beta, c, "beta"), float(eps), float(slope), op, os_, n, c, h * w,
              _lib.stream_ptr(), work=_prof("byte", 8.0 * n * c * h * w, "bn_leaky_forward"))
    return out


def bn_leaky_backward(g_t, t, y, mean, var, gamma, eps, slope, need_data=True, out=None):
    """Adjoint of bn_stats + bn_leaky_forward (vfi_bn_leaky_backward) -> (g_y or None, g_gamma (C,), g_beta (C,)); t is the
    forward's output (its sign gives the LeakyReLU's derivative).  `out`: where g_y goes, g_t itself is fine."""
    n, c, h, w = g_t.shape
    if tuple(y.shape) != (n, c, h, w) or tuple(t.shape) != (n, c, h, w):
        raise VfiLibraryError("bn_leaky_backward: shape mismatch")
    gp, gs = _slice_ptr(g_t, "g_t")
    tp, ts = _slice_ptr(t, "t")
    yp, ys = _slice_ptr(y, "y")
    g_y = None
    if need_data:
        g_y = new((n, c, h, w), g_t) if out is None else out
        if tuple(g_y.shape) != (n, c, h, w):
            raise VfiLibraryError(f"bn_leaky_backward: out shape {tuple(g_y.shape)} != {(n, c, h, w)}")
    op, os_ = (None, 0) if g_y is None else _slice_ptr(g_y, "out")
    g_gamma, g_beta = new((c,), g_t), new((c,), g_t)
    _lib.call("vfi_bn_leaky_backward", gp, gs, tp, ts, yp, ys, _channel_vec(mean, c, "mean"), _channel_vec(var, c, "var"),
              _channel_vec(gamma, c, "gamma"), float(eps), float(slope), op, os_, g_gamma.data_ptr(), g_beta.data_ptr(),
              _reduce_workspace(g_t).data_ptr(), n, c, h * w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * h * w * (3 * (1 + need_data) + need_data), "bn_leaky_backward"))
    return g_y, g_gamma, g_beta


def phase_split(x, out=None):
    """xs (N, 4C, ceil(H/2), ceil(W/2)) with xs[n, (2 py + px) C + c, i, j] = x[n, c, 2 i + py, 2 j + px], zero beyond the
    edge (vfi_phase_split): the tensor whose stride-1 3x3 convolution is x's stride-2 one."""
    n, c, h, w = x.shape
    shape = (n, 4 * c, (h + 1) // 2, (w + 1) // 2)
    if out is None:
        out = new(shape, x)
    elif tuple(out.shape) != shape:
        raise VfiLibraryError(f"phase_split: out shape {tuple(out.shape)} != {shape}")
    xp, xs = _slice_ptr(x, "x")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_phase_split", xp, xs, op, os_, n, c, h, w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * (h * w + 4 * shape[2] * shape[3]), "phase_split"))
    return out


def phase_merge(gs, size, out=None):
    """Adjoint of phase_split: (N, C, H, W) = size's (H, W) from gs (N, 4C, ceil(H/2), ceil(W/2)) (vfi_phase_merge)."""
    n, c4, h2, w2 = gs.shape
    h, w = size
    if c4 % 4 or (h + 1) // 2 != h2 or (w + 1) // 2 != w2:
        raise VfiLibraryError(f"phase_merge: {tuple(gs.shape)} is no phase split of a {h}x{w} tensor")
    c = c4 // 4
    if out is None:
        out = new((n, c, h, w), gs)
    elif tuple(out.shape) != (n, c, h, w):
        raise VfiLibraryError(f"phase_merge: out shape {tuple(out.shape)} != {(n, c, h, w)}")
    gp, gs_ = _slice_ptr(gs, "gs")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_phase_merge", gp, gs_, op, os_, n, c, h, w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * c * (h * w + 4 * h2 * w2), "phase_merge"))
    return out


# tap k of an axis of the stride-2 filter -> (phase, tap) of the stride-1 filter over the split tensor
_STRIDE2_TAP = ((1, 0), (0, 1), (1, 1))
_STRIDE2_INDEX = {}


def _stride2_index(device):
    """For each of the 9 taps (ky, kx) its position among the 36 = (phase 2 py + px, ty, tx) of the expanded filter (cached
    per device)."""
    idx = _STRIDE2_INDEX.get(device)
    if idx is None:
        pos = [(2 * _STRIDE2_TAP[ky][0] + _STRIDE2_TAP[kx][0]) * 9 + _STRIDE2_TAP[ky][1] * 3 + _STRIDE2_TAP[kx][1]
               for ky in range(3) for kx in range(3)]
        idx = _STRIDE2_INDEX[device] = torch.tensor(pos, dtype=torch.long, device=device)
    return idx


def stride2_weight(weight):
    """(Cout, 4C, 3, 3) filter of the stride-1 convolution over phase_split(x) that equals the 3x3 / stride 2 / pad 1
    convolution of x with `weight` (Cout, C, 3, 3): 9 of every 36 entries are non-zero."""
    cout, c, kh, kw = weight.shape
    if (kh, kw) != (3, 3):
        raise VfiLibraryError(f"stride2_weight: 3x3 filters only, got {kh}x{kw}")
    wz = weight.new_zeros((cout, c, 36))
    wz.index_copy_(2, _stride2_index(weight.device), weight.detach().reshape(cout, c, 9))
    return wz.view(cout, c, 4, 9).permute(0, 2, 1, 3).reshape(cout, 4 * c, 3, 3)


def stride2_weight_gather(dw4):
    """The adjoint of stride2_weight: (Cout, C, 3, 3) gathered from the (Cout, 4C, 3, 3) gradient of the expanded filter."""
    cout, c4 = dw4.shape[:2]
    c = c4 // 4
    flat = dw4.view(cout, 4, c, 9).permute(0, 2, 1, 3).reshape(cout, c, 36)
    return flat.index_select(2, _stride2_index(dw4.device)).view(cout, c, 3, 3)


def conv2d_stride2(x, pc, act=None, out=None, split=None):
    """act(conv(x) + bias), 3x3 / stride 2 / zero pad 1, as phase_split + one stride-1 vfi_conv2d; `pc` =
    PackedConv(stride2_weight(weight), bias).  `split`: phase_split(x) when the caller already has it."""
    xs = phase_split(x) if split is None else split
    return conv2d(xs, pc, "zeros", act, out=out)


def conv2d_stride2_backward_data(dy, pct, size, out=None):
    """dX (N, C, H, W), (H, W) = size, of conv2d_stride2 from dy (N, Cout, ceil(H/2), ceil(W/2)); `pct` =
    packed_transposed(stride2_weight(weight)): vfi_conv2d_backward_data, then phase_merge."""
    return phase_merge(conv2d_backward_data(dy, pct, "zeros"), size, out=out)


def conv2d_stride2_backward_weight(x, dy, bias=True, split=None):
    """(dW (Cout, C, 3, 3), dbias or None) of conv2d_stride2: vfi_conv2d_backward_weight on phase_split(x) (or `split`),
    then the gather of the 9 live taps of every 36."""
    xs = phase_split(x) if split is None else split
    dw4, db = conv2d_backward_weight(xs, dy, 3, "zeros", bias=bias)
    return stride2_weight_gather(dw4), db


def _matrix(t, rows, cols, name):
    if t is None:
        return None
    if tuple(t.shape) != (rows, cols):
        raise VfiLibraryError(f"{name} must be {(rows, cols)}, got {tuple(t.shape)}")
    return _lib.dptr(t.detach(), name)


def linear_forward(x, weight, bias=None, slope=1.0):
    """leaky(x (B, K) weight^T (J, K) + bias) -> (B, J), slope 1 = no activation (vfi_linear_forward)."""
    b, k = x.shape
    j = weight.shape[0]
    y = new((b, j), x)
    _lib.call("vfi_linear_forward", _matrix(x, b, k, "x"), _matrix(weight, j, k, "weight"),
              None if bias is None else _vec(bias.detach(), j, "bias"), y.data_ptr(), b, k, j, float(slope), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * (j * k * ((b + 3) // 4) + b * k + b * j), "linear_forward"))
    return y


def linear_backward(x, weight, y, slope, g, need_x=True, need_w=True, need_bias=True):
    """(dx (B, K), dw (J, K), dbias (J)) of linear_forward from the gradient g of its output y; an output not needed is None
    (vfi_linear_backward: one pass over weight for dx and dw together)."""
    b, j = g.shape
    k = weight.shape[1] if weight is not None else x.shape[1]
    dx = new((b, k), g) if need_x else None
    dw = new((j, k), g) if need_w else None
    db = new((j,), g) if need_bias else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.call("vfi_linear_backward", _matrix(x, b, k, "x") if need_w else None, _matrix(weight, j, k, "weight") if need_x else None,
              _matrix(y, b, j, "y") if slope != 1.0 else None, float(slope), _matrix(g, b, j, "g"), ptr(dx), ptr(dw), ptr(db),
              b, k, j, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * j * k * ((b + 3) // 4) * (int(need_x) + int(need_w)) + 4.0 * b * k * (need_x + need_w),
                         "linear_backward"))
    return dx, dw, db


# ---- the WGAN_GP term ------------------------------------------------------------------------------
def _runs(t, name):
    """(address, batch stride, N, count) of a tensor of N batch-strided dense runs: NCHW (maybe a channel slice) or (B, K)."""
    if isinstance(t, torch.Tensor) and t.dim() == 2:
        t = t.unsqueeze(-1).unsqueeze(-1)
    p, s = _slice_ptr(t, name)
    return p, s, t.shape[0], t[0].numel()


def leaky_mask(a, s, slope, out=None):
    """s > 0 ? a : slope * a (vfi_leaky_mask) -> out (default: a new tensor).  `s is a`: LeakyReLU itself; `out is a`: the
    mask of a gradient or of a tangent in place, s the activation's output.  4-d (channel slices allowed) or 2-d tensors."""
    if tuple(s.shape) != tuple(a.shape) or (out is not None and tuple(out.shape) != tuple(a.shape)):
        raise VfiLibraryError("leaky_mask: shape mismatch")
    if out is None:
        out = torch.empty(tuple(a.shape), dtype=torch.float32, device=a.device)
    ap, as_, n, count = _runs(a, "a")
    sp, ss, _, _ = _runs(s, "s")
    op, os_, _, _ = _runs(out, "out")
    _lib.call("vfi_leaky_mask", ap, as_, sp, ss, op, os_, n, count, float(slope), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * count * (2 + (sp != ap)), "leaky_mask"))
    return out


def gp_mix(fake, real, eps):
    """fake * (1 - eps) + real * eps, the bits of that float32 torch expression (vfi_gp_mix): WGAN_GP's interpolate."""
    if tuple(real.shape) != tuple(fake.shape) or tuple(eps.shape) != tuple(fake.shape):
        raise VfiLibraryError("gp_mix: shape mismatch")
    hat = torch.empty(tuple(fake.shape), dtype=torch.float32, device=fake.device)
    fp, fs, n, count = _runs(fake, "fake")
    rp, rs, _, _ = _runs(real, "real")
    ep, es, _, _ = _runs(eps, "eps")
    _lib.call("vfi_gp_mix", fp, fs, rp, rs, ep, es, hat.data_ptr(), count, n, count, _lib.stream_ptr(),
              work=_prof("byte", 16.0 * n * count, "gp_mix"))
    return hat


def grad_penalty_forward(g, weight=10.0):
    """(value 0-d, norms (B,)): norms[b] = ||g[b]||_2, value = weight * mean_b (norms[b] - 1)^2 (vfi_grad_penalty_forward)."""
    gp, gs, b, n = _runs(g, "g")
    norms, value = new((b,), g), new((1,), g)
    _lib.call("vfi_grad_penalty_forward", gp, gs, norms.data_ptr(), value.data_ptr(), b, n, float(weight), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * b * n, "grad_penalty_forward"))
    return value[0], norms


def grad_penalty_backward(g, norms, upstream, weight=10.0):
    """upstream * d value / d g, of g's shape; a row of norm 0 gives zeros (vfi_grad_penalty_backward)."""
    gp, gs, b, n = _runs(g, "g")
    out = torch.empty(tuple(g.shape), dtype=torch.float32, device=g.device)
    _lib.call("vfi_grad_penalty_backward", gp, gs, _vec(norms, b, "norms"), _lib.dptr(upstream.reshape(1), "upstream"),
              out.data_ptr(), n, b, n, float(weight), _lib.stream_ptr(), work=_prof("byte", 8.0 * b * n, "grad_penalty_backward"))
    return out


def phasenet_emit_low(pred, low_in, max_low):
    """The low level's output (vfi_phasenet_emit_low): pred (N,1,H,W), low_in (N,2,H,W) normalised, max_low (N,) -> (N,1,H,W)."""
    n, c, h, w = pred.shape
    if c != 1 or tuple(low_in.shape) != (n, 2, h, w) or max_low.numel() != n:
        raise VfiLibraryError("phasenet_emit_low: pred must be (N,1,H,W), low_in (N,2,H,W), max_low (N,)")
    pp, ps = _slice_ptr(pred, "pred")
    lp, ls = _slice_ptr(low_in, "low_in")
    low = new((n, 1, h, w), pred)
    _lib.call("vfi_phasenet_emit_low", pp, ps, lp, ls, _lib.dptr(max_low, "max_low"), low.data_ptr(), n, h * w,
              _lib.stream_ptr())
    return low


# ---- PhaseNet's level head with two, three or four input images ------------------------------------
def phasenet_pred_channels(num_img):
    """(low level's, a band level's) prediction channels of PhaseNet(num_img) (reference phase_net.py:23-35)."""
    if num_img not in (2, 3, 4):
        raise VfiLibraryError(f"PhaseNet has 2, 3 or 4 input images, not {num_img}")
    return (2, 12) if num_img == 3 else (1, 8)


def phasenet_emit_n(pred, amp_in, max_amp, num_img):
    """phasenet_emit for num_img images (vfi_phasenet_emit_n): pred (N,P,H,W), P = 12 for three images and 8 otherwise, amp_in
    (N,4*num_img,H,W), max_amp (N,) -> (phase, amp), each (N*4,1,H,W).  Three images: the second blend with amp_in[:,8:12]."""
    p_band = phasenet_pred_channels(num_img)[1]
    n, c, h, w = pred.shape
    if c != p_band or tuple(amp_in.shape) != (n, 4 * num_img, h, w) or max_amp.numel() != n:
        raise VfiLibraryError(f"phasenet_emit_n: pred must be (N,{p_band},H,W), amp_in (N,{4 * num_img},H,W), max_amp (N,)")
    pp, ps = _slice_ptr(pred, "pred")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    phase, amp = new((n * 4, 1, h, w), pred), new((n * 4, 1, h, w), pred)
    _lib.call("vfi_phasenet_emit_n", pp, ps, ap, as_, _lib.dptr(max_amp, "max_amp"), phase.data_ptr(), amp.data_ptr(), n, h * w,
              num_img, _lib.stream_ptr())
    return phase, amp


def phasenet_emit_low_n(pred, low_in, max_low, num_img):
    """phasenet_emit_low for num_img images (vfi_phasenet_emit_low_n): pred (N,P,H,W), P = 2 for three images and 1 otherwise,
    low_in (N,num_img,H,W) normalised, max_low (N,) -> (N,1,H,W)."""
    p_low = phasenet_pred_channels(num_img)[0]
    n, c, h, w = pred.shape
    if c != p_low or tuple(low_in.shape) != (n, num_img, h, w) or max_low.numel() != n:
        raise VfiLibraryError(f"phasenet_emit_low_n: pred must be (N,{p_low},H,W), low_in (N,{num_img},H,W), max_low (N,)")
    pp, ps = _slice_ptr(pred, "pred")
    lp, ls = _slice_ptr(low_in, "low_in")
    low = new((n, 1, h, w), pred)
    _lib.call("vfi_phasenet_emit_low_n", pp, ps, lp, ls, _lib.dptr(max_low, "max_low"), low.data_ptr(), n, h * w, num_img,
              _lib.stream_ptr())
    return low


def phasenet_predict_n(feat, pc, amp_in, max_amp, num_img, pred=None):
    """phasenet_predict for num_img images (vfi_phasenet_predict_n): feat (N,64,H,W), pc the PackedConv of the 64 -> P 1x1
    prediction map (P = 12 for three images, 8 otherwise), amp_in (N,4*num_img,H,W), max_amp (N,) -> (pred (N,P,H,W) post-tanh,
    phase, amp (N*4,1,H,W)).  Small or odd-sized levels run vfi_conv2d + vfi_phasenet_emit_n inside the library."""
    p_band = phasenet_pred_channels(num_img)[1]
    n, cin, h, w = feat.shape
    if pc.cout != p_band or pc.ks != 1 or pc.cin != cin or tuple(amp_in.shape) != (n, 4 * num_img, h, w) or max_amp.numel() != n:
        raise VfiLibraryError(f"phasenet_predict_n: needs a 1x1 map with {p_band} outputs, amp_in (N,{4 * num_img},H,W) and max_amp (N,)")
    if pred is None:
        pred = new((n, p_band, h, w), feat)
    elif tuple(pred.shape) != (n, p_band, h, w):
        raise VfiLibraryError(f"phasenet_predict_n: pred shape {tuple(pred.shape)} != {(n, p_band, h, w)}")
    fp, fs = _slice_ptr(feat, "feat")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    pp, ps = _slice_ptr(pred, "pred")
    phase, amp = new((n * 4, 1, h, w), feat), new((n * 4, 1, h, w), feat)
    planes = cin + p_band + 8 + (12 if num_img == 3 else 8)             # read: features, the blended amplitudes; written: pred, outputs
    _lib.call("vfi_phasenet_predict_n", fp, fs, pc.packed.data_ptr(), pc.bias.data_ptr(), ap, as_, _lib.dptr(max_amp, "max_amp"),
              pp, ps, phase.data_ptr(), amp.data_ptr(), n, cin, h, w, num_img, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * planes * h * w, "phasenet_predict_fuse_kernel" if num_img == 3 else "phasenet_predict_kernel"))
    return pred, phase, amp


def phasenet_emit_low_backward(grad_low, low_in, max_low):
    n, _, h, w = low_in.shape
    if grad_low.numel() != n * h * w:
        raise VfiLibraryError("phasenet_emit_low_backward: gradient shape mismatch")
    lp, ls = _slice_ptr(low_in, "low_in")
    out = new((n, 1, h, w), low_in)
    _lib.call("vfi_phasenet_emit_low_backward", _lib.dptr(grad_low, "grad_low"), lp, ls, _lib.dptr(max_low, "max_low"),
              out.data_ptr(), out.stride(0), n, h * w, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * h * w * 4, "phasenet_emit_low_backward"))
    return out


# ---- the adjoints of the three heads above ----------------------------------------------------------
def phasenet_emit_n_backward(grad_phase, grad_amp, pred, amp_in, max_amp, num_img, out=None):
    """grad of phasenet_emit_n's pred (N,P,H,W) from the gradients of its outputs (either may be None = zero).  pred (the
    forward's input) is read for three images only, by the second blend's adjoint; amp_in is passed whole (N,4*num_img,H,W).
    `out`: where the gradient goes (a channel slice is fine)."""
    p_band = phasenet_pred_channels(num_img)[1]
    n, c, h, w = amp_in.shape
    if c != 4 * num_img or tuple(pred.shape) != (n, p_band, h, w) or max_amp.numel() != n:
        raise VfiLibraryError(f"phasenet_emit_n_backward: pred must be (N,{p_band},H,W), amp_in (N,{4 * num_img},H,W), max_amp (N,)")
    if grad_phase is None and grad_amp is None:
        raise VfiLibraryError("phasenet_emit_n_backward: no upstream gradient")
    for g, name in ((grad_phase, "grad_phase"), (grad_amp, "grad_amp")):
        if g is not None and g.numel() != n * 4 * h * w:
            raise VfiLibraryError(f"phasenet_emit_n_backward: {name} shape mismatch")
    if out is None:
        out = new((n, p_band, h, w), amp_in)
    elif tuple(out.shape) != (n, p_band, h, w):
        raise VfiLibraryError(f"phasenet_emit_n_backward: out shape {tuple(out.shape)} != {(n, p_band, h, w)}")
    pp, ps = _slice_ptr(pred, "pred")
    ap, as_ = _slice_ptr(amp_in, "amp_in")
    op, os_ = _slice_ptr(out, "out")
    planes = p_band + 4 * (grad_phase is not None) + (4 + (20 if num_img == 3 else 8)) * (grad_amp is not None)
    _lib.call("vfi_phasenet_emit_n_backward", _lib.dptr(grad_phase, "grad_phase"), _lib.dptr(grad_amp, "grad_amp"), pp, ps, ap, as_,
              _lib.dptr(max_amp, "max_amp"), op, os_, n, h * w, num_img, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * h * w * planes, "phasenet_emit_n_backward"))
    return out


def phasenet_emit_low_n_backward(grad_low, pred, low_in, max_low, num_img, out=None):
    """grad of phasenet_emit_low_n's pred (N,P,H,W), P = 2 for three images and 1 otherwise; low_in whole (N,num_img,H,W)."""
    p_low = phasenet_pred_channels(num_img)[0]
    n, c, h, w = low_in.shape
    if c != num_img or tuple(pred.shape) != (n, p_low, h, w) or max_low.numel() != n:
        raise VfiLibraryError(f"phasenet_emit_low_n_backward: pred must be (N,{p_low},H,W), low_in (N,{num_img},H,W), max_low (N,)")
    if grad_low.numel() != n * h * w:
        raise VfiLibraryError("phasenet_emit_low_n_backward: gradient shape mismatch")
    if out is None:
        out = new((n, p_low, h, w), low_in)
    elif tuple(out.shape) != (n, p_low, h, w):
        raise VfiLibraryError(f"phasenet_emit_low_n_backward: out shape {tuple(out.shape)} != {(n, p_low, h, w)}")
    pp, ps = _slice_ptr(pred, "pred")
    lp, ls = _slice_ptr(low_in, "low_in")
    op, os_ = _slice_ptr(out, "out")
    _lib.call("vfi_phasenet_emit_low_n_backward", _lib.dptr(grad_low, "grad_low"), pp, ps, lp, ls, _lib.dptr(max_low, "max_low"),
              op, os_, n, h * w, num_img, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * h * w * (8 if num_img == 3 else 4), "phasenet_emit_low_n_backward"))
    return out


def phasenet_predict_n_backward(feat, pred, amp_in, max_amp, weight, num_img, grad_phase=None, grad_amp=None, grad_pred_in=None,
                                need_feat=True, need_weight=True, need_bias=True, out=None):
    """Adjoint of phasenet_predict_n in one pass (vfi_phasenet_predict_n_backward): phasenet_predict_backward's arguments and
    results with P = 12 predictions for three images (8 otherwise) and amp_in passed whole (N,4*num_img,H,W):
    -> (grad_feat (N,64,H,W), grad_weight (P,64,1,1), grad_bias (P,)), None where not needed."""
    p_band = phasenet_pred_channels(num_img)[1]
    n, cin, h, w = feat.shape
    if cin != 64 or tuple(pred.shape) != (n, p_band, h, w) or tuple(weight.shape) != (p_band, 64, 1, 1):
        raise VfiLibraryError(f"phasenet_predict_n_backward: feat (N,64,H,W), pred (N,{p_band},H,W), weight ({p_band},64,1,1)")
    if not (need_feat or need_weight or need_bias):
        raise VfiLibraryError("phasenet_predict_n_backward: no output asked for")
    for g, name in ((grad_phase, "grad_phase"), (grad_amp, "grad_amp")):
        if g is not None and g.numel() != n * 4 * h * w:
            raise VfiLibraryError(f"phasenet_predict_n_backward: {name} shape mismatch")
    if grad_pred_in is not None and tuple(grad_pred_in.shape) != (n, p_band, h, w):
        raise VfiLibraryError("phasenet_predict_n_backward: grad_pred_in shape mismatch")
    if grad_amp is not None and (tuple(amp_in.shape) != (n, 4 * num_img, h, w) or max_amp.numel() != n):
        raise VfiLibraryError(f"phasenet_predict_n_backward: amp_in must be (N,{4 * num_img},H,W), max_amp (N,)")
    fp, fs = _slice_ptr(feat, "feat")
    pp, ps = _slice_ptr(pred, "pred")
    ap, as_ = (None, 0) if grad_amp is None else _slice_ptr(amp_in, "amp_in")
    ip, is_ = (None, 0) if grad_pred_in is None else _slice_ptr(grad_pred_in, "grad_pred_in")
    gf = None
    if need_feat:
        gf = new((n, 64, h, w), feat) if out is None else out
        if tuple(gf.shape) != (n, 64, h, w):
            raise VfiLibraryError(f"phasenet_predict_n_backward: out shape {tuple(gf.shape)} != {(n, 64, h, w)}")
    gp, gs = (None, 0) if gf is None else _slice_ptr(gf, "out")
    gw = new((p_band, 64, 1, 1), feat) if need_weight else None
    gb = new((p_band,), feat) if need_bias else None
    floats = _lib.PHASENET_HEAD_N_WORKSPACE_FLOATS if num_img == 3 else _lib.PHASENET_HEAD_WORKSPACE_FLOATS
    ws = torch.empty(floats, dtype=torch.float32, device=feat.device) if need_weight or need_bias else None
    planes = p_band + 64 * (need_weight or need_bias) + 64 * need_feat + 4 * (grad_phase is not None) + \
        (4 + (20 if num_img == 3 else 8)) * (grad_amp is not None) + p_band * (grad_pred_in is not None)
    _lib.call("vfi_phasenet_predict_n_backward", fp, fs, pp, ps, ap, as_, _lib.dptr(max_amp, "max_amp") if grad_amp is not None else None,
              _lib.dptr(weight.detach(), "weight"), _lib.dptr(grad_phase, "grad_phase"), _lib.dptr(grad_amp, "grad_amp"), ip, is_,
              gp, gs, _lib.dptr(gw), _lib.dptr(gb), _lib.dptr(ws), n, h * w, num_img, _lib.stream_ptr(),
              work=_prof("byte", 4.0 * n * h * w * planes, "phasenet_predict_n_backward"))
    return gf, gw, gb


def l1_forward(a, b, wrap=False, scale=1.0):
    """scale * mean |w(a - b)| -> 0-dim tensor; w = atan2(sin, cos) when wrap (the phase loss), else the identity."""
    if a.numel() != b.numel():
        raise VfiLibraryError("l1_forward: shape mismatch")
    out = new((1,), a)
    _lib.call("vfi_l1_forward", _lib.dptr(a, "a"), _lib.dptr(b, "b"), a.numel(), int(bool(wrap)), float(scale),
              _reduce_workspace(a).data_ptr(), out.data_ptr(), _lib.stream_ptr(),
              work=_prof("byte", 8.0 * a.numel(), "l1_forward"))
    return out[0]


def l1_backward(a, b, upstream, wrap=False, scale=1.0, need_a=True, need_b=True):
    ga = torch.empty_like(a) if need_a else None
    gb = torch.empty_like(b) if need_b else None
    _lib.call("vfi_l1_backward", _lib.dptr(a, "a"), _lib.dptr(b, "b"), _lib.dptr(upstream.reshape(1), "upstream"),
              _lib.dptr(ga), _lib.dptr(gb), a.numel(), int(bool(wrap)), float(scale), _lib.stream_ptr(),
              work=_prof("byte", 4.0 * a.numel() * (2 + need_a + need_b), "l1_backward"))
    return ga, gb


def _out_like(x, out, name):
    """`out`: None (a new tensor) or a contiguous tensor of x's shape the op writes into (a slice of a wider buffer: no
    concat copy afterwards)."""
    if out is None:
        return torch.empty_like(x)
    if tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != x.device:
        raise VfiLibraryError(f"{name}: out must be a contiguous float32 tensor of shape {tuple(x.shape)} on {x.device}")
    return out


def rgb2lab(rgb, out=None):
    """(N,3,H,W) or (3,H,W) rgb in [0,1] -> scaled Lab, same shape (reference src/train/transform.py:17-25)."""
    x = rgb.contiguous()
    hw = x.shape[-1] * x.shape[-2]
    out = _out_like(x, out, "rgb2lab")
    _lib.call("vfi_rgb2lab", _lib.dptr(x, "rgb"), out.data_ptr(), x.numel() // (3 * hw), hw, _lib.stream_ptr())
    return out


def lab2rgb(lab):
    x = lab.contiguous()
    hw = x.shape[-1] * x.shape[-2]
    out = torch.empty_like(x)
    _lib.call("vfi_lab2rgb", _lib.dptr(x, "lab"), out.data_ptr(), x.numel() // (3 * hw), hw, _lib.stream_ptr())
    return out


def channel_mean_diff(a, b=None, scale=1.0, clamp01=False, signed=False):
    """a, b (N,C,H,W) -> (N,H,W): mean over C of a (minus that of b; abs unless signed), * scale, optional clamp."""
    a = a.contiguous()
    n, c, h, w = a.shape
    out = torch.empty((n, h, w), dtype=torch.float32, device=a.device)
    _lib.call("vfi_channel_mean_diff", _lib.dptr(a, "a"), _lib.dptr(b.contiguous(), "b") if b is not None else None,
              out.data_ptr(), n, c, h * w, float(scale), int(bool(clamp01)) | (2 if signed else 0), _lib.stream_ptr())
    return out


def absdiff(x, y, scale=1.0, clamp01=False, out=None):
    """|x - y| * scale, or |x| * scale for y=None (no zero tensor is built to subtract)."""
    x = x.contiguous()
    if y is not None:
        y = y.contiguous()
        if x.shape != y.shape:
            raise VfiLibraryError("absdiff: shape mismatch")
    out = _out_like(x, out, "absdiff")
    _lib.call("vfi_absdiff", _lib.dptr(x, "x"), _lib.dptr(y, "y") if y is not None else None, out.data_ptr(), x.numel(),
              float(scale), int(bool(clamp01)), _lib.stream_ptr())
    return out


def gaussian_filter(x, sigma, truncate=4.0, out=None):
    """scipy.ndimage.gaussian_filter per (H,W) image of x (N,H,W)."""
    x = x.contiguous()
    n, h, w = x.shape
    tmp, out = torch.empty_like(x), _out_like(x, out, "gaussian_filter")
    _lib.call("vfi_gaussian_filter", _lib.dptr(x, "x"), tmp.data_ptr(), out.data_ptr(), n, h, w, float(sigma),
              float(truncate), _lib.stream_ptr())
    return out


def median_filter(x, size):
    """scipy.ndimage.median_filter(size=size) per (H,W) image of x (N,H,W)."""
    x = x.contiguous()
    n, h, w = x.shape
    out = torch.empty_like(x)
    _lib.call("vfi_median_filter", _lib.dptr(x, "x"), out.data_ptr(), n, h, w, int(size), _lib.stream_ptr())
    return out


def _triplet_out(t, name, b, h, w, device, who="triplet_batch_prepare"):
    """(address, slot stride, sample stride) of an output of triplet_batch_prepare: (3, B, 3, h, w), or (3, 3B, h, w) for the
    same layout with dense samples; the (3, h, w) block of a sample is dense, the two outer strides are free."""
    if t is None:
        return None, 0, 0
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.device != device:
        raise VfiLibraryError(f"{who}: {name} must be a float32 tensor on {device}")
    _lib.check_device(t, name)
    if t.dim() == 4 and tuple(t.shape) == (3, 3 * b, h, w):
        t = t.unflatten(1, (b, 3))
    if t.dim() != 5 or tuple(t.shape) != (3, b, 3, h, w):
        raise VfiLibraryError(f"{who}: {name} must be (3, {b}, 3, {h}, {w}) or (3, {3 * b}, {h}, {w}), "
                              f"got {tuple(t.shape)}")
    s0, s1, sc, sh, sw = t.stride()
    if not ((sw == 1 or w == 1) and (sh == w or h == 1) and sc == h * w):
        raise VfiLibraryError(f"{who}: {name}: a sample's (3,h,w) block must be dense, strides {t.stride()}")
    return t.data_ptr(), s0, (s1 if b > 1 else 3 * h * w)


def triplet_batch_prepare(src, params, size, rgb=True, lab=True):
    """One training batch from decoded frames (vfi_triplet_batch_prepare; reference src/train/datareader.py:45-69 and
    src/train/trainer.py:115-121, :103).
    src: uint8 (B, 3, Hs, Ws, 3) on the device: im1, im2, im3 of each sample, HWC.  params: int32 (B, 3) ON THE HOST =
    (crop row, crop column, flags: 1 hflip | 2 vflip | 4 temporal swap).  size = (h, w) of the crop.
    rgb / lab: True = a new tensor, None / False = not wanted, or a float32 tensor to write into (a slice of a wider buffer).
    -> (rgb (3, B, 3, h, w) = [first, last, middle frame] / 255, lab (3, 3B, h, w) = preprocess of each slot), None where
    not wanted."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise VfiLibraryError("triplet_batch_prepare: src must be a tensor on a HIP device (vfi_amd has no CPU path)")
    if src.dtype != torch.uint8 or src.dim() != 5 or src.shape[1] != 3 or src.shape[4] != 3:
        raise VfiLibraryError(f"triplet_batch_prepare: src must be uint8 (B, 3, Hs, Ws, 3), got {src.dtype} {tuple(src.shape)}")
    b, _, hs, ws, _ = src.shape
    h, w = int(size[0]), int(size[1])
    params = torch.as_tensor(params)
    if params.is_cuda or params.dtype != torch.int32 or tuple(params.shape) != (b, 3):
        raise VfiLibraryError(f"triplet_batch_prepare: params must be a host int32 tensor of shape ({b}, 3)")
    params = params.contiguous()
    if h <= 0 or w <= 0:
        raise VfiLibraryError(f"triplet_batch_prepare: bad crop size {h}x{w}")
    if rgb is True:
        rgb = torch.empty((3, b, 3, h, w), dtype=torch.float32, device=src.device)
    elif rgb is False:
        rgb = None
    if lab is True:
        lab = torch.empty((3, 3 * b, h, w), dtype=torch.float32, device=src.device)
    elif lab is False:
        lab = None
    rp, rs, rb = _triplet_out(rgb, "rgb", b, h, w, src.device)
    lp, ls, lb = _triplet_out(lab, "lab", b, h, w, src.device)
    moved = 3 * b * h * w * (3 + 12 * (rgb is not None) + 12 * (lab is not None))
    _lib.call("vfi_triplet_batch_prepare", _lib.dptr(src, "src", torch.uint8), params.data_ptr(), rp, rs, rb, lp, ls, lb,
              b, hs, ws, h, w, _lib.stream_ptr(), work=("byte", float(moved), "triplet_batch_prepare"))
    return rgb, lab


def yuv_triplet_batch_prepare(src, fmt, params, size, source_size, rgb=True, lab=True):
    """One training batch from the Y'CbCr frames of a clip (vfi_yuv_triplet_batch_prepare): what triplet_batch_prepare makes
    of `yuv_to_rgb` of each whole frame, in one launch that decodes only the crops.
    src: uint8 (B, 3, frame_stride) on the device: the three frames of each sample in the Y4M frame layout, frame_stride >=
    the frame's bytes, any alignment.  fmt: see _yuv_format.  source_size = (Hs, Ws) of the frames.  params, size, rgb, lab
    and the result: as triplet_batch_prepare."""
    who = "yuv_triplet_batch_prepare"
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise VfiLibraryError(f"{who}: src must be a tensor on a HIP device (vfi_amd has no CPU path)")
    cfmt, sub = _yuv_format(fmt, who)
    hs, ws = int(source_size[0]), int(source_size[1])
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0 or hs <= 0 or ws <= 0:
        raise VfiLibraryError(f"{who}: bad sizes: crop {h}x{w} of {hs}x{ws}")
    if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[1] != 3:
        raise VfiLibraryError(f"{who}: src must be uint8 (B, 3, frame_stride), got {src.dtype} {tuple(src.shape)}")
    b, _, n = src.shape
    fs = src.stride(1)
    if n < yuv_frame_bytes(hs, ws, sub) or (src.stride(2) != 1 and n > 1) or fs < n or (b > 1 and src.stride(0) != 3 * fs):
        raise VfiLibraryError(f"{who}: src must hold frames of at least {yuv_frame_bytes(hs, ws, sub)} bytes for {hs}x{ws} at one "
                              f"stride, got shape {tuple(src.shape)} strides {src.stride()}")
    params = torch.as_tensor(params)
    if params.is_cuda or params.dtype != torch.int32 or tuple(params.shape) != (b, 3):
        raise VfiLibraryError(f"{who}: params must be a host int32 tensor of shape ({b}, 3)")
    params = params.contiguous()
    if rgb is True:
        rgb = torch.empty((3, b, 3, h, w), dtype=torch.float32, device=src.device)
    elif rgb is False:
        rgb = None
    if lab is True:
        lab = torch.empty((3, 3 * b, h, w), dtype=torch.float32, device=src.device)
    elif lab is False:
        lab = None
    rp, rs, rb = _triplet_out(rgb, "rgb", b, h, w, src.device, who)
    lp, ls, lb = _triplet_out(lab, "lab", b, h, w, src.device, who)
    _lib.check_device(src, "src")
    moved = 3 * b * h * w * ((1.5 if sub == YUV_420 else 3) + 12 * (rgb is not None) + 12 * (lab is not None))
    _lib.call("vfi_yuv_triplet_batch_prepare", src.data_ptr(), fs, ctypes.addressof(cfmt), params.data_ptr(), rp, rs, rb,
              lp, ls, lb, b, hs, ws, h, w, _lib.stream_ptr(), work=("byte", float(moved), who))
    return rgb, lab


YUV_420, YUV_444 = 0, 1                       # VFI_YUV_*: subsampling
YUV_SITING_CENTRE, YUV_SITING_LEFT = 0, 1     # horizontal chroma siting
YUV_BT709, YUV_BT601 = 0, 1                   # matrix
YUV_LIMITED, YUV_FULL = 0, 1                  # range


def yuv_frame_bytes(h, w, subsampling):
    """Bytes of one frame: H * W luma, then two chroma planes."""
    return h * w + 2 * ((h // 2) * (w // 2) if subsampling == YUV_420 else h * w)


def _yuv_format(fmt, name):
    """(ctypes int[4], subsampling) of a format: four integers (subsampling, siting, matrix, range), or an object whose
    `.yuv` holds them (fusion_net.y4m.Y4MFormat).  The library checks the values."""
    fmt = getattr(fmt, "yuv", fmt)
    try:
        vals = [int(v) for v in fmt]
    except (TypeError, ValueError):
        vals = None
    if vals is None or len(vals) != 4:
        raise VfiLibraryError(f"{name}: fmt must be four integers (subsampling, siting, matrix, range), got {fmt!r}")
    return (ctypes.c_int * 4)(*vals), vals[0]


def _yuv_frame(t, name, h, w, sub):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise VfiLibraryError(f"{name}: frame must be a tensor on a HIP device (vfi_amd has no CPU path)")
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != yuv_frame_bytes(h, w, sub):
        raise VfiLibraryError(f"{name}: frame must be dense uint8 with {yuv_frame_bytes(h, w, sub)} bytes for {h}x{w}, "
                              f"got {t.dtype} {tuple(t.shape)}")
    _lib.check_device(t, "frame")
    return t.data_ptr()


def _yuv_out(t, name, h, w, device):
    """True = a new (3, h, w) tensor, None / False = not wanted, or a contiguous float32 (3, h, w) tensor to write into."""
    if t is None or t is False:
        return None
    if t is True:
        return torch.empty((3, h, w), dtype=torch.float32, device=device)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.device != device \
            or tuple(t.shape) != (3, h, w) or not t.is_contiguous():
        raise VfiLibraryError(f"yuv_to_rgb: {name} must be a contiguous float32 tensor of shape (3, {h}, {w}) on {device}")
    return t


def yuv_to_rgb(frame, h, w, fmt, rgb=None, lab=(None, None)):
    """One planar 8-bit Y'CbCr frame -> rgb in [0, 1] and its scaled Lab (vfi_yuv_to_rgb), in one launch on the current stream.
    frame: dense uint8 on the device, any alignment, Y then Cb then Cr.  fmt: see _yuv_format.
    rgb, lab[0], lab[1]: True = a new tensor, None / False = not wanted, or a (3, h, w) float32 tensor to write into (a
    slice of a (6, h, w) Lab buffer); both Lab destinations get the same bits.  At least one must be wanted.
    -> (rgb, lab[0], lab[1]), None where not wanted."""
    h, w = int(h), int(w)
    cfmt, sub = _yuv_format(fmt, "yuv_to_rgb")
    if h <= 0 or w <= 0:
        raise VfiLibraryError(f"yuv_to_rgb: bad size {h}x{w}")
    fp = _yuv_frame(frame, "yuv_to_rgb", h, w, sub)
    lab_a, lab_b = lab
    rgb = _yuv_out(rgb, "rgb", h, w, frame.device)
    lab_a, lab_b = _yuv_out(lab_a, "lab[0]", h, w, frame.device), _yuv_out(lab_b, "lab[1]", h, w, frame.device)
    outs = [t.data_ptr() if t is not None else None for t in (rgb, lab_a, lab_b)]
    moved = frame.numel() + 12 * h * w * sum(t is not None for t in (rgb, lab_a, lab_b))
    _lib.call("vfi_yuv_to_rgb", fp, h, w, ctypes.addressof(cfmt), *outs, _lib.stream_ptr(),
              work=("byte", float(moved), "yuv_to_rgb"))
    return rgb, lab_a, lab_b


def rgb_to_yuv(rgb, fmt, out=None):
    """(3, H, W) float32 rgb (clamped to [0, 1] by the kernel) -> one planar 8-bit Y'CbCr frame (vfi_rgb_to_yuv), in one launch
    on the current stream.  out: None (a new tensor) or a dense uint8 device tensor of the frame's size, any alignment."""
    cfmt, sub = _yuv_format(fmt, "rgb_to_yuv")
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda:
        raise VfiLibraryError("rgb_to_yuv: rgb must be a tensor on a HIP device (vfi_amd has no CPU path)")
    if rgb.dim() != 3 or rgb.shape[0] != 3:
        raise VfiLibraryError(f"rgb_to_yuv: rgb must be (3, H, W), got {tuple(rgb.shape)}")
    h, w = rgb.shape[1:]
    if sub == YUV_420 and (h % 2 or w % 2):
        raise VfiLibraryError(f"rgb_to_yuv: 4:2:0 needs even sizes, got {h}x{w}")
    if out is None:
        out = torch.empty(yuv_frame_bytes(h, w, sub), dtype=torch.uint8, device=rgb.device)
    op = _yuv_frame(out, "rgb_to_yuv", h, w, sub)
    if out.device != rgb.device:
        raise VfiLibraryError(f"rgb_to_yuv: out is on {out.device}, rgb on {rgb.device}")
    _lib.call("vfi_rgb_to_yuv", _lib.dptr(rgb, "rgb"), h, w, ctypes.addressof(cfmt), op, _lib.stream_ptr(),
              work=("byte", float(12 * h * w + out.numel()), "rgb_to_yuv"))
    return out


def _scene_bytes(t, name, who, least):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise VfiLibraryError(f"{who}: {name} must be a tensor on a HIP device (vfi_amd has no CPU path)")
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < least:
        raise VfiLibraryError(f"{who}: {name} must be dense uint8 with at least {least} bytes, got {t.dtype} {tuple(t.shape)}")
    _lib.check_device(t, name)
    return t.data_ptr()


def _scene_word(t, name, who, dtype, device):
    """One device word of `dtype` (None -> NULL)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise VfiLibraryError(f"{who}: {name} must be a tensor on a HIP device (vfi_amd has no CPU path)")
    if t.dtype != dtype or t.numel() != 1 or t.device != device:
        raise VfiLibraryError(f"{who}: {name} must be one {dtype} element on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.data_ptr()


def luma_sad(frame_a, frame_b, n, out=None):
    """Sum of |a[i] - b[i]| over the first n bytes of two dense uint8 device tensors (vfi_luma_sad; two frames and n = H * W
    give the luma planes), exact, in launches on the current stream.  -> `out`, a one-element int64 device tensor (a new
    one for None; what it held before does not matter).  Nothing comes back to the host."""
    n = int(n)
    if n <= 0:
        raise VfiLibraryError(f"luma_sad: bad size {n}")
    pa, pb = _scene_bytes(frame_a, "frame_a", "luma_sad", n), _scene_bytes(frame_b, "frame_b", "luma_sad", n)
    if frame_a.device != frame_b.device:
        raise VfiLibraryError(f"luma_sad: frame_a is on {frame_a.device}, frame_b on {frame_b.device}")
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=frame_a.device)
    _lib.call("vfi_luma_sad", pa, pb, n, _scene_word(out, "out", "luma_sad", torch.int64, frame_a.device), _lib.stream_ptr(),
              work=("byte", float(2 * n), "luma_sad"))
    return out


def frame_pick(dst, src, sad, sad_prev, min_sad, cut=None):
    """Scene-cut decision and replacement on the device (vfi_frame_pick), one launch on the current stream: with
    p = sad_prev (0 for None) the pair is a cut when min(sad, |sad - p|) >= min_sad (fusion_net.scene.min_sad turns a
    threshold into it); on a cut dst's bytes become src's, otherwise dst is left alone.  dst, src: dense uint8 device
    tensors of one size; sad, sad_prev: one-element int64 device tensors as luma_sad returns them; cut: a one-element int32
    device tensor that receives 1 or 0, or None.  -> cut."""
    min_sad = int(min_sad)
    if not 0 <= min_sad < 1 << 64:
        raise VfiLibraryError(f"frame_pick: min_sad {min_sad} is not an unsigned 64-bit value")
    pd = _scene_bytes(dst, "dst", "frame_pick", 1)
    ps = _scene_bytes(src, "src", "frame_pick", dst.numel())
    if src.numel() != dst.numel() or src.device != dst.device:
        raise VfiLibraryError(f"frame_pick: src must have dst's {dst.numel()} bytes on {dst.device}, "
                              f"got {src.numel()} on {src.device}")
    if sad is None:
        raise VfiLibraryError("frame_pick: sad must be a one-element int64 device tensor")
    words = [_scene_word(sad, "sad", "frame_pick", torch.int64, dst.device),
             _scene_word(sad_prev, "sad_prev", "frame_pick", torch.int64, dst.device)]
    _lib.call("vfi_frame_pick", pd, ps, dst.numel(), *words, min_sad, _scene_word(cut, "cut", "frame_pick", torch.int32, dst.device),
              _lib.stream_ptr(), work=("byte", float(2 * dst.numel()), "frame_pick"))
    return cut


def optim_limits():
    """(elements per chunk, tensors per launch, chunks per launch, largest numel) of vfi_optim_step; needs no device."""
    c, m = ctypes.c_longlong(), ctypes.c_longlong()
    t, k = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().vfi_optim_limits(ctypes.byref(c), ctypes.byref(t), ctypes.byref(k), ctypes.byref(m)),
               "vfi_optim_limits")
    return c.value, t.value, k.value, m.value


def optim_step(kind, params, grads, state0=None, state1=None, *, lr, betas=(0.0, 0.0), alpha=0.0, eps=0.0, weight_decay=0.0,
               momentum=0.0, dampening=0.0, nesterov=False, first_step=False, step=1, clamp=None):
    """One optimiser update of the tensors `params`, which share these hyper-parameters and the step count `step` (the count
    AFTER this update, 1 for the first): kind in sgd | adam | adamax | rmsprop; include/vfi_hip.h gives the formulas and
    which state goes where.  params, grads, state0, state1: equally long lists of contiguous float32 tensors on the current
    HIP device (a state list may be None where the kind keeps no such state).  Everything is written in place through raw
    pointers, so no version counter moves: vfi_amd.optim bumps them."""
    n = len(params)
    if n == 0:
        return
    dev, f32 = torch.cuda.current_device(), torch.float32
    lists = [("param", params), ("grad", grads)] + [(nm, s) for nm, s in (("state0", state0), ("state1", state1)) if s is not None]
    recs = (_lib.OptimTensor * n)()
    total = 0
    for name, tensors in lists:
        if len(tensors) != n:
            raise VfiLibraryError(f"optim_step: {len(tensors)} {name} tensors for {n} params")
        for i, t in enumerate(tensors):
            if not (t.is_cuda and t.device.index == dev and t.dtype is f32 and t.is_contiguous()
                    and t.numel() == params[i].numel()):
                raise VfiLibraryError(f"optim_step: {name} {i} must be a contiguous float32 tensor of its param's size on "
                                      f"cuda:{dev} (vfi_amd has no CPU path)")
            setattr(recs[i], name, t.data_ptr())
    for i, p in enumerate(params):
        recs[i].numel = p.numel()
        total += recs[i].numel
    step = float(step)
    h = _lib.OptimHyper(lr=lr, beta1=betas[0], beta2=betas[1], alpha=alpha, eps=eps, weight_decay=weight_decay,
                        momentum=momentum, dampening=dampening, bias_correction1=1 - betas[0] ** step,
                        bias_correction2=1 - betas[1] ** step, nesterov=int(nesterov), first_step=int(first_step))
    if clamp is not None:
        h.clamp_min, h.clamp_max, h.has_clamp = float(clamp[0]), float(clamp[1]), 1
    _lib.call("vfi_optim_step", _lib.OPTIM_KINDS[kind], ctypes.addressof(recs), n, ctypes.addressof(h), _lib.stream_ptr(),
              work=("byte", 4.0 * (2 * len(lists) - 1) * total, "optim_" + kind))
