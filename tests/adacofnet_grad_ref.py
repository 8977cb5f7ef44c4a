"""References for the AdaCoF network's HIP backward.

1. float64 host models of the glue adjoints, written the way the kernels of csrc/vfi_adacofnet_grad.hip compute them
   (gather forms, explicit stencils), checked against torch autograd by tests/test_adacofnet_grad_host.py.
2. `training_dict`: a differentiable torch restatement of AdaCoFNet.forward's training branch (reference
   src/adacof/models/adacofnet.py:170-217) from oracle.nets_cpu's layers and adacof_grad_ref.adacof_restated, with the
   piecewise decisions (ReLU masks) optionally pinned to recorded ones.
"""
import numpy as np
import torch
import torch.nn.functional as F

from adacof_grad_ref import adacof_restated
from oracle import nets_cpu

EPS = 0.001
HEADS = ("moduleWeight1", "moduleAlpha1", "moduleBeta1", "moduleWeight2", "moduleAlpha2", "moduleBeta2", "moduleOcclusion")


# ---- 1. host models -----------------------------------------------------------------------------------------------
def up2ac_sources(j, n):
    """(output index, weight) pairs of one axis of Upsample(x2, bilinear, align_corners=True) reading source j of n
    (up2ac_sources in the kernel): output o sits at o (n-1)/(2n-1), exact in integers here."""
    if n == 1:
        return [(0, 1.0), (1, 1.0)]
    den, out = 2 * n - 1, []
    for o in range(2 * n):
        i0, r = divmod(o * (n - 1), den)
        i0 = min(i0, n - 1)
        i1, l = min(i0 + 1, n - 1), r / den
        w = (1.0 - l if i0 == j else 0.0) + (l if i1 == j else 0.0)
        if w != 0.0:
            out.append((o, w))
    return out


def up2ac_adjoint(g, mask_src=None):
    n, c, ho, wo = g.shape
    h, w = ho // 2, wo // 2
    out = np.zeros((n, c, h, w))
    for y in range(h):
        for x in range(w):
            for oy, wy in up2ac_sources(y, h):
                for ox, wx in up2ac_sources(x, w):
                    out[:, :, y, x] += wy * wx * g[:, :, oy, ox]
    return out * (mask_src > 0) if mask_src is not None else out


def avgpool_backward(y, gp, gskip=None):
    g = 0.25 * np.repeat(np.repeat(gp, 2, axis=2), 2, axis=3)
    if gskip is not None:
        g = g + gskip
    return g * (y > 0)


def softmax_backward(w, gw):
    return w * (gw - (w * gw).sum(1, keepdims=True))


def charb_stencil(m):
    """d/dm of mean_h sqrt((m[x]-m[x+1])^2 + e^2) + mean_v sqrt((m[y]-m[y+1])^2 + e^2) over an (N, 1, H, W) map: per pixel
    the <= 4 neighbour terms, each over its direction's element count (charb_stencil in the kernel)."""
    n, _, h, w = m.shape
    q = np.zeros_like(m)
    dh = m[..., :, :-1] - m[..., :, 1:]
    th = dh / np.sqrt(dh * dh + EPS * EPS) / (n * h * (w - 1))
    q[..., :, :-1] += th
    q[..., :, 1:] -= th
    dv = m[..., :-1, :] - m[..., 1:, :]
    tv = dv / np.sqrt(dv * dv + EPS * EPS) / (n * (h - 1) * w)
    q[..., :-1, :] += tv
    q[..., 1:, :] -= tv
    return q


def charb_term(m):
    dh = m[..., :, :-1] - m[..., :, 1:]
    dv = m[..., :-1, :] - m[..., 1:, :]
    return np.sqrt(dh * dh + EPS * EPS).mean() + np.sqrt(dv * dv + EPS * EPS).mean()


def smooth_forward(w1, a1, b1, w2, a2, b2, occ):
    """-> (m (N,4,H,W) = [m_Alpha1, m_Beta1, m_Alpha2, m_Beta2], g_Spatial, g_Occlusion)."""
    m = np.stack([(w1 * a1).mean(1), (w1 * b1).mean(1), (w2 * a2).mean(1), (w2 * b2).mean(1)], 1)
    return m, sum(charb_term(m[:, i:i + 1]) for i in range(4)), charb_term(occ)


def head_backward(gw, ga, gb, w, a, b, m_a, m_b, up_spatial):
    """(grad_logit, grad_alpha, grad_beta) of one side (head_backward_kernel)."""
    f2 = w.shape[1]
    qa, qb = up_spatial * charb_stencil(m_a) / f2, up_spatial * charb_stencil(m_b) / f2
    return softmax_backward(w, gw + qa * a + qb * b), ga + qa * w, gb + qb * w


def blend_backward(g, t1, t2, occ, up_occ):
    """(grad_t1, grad_t2, grad_z); g is (N, C, h0, w0) with h0 <= H, w0 <= W (zero outside the crop)."""
    ge = np.zeros_like(t1)
    ge[:, :, :g.shape[2], :g.shape[3]] = g
    go = (ge * (t1 - t2)).sum(1, keepdims=True) + up_occ * charb_stencil(occ)
    return ge * occ, ge * (1 - occ), go * occ * (1 - occ)


# ---- 2. the training branch restated ------------------------------------------------------------------------------
def charbonnier(d):
    return torch.sqrt(d ** 2 + EPS ** 2).mean()


def smoothness(w1, a1, b1, w2, a2, b2, occ):
    """(g_Spatial, g_Occlusion) of adacofnet.py:204-215 in torch (differentiable)."""
    term = lambda m: charbonnier(m[:, :, :, :-1] - m[:, :, :, 1:]) + charbonnier(m[:, :, :-1, :] - m[:, :, 1:, :])
    mean = lambda w, x: (w * x).mean(1, keepdim=True)
    return term(mean(w1, a1)) + term(mean(w1, b1)) + term(mean(w2, a2)) + term(mean(w2, b2)), term(occ)


def kernel_estimation(sd, x6, masks=None, record=None, prefix="get_kernel."):
    """oracle.nets_cpu.kernel_estimation layer by layer -> the seven maps.  `masks` {layer name: bool tensor} replaces every
    ReLU by a multiplication with the recorded mask; `record` (a dict) receives relu outputs' masks of this run."""
    P = lambda n: prefix + n

    def conv_relu(name, x):
        z = nets_cpu._conv(sd, P(name), x, 1)
        if masks is not None:
            return z * masks[name]
        y = F.relu(z)
        if record is not None:
            record[name] = y > 0
        return y

    def basic(name, x):
        for i in (0, 2, 4):
            x = conv_relu(f"{name}.{i}", x)
        return x

    c1 = basic("moduleConv1", x6)
    c2 = basic("moduleConv2", F.avg_pool2d(c1, 2, 2))
    c3 = basic("moduleConv3", F.avg_pool2d(c2, 2, 2))
    c4 = basic("moduleConv4", F.avg_pool2d(c3, 2, 2))
    c5 = basic("moduleConv5", F.avg_pool2d(c4, 2, 2))
    x = basic("moduleDeconv5", F.avg_pool2d(c5, 2, 2))
    x = conv_relu("moduleUpsample5.1", nets_cpu._up2(x)) + c5
    x = conv_relu("moduleUpsample4.1", nets_cpu._up2(basic("moduleDeconv4", x))) + c4
    x = conv_relu("moduleUpsample3.1", nets_cpu._up2(basic("moduleDeconv3", x))) + c3
    x = conv_relu("moduleUpsample2.1", nets_cpu._up2(basic("moduleDeconv2", x))) + c2
    outs = []
    for h in HEADS:
        t = basic(h, x)
        t = nets_cpu._conv(sd, P(f"{h}.7"), nets_cpu._up2(t), 1)
        outs.append(torch.softmax(t, 1) if h.startswith("moduleWeight") else (torch.sigmoid(t) if h == "moduleOcclusion" else t))
    return tuple(outs)


def training_dict(sd, frame0, frame2, kernel_size=5, dilation=1, masks=None, record=None, offsets=None):
    """adacofnet.py:170-217 in torch, dtype of `sd`.  `offsets`: (a1, b1, a2, b2) recorded tensors whose truncated integer
    cells replace the restatement's own (the sampler's piecewise decision): alpha is then sampled as
    trunc(recorded) + (alpha - trunc(recorded)), which adacof_restated's `A` would only equal when both truncate alike."""
    h0, w0 = frame0.shape[2:]
    ph, pw = (32 - h0 % 32) % 32, (32 - w0 % 32) % 32
    if ph:
        frame0, frame2 = (F.pad(f, (0, 0, 0, ph), mode="reflect") for f in (frame0, frame2))
    if pw:
        frame0, frame2 = (F.pad(f, (0, pw, 0, 0), mode="reflect") for f in (frame0, frame2))
    mean = torch.tensor(nets_cpu.CHANNEL_MEANS, dtype=frame0.dtype).view(1, 3, 1, 1)
    x6 = torch.cat([frame0 - mean, frame2 - mean], 1)
    w1, a1, b1, w2, a2, b2, occ = kernel_estimation(sd, x6, masks, record)
    pad = int(((kernel_size - 1) * dilation) / 2.0)
    rp = lambda x: F.pad(x, (pad,) * 4, mode="replicate")
    sample = (lambda fr, w, a, b, d, side: adacof_restated(fr, w, a, b, d)) if offsets is None else _pinned_sampler(offsets)
    t1 = sample(rp(frame0), w1, a1, b1, dilation, 0)
    t2 = sample(rp(frame2), w2, a2, b2, dilation, 1)
    frame1 = (occ * t1 + (1 - occ) * t2)[:, :, :h0, :w0]
    g_spatial, g_occlusion = smoothness(w1, a1, b1, w2, a2, b2, occ)
    return {"frame1": frame1, "g_Spatial": g_spatial, "g_Occlusion": g_occlusion}, (w1, a1, b1, w2, a2, b2, occ)


def _pinned_sampler(offsets):
    """adacof_restated with the integer cells taken from recorded fp32 offsets: the offset handed on is
    cell + (alpha - cell) evaluated so that trunc() inside adacof_restated returns the recorded cell."""
    def sample(frame, w, a, b, dilation, side):
        ra, rb = offsets[2 * side].to(a.dtype), offsets[2 * side + 1].to(a.dtype)
        return _restated_with_cells(frame, w, a, b, ra.trunc(), rb.trunc(), dilation)
    return sample


def _restated_with_cells(input, weight, offset_i, offset_j, cell_i, cell_j, dilation):
    """adacof_grad_ref.adacof_restated with A = cell_i, B = cell_j given instead of trunc(offset)."""
    n, c, hin, win = input.shape
    ff, h, w = weight.shape[1:]
    f = int(round(ff ** 0.5))
    rows = torch.arange(h).view(1, h, 1)
    cols = torch.arange(w).view(1, 1, w)
    flat = input.reshape(n, c, hin * win)
    out = input.new_zeros((n, c, h, w))
    for k in range(f):
        for l in range(f):
            t = k * f + l
            A, B = cell_i[:, t], cell_j[:, t]
            fa, fb = offset_i[:, t] - A, offset_j[:, t] - B
            r = rows + k * dilation + A.long()
            q = cols + l * dilation + B.long()
            i0, i1 = r.clamp(0, hin - 1), (r + 1).clamp(0, hin - 1)
            j0, j1 = q.clamp(0, win - 1), (q + 1).clamp(0, win - 1)

            def gather(i, j):
                idx = (i * win + j).reshape(n, 1, h * w).expand(n, c, h * w)
                return flat.gather(2, idx).reshape(n, c, h, w)

            ga, gb = (1 - fa).unsqueeze(1), (1 - fb).unsqueeze(1)
            fa, fb = fa.unsqueeze(1), fb.unsqueeze(1)
            v = gather(i0, j0) * ga * gb + gather(i1, j0) * fa * gb + gather(i0, j1) * ga * fb + gather(i1, j1) * fa * fb
            out = out + weight[:, t].unsqueeze(1) * v
    return out
