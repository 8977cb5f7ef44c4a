"""Float64 statement of the fused AdaCoF operator (reference src/fusion_net/fusion_adacofnet.py:195-213 with the sampling of
src/adacof/cupy_module/adacof.py:6-65), the case table every instantiation of `adacof_fused_kernel` is tested on, and the
runner that tests/test_adacof_fused_gpu.py and tools/check_adacof_fused.py share.

The reference is NumPy, vectorised over pixels (the only Python loop is over the F*F taps).  It takes the fp32 inputs the
kernel takes and chooses the kernel's corners: A = trunc(alpha), B = trunc(beta) toward zero on the fp32 value, each of the
four corner indices clamped on its own (the replication pad of (F-1)*dilation/2 is that clamp), the fractions alpha - A and
beta - B left un-clamped (they may be negative: the bilinear weights extrapolate).  Everything after the corner choice is
float64, so what a kernel differs from it by is the kernel's own fp32 rounding.

Which (F, dilation) reaches which instantiation (host dispatch: `adacof_fused_impl`, csrc/vfi_adacof.hip).  An rgbx call takes a
`WIN` kernel (tile neighbourhood staged in LDS) when two windows of wh x ww 16-byte pixels fit 64 KiB,
    wh = 4 + e + 2*margin + 1,  ww = 64 + e + 2*margin + 1,  e = (F-1)*dilation,  margin = 4 (VFI_ADACOF_MARGIN),
that is (13 + e) * (73 + e) <= 2048, which holds up to e = 10 (23 * 83 = 1909) and fails from e = 12 (25 * 85 = 2125); e is
even.  F == 5 selects the compile-time-F kernels (FT = 5), any other F the run-time-F ones (FT = 0); `weights_are_logits`
selects SOFTMAX.  So, with the default environment:
    (5,1) e=4, (5,2) e=8      rgbx: WIN, FT=5 (+SOFTMAX: the production kernel)     planar: VEC=1, FT=5
    (3,2) e=4, (7,1) e=6      rgbx: WIN, FT=0 (+SOFTMAX)                            planar: VEC=1, FT=0
    (5,3) e=12                rgbx: non-WIN, FT=5 (+SOFTMAX)                        planar: VEC=1, FT=5
    (7,2) e=12, (11,2) e=20   rgbx: non-WIN, FT=0 (+SOFTMAX)                        planar: VEC=1, FT=0
VFI_ADACOF_MARGIN=0 sends every rgbx call to the non-WIN kernels.  VFI_ADACOF_VARIANT=0 gives the planar call VEC=4 where
W % 4 == 0 (widths 64, 260), VEC=2 where W % 2 == 0 (width 70) and VEC=1 otherwise (129); VFI_ADACOF_VARIANT=1 gives VEC=2
for every even width.  Both switches are read once per process, hence tools/check_adacof_fused.py in a child process.
"""
import collections
import functools
import zlib

import numpy as np

# tests/test_adacof_gpu.py's bounds (fp32 kernel: precomputed bilinear weights, fma contraction)
IMAGE_ATOL = 2e-5
MASK_RTOL, MASK_ATOL = 1e-4, 2e-5
MASK_RTOL_FAR = 1e-3      # offsets of ~100 px with a spread of 0.5: the variance is a 1e-5 fraction of the second moment

MODES = ("planar", "rgbx", "rgbx_logits")


# ---- the operator in float64 ----------------------------------------------------------------------------------------------
def sample_side(frame, weight, alpha, beta, dilation, padded=False):
    """One sampling side, float64 (N,C,H,W).  frame (N,C,Hin,Win) fp32; weight / alpha / beta (N,F*F,H,W).

    padded=True: `frame` already carries the (F-1)*dilation border (FunctionAdaCoF.forward, adacof.py:326-327) and tap (k,l)
    of pixel (i,j) starts at (i + k*dilation, j + l*dilation).  padded=False: the frame is un-padded and the replication pad
    is the clamp: the tap starts (F-1)*dilation/2 further up and left."""
    n, c, hin, win = frame.shape
    _, k2, h, w = weight.shape
    f = int(round(np.sqrt(k2)))
    assert f * f == k2
    if padded:
        assert hin == h + (f - 1) * dilation and win == w + (f - 1) * dilation
        origin = 0
    else:
        assert (hin, win) == (h, w) and ((f - 1) * dilation) % 2 == 0
        origin = -((f - 1) * dilation // 2)
    frame = frame.astype(np.float64)
    weight = np.asarray(weight, dtype=np.float64)
    a32, b32 = np.asarray(alpha, dtype=np.float32), np.asarray(beta, dtype=np.float32)
    ta, tb = np.trunc(a32), np.trunc(b32)                       # (int)alpha: toward zero, on the fp32 value
    fa, fb = a32.astype(np.float64) - ta, b32.astype(np.float64) - tb
    ta, tb = ta.astype(np.int64), tb.astype(np.int64)
    nn = np.arange(n)[:, None, None]
    ii = np.arange(h)[None, :, None]
    jj = np.arange(w)[None, None, :]
    out = np.zeros((n, h, w, c), np.float64)
    for k in range(f):
        for l in range(f):
            t = k * f + l
            r = ii + k * dilation + origin + ta[:, t]
            q = jj + l * dilation + origin + tb[:, t]
            i0, i1 = np.clip(r, 0, hin - 1), np.clip(r + 1, 0, hin - 1)
            j0, j1 = np.clip(q, 0, win - 1), np.clip(q + 1, 0, win - 1)
            px = lambda i, j: frame[nn, :, i, j]                # (N,H,W,C)
            ga, gb = 1.0 - fa[:, t], 1.0 - fb[:, t]
            v = (px(i0, j0) * (ga * gb)[..., None] + px(i1, j0) * (fa[:, t] * gb)[..., None]
                 + px(i0, j1) * (ga * fb[:, t])[..., None] + px(i1, j1) * (fa[:, t] * fb[:, t])[..., None])
            out += weight[:, t][..., None] * v
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def softmax64(logits):
    z = np.asarray(logits, dtype=np.float64)
    z = np.exp(z - z.max(1, keepdims=True))
    return z / z.sum(1, keepdims=True)


def flow_variance(weight, alpha, beta):
    """sum over alpha and beta of sum_k W (Mean - x)^2, Mean = sum_k W x  (fusion_adacofnet.py:201-208); W need not sum to 1."""
    wgt = np.asarray(weight, dtype=np.float64)
    var = 0.0
    for x in (alpha, beta):
        x = np.asarray(x, dtype=np.float64)
        mean = (wgt * x).sum(1, keepdims=True)
        var = var + (wgt * (mean - x) ** 2).sum(1, keepdims=True)
    return var


def fused_ref(f0, f2, w1, a1, b1, w2, a2, b2, occ, dilation, weights_are_logits=False):
    """-> dict(t1, t2, frame (N,3,H,W), mask (N,1,H,W)), float64.  Frames planar and un-padded."""
    if weights_are_logits:
        w1, w2 = softmax64(w1), softmax64(w2)
    t1 = sample_side(f0, w1, a1, b1, dilation)
    t2 = sample_side(f2, w2, a2, b2, dilation)
    o = np.asarray(occ, dtype=np.float64)
    var = np.maximum(flow_variance(w1, a1, b1), flow_variance(w2, a2, b2))
    return dict(t1=t1, t2=t2, frame=o * t1 + (1.0 - o) * t2, mask=np.clip(var, 0.0, 20.0) / 20.0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
# Offset fields (both sides get the same kind):
#   gauss3    N(0, 3^2): the field of tests/test_adacof_gpu.py; the mask is mostly saturated
#   gauss1    N(0, 1): the mask is mostly strictly inside (0, 1) (asserted on the reference by the host test)
#   gauss02, gauss01   N(0, 0.2^2), N(0, 0.1^2): the same for weights that sum to ~F*F/2 (F <= 5, F = 7)
#   boundary  every tap's alpha and beta drawn independently from BOUNDARY_OFFSETS.  With margin 4, integer part -4 is the
#             first row / column inside the staged window for thread row 0 / tap row 0 and -5 the first one outside (the
#             fallback gathers); 4 and 5 are the same for the last thread row / last tap row; -0.5 truncates to 0 with a
#             negative fraction
#   edge      the same with EDGE_OFFSETS: the integer parts -5 / -4 and 4 / 5 again, each with a fraction that is not zero.  A tap
#             at 5.0 gives its second row and column the weight 0, so a membership test that lets integer part 5 into the
#             window (row WH: the other side's window, or LDS nobody staged) goes unnoticed on `boundary`; at 5.25 it does not
#   far       +-97.3 with a spread of 0.5: every tap leaves the window and clamps at the image border, and the mask depends on
#             the pivoted moments (surviving the softmax rescaling, in the logits mode)
# Weights: softmax (sum to 1), rand (uniform [0,1): sum to ~F*F/2; no logits mode), dominant (softmax in which one tap per
# pixel is ahead by 80 in the logit).
BOUNDARY_OFFSETS = (-5.0, -4.5, -4.0, -0.5, 0.0, 0.5, 4.0, 4.75, 5.0)
EDGE_OFFSETS = (-5.25, -4.25, -0.5, 0.5, 4.25, 5.25)

Case = collections.namedtuple("Case", "n h w f dil field weights")


def case_id(c):
    return f"f{c.f}d{c.dil}-{c.n}x{c.h}x{c.w}-{c.field}-{c.weights}"


def _c(f, dil, shape, field, weights="softmax"):
    n, h, w = shape if len(shape) == 3 else (1,) + tuple(shape)
    return Case(n, h, w, f, dil, field, weights)


# Shapes: (1,1) every corner clamps; (3,5) smaller than one 4x64 tile both ways; (9,70) H no multiple of 4 and a 6-pixel last
# tile column (idle threads still stage); (10,129) three tile columns, the last one pixel wide; (2,8,64) exact tiles and the
# batch offset of the float4 frame pointer; (6,260) a second width that is a multiple of 4 (two VEC=4 tile columns, the last
# one thread wide).
CASES = (
    # (5,1): WIN, FT=5 -- the production configuration
    _c(5, 1, (9, 70), "gauss3"), _c(5, 1, (9, 70), "gauss1"), _c(5, 1, (9, 70), "boundary"), _c(5, 1, (9, 70), "far"),
    _c(5, 1, (9, 70), "gauss1", "dominant"), _c(5, 1, (9, 70), "gauss3", "rand"), _c(5, 1, (9, 70), "gauss02", "rand"),
    _c(5, 1, (10, 129), "gauss3"), _c(5, 1, (10, 129), "boundary"), _c(5, 1, (1, 1), "gauss3"), _c(5, 1, (3, 5), "boundary"),
    _c(5, 1, (2, 8, 64), "gauss1"), _c(5, 1, (6, 260), "gauss3"), _c(5, 1, (9, 70), "edge"), _c(5, 1, (10, 129), "edge"),
    # (5,2): WIN, FT=5, e=8
    _c(5, 2, (9, 70), "boundary"), _c(5, 2, (9, 70), "gauss1"), _c(5, 2, (3, 5), "gauss3"),
    _c(5, 2, (9, 70), "edge"),
    # (3,2), (7,1): WIN, FT=0
    _c(3, 2, (9, 70), "boundary"), _c(3, 2, (9, 70), "gauss1"), _c(3, 2, (9, 70), "gauss02", "rand"),
    _c(3, 2, (2, 8, 64), "gauss3"), _c(3, 2, (6, 260), "boundary"), _c(3, 2, (9, 70), "far"),
    _c(7, 1, (9, 70), "boundary"), _c(7, 1, (10, 129), "gauss3"), _c(7, 1, (1, 1), "gauss3"),
    _c(7, 1, (9, 70), "gauss1", "dominant"), _c(3, 2, (9, 70), "edge"), _c(7, 1, (9, 70), "edge"),
    # (5,3): non-WIN, FT=5
    _c(5, 3, (9, 70), "boundary"), _c(5, 3, (9, 70), "gauss3"), _c(5, 3, (10, 129), "gauss1"), _c(5, 3, (2, 8, 64), "far"),
    _c(5, 3, (9, 70), "gauss02", "rand"),
    # (7,2), (11,2): non-WIN, FT=0
    _c(7, 2, (9, 70), "boundary"), _c(7, 2, (3, 5), "gauss3"), _c(7, 2, (9, 70), "gauss01", "rand"),
    _c(11, 2, (9, 70), "gauss3"), _c(11, 2, (9, 70), "far"), _c(11, 2, (2, 10, 129), "boundary"),
)
assert len({case_id(c) for c in CASES}) == len(CASES)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 arrays f0, f2 (planar), w1, a1, b1, w2, a2, b2, occ, and lg1, lg2 (logits whose softmax is w1 / w2; None for
    rand weights)."""
    n, h, w, f, _, field, weights = case
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    k = f * f
    d = dict(f0=rng.random((n, 3, h, w), dtype=np.float32), f2=rng.random((n, 3, h, w), dtype=np.float32),
             occ=rng.random((n, 1, h, w), dtype=np.float32))
    for side in "12":
        if weights == "rand":
            d["w" + side], d["lg" + side] = rng.random((n, k, h, w), dtype=np.float32), None
        else:
            lg = rng.standard_normal((n, k, h, w))
            if weights == "dominant":
                np.put_along_axis(lg, rng.integers(0, k, (n, 1, h, w)), 80.0, axis=1)
            wgt = softmax64(lg).astype(np.float32)
            # log W + a per-pixel shift of tens of units (it cancels in the softmax)
            shift = (3.0 if side == "1" else -50.0) + 20.0 * rng.standard_normal((n, 1, h, w))
            d["w" + side], d["lg" + side] = wgt, (np.log(wgt.astype(np.float64)) + shift).astype(np.float32)
        for name in "ab":
            if field in ("boundary", "edge"):
                values = BOUNDARY_OFFSETS if field == "boundary" else EDGE_OFFSETS
                off = rng.choice(np.array(values, np.float32), size=(n, k, h, w))
            elif field == "far":
                sign = 1.0 if (side == "1") == (name == "a") else -1.0
                off = (rng.standard_normal((n, k, h, w)) * 0.5 + sign * 97.3).astype(np.float32)
            else:
                amp = {"gauss3": 3.0, "gauss1": 1.0, "gauss02": 0.2, "gauss01": 0.1}[field]
                off = (rng.standard_normal((n, k, h, w)) * amp).astype(np.float32)
            d[name + side] = off
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(case, logits=False):
    """fused_ref of the case's inputs, computed once per process; logits=True: from lg1 / lg2 (the kernel's input there)."""
    d = inputs(case)
    w1, w2 = (d["lg1"], d["lg2"]) if logits else (d["w1"], d["w2"])
    ref = fused_ref(d["f0"], d["f2"], w1, d["a1"], d["b1"], w2, d["a2"], d["b2"], d["occ"], case.dil, weights_are_logits=logits)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def modes_of(case):
    return MODES[:2] if case.weights == "rand" else MODES


def errors(case, got, ref):
    """(largest image error, largest mask excess over its bound [<= 0 passes], largest mask error, all finite) of the four
    outputs `got` (t1, t2, frame, mask as arrays) against the float64 `ref`."""
    rtol = MASK_RTOL_FAR if case.field == "far" else MASK_RTOL
    g = [np.asarray(x, dtype=np.float64) for x in got]
    finite = all(np.isfinite(x).all() for x in g)
    img = max(float(np.abs(x - ref[k]).max()) for x, k in zip(g[:3], ("t1", "t2", "frame")))
    merr = np.abs(g[3] - ref["mask"])
    excess = float((merr - (MASK_ATOL + rtol * np.abs(ref["mask"]))).max())
    return img, excess, float(merr.max()), finite


def passes(img, excess, finite):
    return finite and img <= IMAGE_ATOL and excess <= 0.0


# ---- the kernels, through the Python wrapper ------------------------------------------------------------------------------
def interleave(frame):
    """planar (N,3,H,W) -> (N,H,W,4) with NaN in the fourth lane: a finite output proves the lane is never used."""
    import torch
    return torch.cat((frame, torch.full_like(frame[:, :1], float("nan"))), 1).permute(0, 2, 3, 1).contiguous()


def device_inputs(case, device):
    import torch
    d = {k: torch.from_numpy(np.array(v)).to(device) for k, v in inputs(case).items() if v is not None}
    d["x0"], d["x2"] = interleave(d["f0"]), interleave(d["f2"])
    return d


def launch(case, d, mode, **kw):
    """One adacof_fused call of the case in `mode` on the device tensors `d` -> (t1, t2, frame, mask)."""
    from vfi_amd.adacof.cupy_module.adacof import adacof_fused
    rgbx, logits = mode != "planar", mode == "rgbx_logits"
    fr0, fr2 = (d["x0"], d["x2"]) if rgbx else (d["f0"], d["f2"])
    w1, w2 = (d["lg1"], d["lg2"]) if logits else (d["w1"], d["w2"])
    return adacof_fused(fr0, fr2, w1, d["a1"], d["b1"], w2, d["a2"], d["b2"], d["occ"], case.dil, rgbx=rgbx,
                        weights_are_logits=logits, **kw)


def run_case(case, device):
    """Runs every mode of the case; yields (mode, image error, mask excess, mask error, finite)."""
    import torch
    d = device_inputs(case, device)
    for mode in modes_of(case):
        got = launch(case, d, mode)
        torch.cuda.synchronize()
        yield (mode,) + errors(case, [x.cpu().numpy() for x in got], reference(case, mode == "rgbx_logits"))
