"""Numpy restatements of the two clip I/O conversions (include/vfi_hip.h, section "Clip I/O"), every step in the given dtype:
float64 is the reference, float32 the `ref32` of tests/glue_ref.tol_of.  Imports nothing of the library.

A format is (subsampling, siting, matrix, range): 0 = 4:2:0 | 1 = 4:4:4, 0 = centre | 1 = left, 0 = BT.709 | 1 = BT.601,
0 = limited | 1 = full.  A frame is a flat uint8 array: H * W luma bytes, then Cb, then Cr.
"""
import numpy as np

S420, S444 = 0, 1
CENTRE, LEFT = 0, 1
BT709, BT601 = 0, 1
LIMITED, FULL = 0, 1

# the eight 4:2:0 formats, and 4:4:4 in both ranges (its siting field is unused) for both matrices
FORMATS_420 = [(S420, s, m, r) for s in (CENTRE, LEFT) for m in (BT709, BT601) for r in (LIMITED, FULL)]
FORMATS_444 = [(S444, CENTRE, m, r) for m in (BT709, BT601) for r in (LIMITED, FULL)]


def fmt_id(fmt):
    return "-".join((("420", "444")[fmt[0]], ("centre", "left")[fmt[1]], ("bt709", "bt601")[fmt[2]], ("limited", "full")[fmt[3]]))


def frame_bytes(h, w, fmt):
    return h * w + 2 * ((h // 2) * (w // 2) if fmt[0] == S420 else h * w)


def split(frame, h, w, fmt):
    """flat frame -> (Y (h, w), Cb, Cr) uint8 views"""
    ch, cw = (h // 2, w // 2) if fmt[0] == S420 else (h, w)
    y = frame[:h * w].reshape(h, w)
    cb = frame[h * w:h * w + ch * cw].reshape(ch, cw)
    cr = frame[h * w + ch * cw:h * w + 2 * ch * cw].reshape(ch, cw)
    return y, cb, cr


def coefficients(fmt, f):
    kr, kb = (f(0.2126), f(0.0722)) if fmt[2] == BT709 else (f(0.299), f(0.114))
    kg = f(1) - kr - kb
    lim = fmt[3] == LIMITED
    return dict(kr=kr, kb=kb, kg=kg, r_cr=f(2) * (f(1) - kr), b_cb=f(2) * (f(1) - kb), y_off=f(16 if lim else 0),
                y_scale=f(219 if lim else 255), c_scale=f(224 if lim else 255), y_lim=(16, 235) if lim else (0, 255),
                c_lim=(16, 240) if lim else (0, 255))


def _up_centre(c, n, axis, f):
    """bilinear x2 along `axis` for samples sited between output positions 2i and 2i + 1; n = output length"""
    pos = np.arange(n)
    even = pos % 2 == 0
    last = c.shape[axis] - 1
    a = np.where(even, pos // 2 - 1, (pos - 1) // 2).clip(0, last)
    b = np.where(even, pos // 2, (pos + 1) // 2).clip(0, last)
    wa = np.where(even, f(0.25), f(0.75)).astype(f)
    wb = np.where(even, f(0.75), f(0.25)).astype(f)
    shape = [1, 1]
    shape[axis] = n
    return wa.reshape(shape) * np.take(c, a, axis) + wb.reshape(shape) * np.take(c, b, axis)


def _up_left(c, n, f):
    """x2 along columns for samples sited on output column 2i"""
    pos = np.arange(n)
    last = c.shape[1] - 1
    a = np.where(pos % 2 == 0, pos // 2, (pos - 1) // 2).clip(0, last)
    b = np.where(pos % 2 == 0, pos // 2, (pos + 1) // 2).clip(0, last)
    return f(0.5) * (c[:, a] + c[:, b])


def upsample_chroma(c, h, w, fmt, f):
    c = c.astype(f)
    if fmt[0] == S444:
        return c
    c = _up_centre(c, h, 0, f)
    return _up_left(c, w, f) if fmt[1] == LEFT else _up_centre(c, w, 1, f)


def yuv_to_rgb(frame, h, w, fmt, dtype, clamp=True):
    """-> rgb (3, h, w) in `dtype`, clamped to [0, 1] (clamp=False: before the clamp, to see what it cut)"""
    f = dtype
    k = coefficients(fmt, f)
    yb, cbb, crb = split(np.asarray(frame), h, w, fmt)
    y = (yb.astype(f) - k["y_off"]) / k["y_scale"]
    cb = (upsample_chroma(cbb, h, w, fmt, f) - f(128)) / k["c_scale"]
    cr = (upsample_chroma(crb, h, w, fmt, f) - f(128)) / k["c_scale"]
    r = y + k["r_cr"] * cr
    b = y + k["b_cb"] * cb
    g = (y - k["kr"] * r - k["kb"] * b) / k["kg"]
    out = np.stack([r, g, b])
    if clamp:
        out = np.clip(out, f(0), f(1))
    assert out.dtype == f
    return out


# the Lab of oracle.color_cpu.rgb2lab_single, restated so that every step runs in `dtype`
_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
_WHITE = np.array([0.95047, 1.0, 1.08883])


def rgb2lab(rgb, dtype):
    """rgb (3, h, w) -> scaled Lab (3, h, w), every step in `dtype`"""
    f = dtype
    arr = np.moveaxis(rgb, 0, -1).astype(f)
    arr = np.where(arr > f(0.04045), np.power((arr + f(0.055)) / f(1.055), f(2.4)), arr / f(12.92))
    xyz = arr @ _XYZ.T.astype(f) / _WHITE.astype(f)
    t = np.where(xyz > f(0.008856), np.cbrt(xyz), f(7.787) * xyz + f(16.0) / f(116.0))
    L = f(116.0) * t[..., 1] - f(16.0)
    a = f(500.0) * (t[..., 0] - t[..., 1])
    b = f(200.0) * (t[..., 1] - t[..., 2])
    lab = np.stack([L / f(100.0), (a + f(128.0)) / f(255.0), (b + f(128.0)) / f(255.0)])
    assert lab.dtype == f
    return lab


def rgb_to_yuv_unrounded(rgb, fmt, dtype):
    """rgb (3, h, w) float -> flat array in `dtype` of the frame's layout: each byte's value BEFORE floor(v + 0.5) and the
    clamp to the range's limits.  NaN stays NaN."""
    f = dtype
    k = coefficients(fmt, f)
    x = np.asarray(rgb).astype(f)
    x = np.where(x < f(0), f(0), np.where(x > f(1), f(1), x))           # NaN passes
    r, g, b = x
    y = k["kr"] * r + k["kg"] * g + k["kb"] * b
    planes = [(b - y) / k["b_cb"], (r - y) / k["r_cr"]]
    if fmt[0] == S420:
        w = x.shape[2]
        for i, c in enumerate(planes):
            m = f(0.5) * (c[0::2] + c[1::2])
            if fmt[1] == LEFT:
                before = np.arange(0, w, 2) - 1
                planes[i] = (m[:, before.clip(0)] + f(2) * m[:, 0::2] + m[:, 1::2]) * f(0.25)
            else:
                planes[i] = f(0.5) * (m[:, 0::2] + m[:, 1::2])
    out = np.concatenate([(k["y_off"] + k["y_scale"] * y).ravel()] + [(f(128) + k["c_scale"] * c).ravel() for c in planes])
    assert out.dtype == f
    return out


def limits(h, w, fmt):
    """(lo, hi) per byte of a frame, as flat int arrays"""
    k = coefficients(fmt, np.float64)
    n = frame_bytes(h, w, fmt)
    lo, hi = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    lo[:h * w], hi[:h * w] = k["y_lim"]
    lo[h * w:], hi[h * w:] = k["c_lim"]
    return lo, hi


def quantise(v, h, w, fmt):
    """floor(v + 0.5), then the clamp to the range's limits; NaN -> the lower limit.  -> uint8"""
    lo, hi = limits(h, w, fmt)
    with np.errstate(invalid="ignore"):
        q = np.floor(v + v.dtype.type(0.5))
    q = np.where(np.isnan(q), lo, np.clip(np.nan_to_num(q, nan=0.0), lo, hi))
    return q.astype(np.uint8)


def rgb_to_yuv(rgb, fmt, dtype):
    h, w = np.asarray(rgb).shape[1:]
    return quantise(rgb_to_yuv_unrounded(rgb, fmt, dtype), h, w, fmt)


# ------------------------------------------------------------------------------------------------ inputs and the tie rule

def encode_input(h, w, seed):
    """(3, h, w) float32: uniform in [-0.1, 1.1], a quarter of the elements set exactly to k / 255, and of those every
    seventh to 0 and every seventh to 1"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, max(1, flat.size // 4), replace=False)
    flat[idx] = rng.integers(0, 256, idx.size).astype(np.float32) / np.float32(255)
    flat[idx[::7]] = 0
    flat[idx[1::7]] = 1
    return x


def expected_bytes(rgb, fmt):
    """-> (bytes of the float64 restatement, mask of the bytes whose float64 pre-rounding value lies within
    tol_of(pre-round float32, pre-round float64) of a tie, that tolerance).  Only there may an encoder differ, by 1."""
    h, w = rgb.shape[1:]
    v64, v32 = rgb_to_yuv_unrounded(rgb, fmt, np.float64), rgb_to_yuv_unrounded(rgb, fmt, np.float32)
    ok = ~np.isnan(v64)
    tol = max(4.0 * np.abs(v32[ok].astype(np.float64) - v64[ok]).max(), 2.0 ** -23 * np.abs(v64[ok]).max())      # glue_ref.tol_of
    frac = v64 + 0.5 - np.floor(v64 + 0.5)
    with np.errstate(invalid="ignore"):
        near = np.minimum(frac, 1 - frac) <= tol
    return quantise(v64, h, w, fmt), near & ok, tol
