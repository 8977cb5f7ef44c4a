"""Clip I/O over Y4M streams, the parts that need no device: header and frame framing of
vfi_amd.fusion_net.y4m, the command line's parser, the argument validation of vfi_yuv_to_rgb / vfi_rgb_to_yuv, and
self-checks of the numpy restatements in yuv_ref.py that the GPU tests compare against."""
import ctypes
import io

import numpy as np
import pytest

import yuv_ref as YR
from vfi_amd.fusion_net import y4m


class Dribble(io.RawIOBase):
    """A pipe at its worst: every read returns 1 to 7 bytes."""

    def __init__(self, data, seed=0):
        self.data, self.pos, self.rng = bytes(data), 0, np.random.default_rng(seed)

    def readable(self):
        return True

    def readinto(self, b):
        n = min(len(b), int(self.rng.integers(1, 8)), len(self.data) - self.pos)
        b[:n] = self.data[self.pos:self.pos + n]
        self.pos += n
        return n


def _stream(header, frames, lines=None):
    out = bytearray(header)
    for i, f in enumerate(frames):
        out += (lines[i] if lines else b"FRAME\n") + bytes(f)
    return bytes(out)


@pytest.mark.parametrize("tag,sub,siting", [("C420jpeg", 0, 0), ("C420paldv", 0, 0), ("C420mpeg2", 0, 1), ("C420", 0, 1),
                                            ("C444", 1, 0), (None, 0, 0)])
def test_header_round_trip_for_every_accepted_c_tag(tag, sub, siting):
    tokens = ["W96", "H64", "F30000:1001", "Ip", "A1:1"] + ([tag] if tag else []) + ["XYSCSS=420JPEG", "XCOLORRANGE=LIMITED"]
    line = ("YUV4MPEG2 " + " ".join(tokens) + "\n").encode()
    fmt = y4m.read_header(io.BytesIO(line + b"FRAME\n"))
    assert (fmt.width, fmt.height, fmt.rate, fmt.interlace, fmt.aspect) == (96, 64, (30000, 1001), "p", "1:1")
    assert fmt.c_tag == (tag[1:] if tag else None) and fmt.x_tokens == ["XYSCSS=420JPEG", "XCOLORRANGE=LIMITED"]
    assert fmt.yuv == (sub, siting, y4m.BT709, y4m.LIMITED)
    assert fmt.frame_bytes == (96 * 64 * 3 if sub else 96 * 64 * 3 // 2)
    out = io.BytesIO()
    y4m.write_header(out, fmt)
    assert out.getvalue() == line                                     # verbatim, token for token
    out = io.BytesIO()
    y4m.write_header(out, fmt, rate=(fmt.rate[0] * 2, fmt.rate[1]))
    assert out.getvalue() == line.replace(b"F30000:1001", b"F60000:1001")


def test_header_without_optional_tokens_and_with_unknown_interlace():
    fmt = y4m.read_header(io.BytesIO(b"YUV4MPEG2 W8 H6\n"))
    assert (fmt.rate, fmt.interlace, fmt.aspect, fmt.c_tag, fmt.x_tokens) == (None, None, None, None, [])
    assert fmt.frame_bytes == 72 and fmt.tokens == ["W8", "H6"]
    assert y4m.header_line(fmt) == b"YUV4MPEG2 W8 H6\n"
    assert y4m.header_line(fmt, rate=(50, 1)) == b"YUV4MPEG2 W8 H6 F50:1\n"
    assert y4m.read_header(io.BytesIO(b"YUV4MPEG2 W8 H6 I? F25:1\n")).interlace == "?"
    assert y4m.read_header(io.BytesIO(b"YUV4MPEG2 H5 W3 C444\n")).frame_bytes == 45     # 4:4:4 takes odd sizes


def test_matrix_and_range_come_from_the_caller_unless_the_header_names_the_range():
    h = b"YUV4MPEG2 W8 H8 C420mpeg2\n"
    assert y4m.read_header(io.BytesIO(h)).yuv == (0, 1, y4m.BT709, y4m.LIMITED)
    assert y4m.read_header(io.BytesIO(h), matrix="bt601", range="full").yuv == (0, 1, y4m.BT601, y4m.FULL)
    hf = b"YUV4MPEG2 W8 H8 C420mpeg2 XCOLORRANGE=FULL\n"
    assert y4m.read_header(io.BytesIO(hf), range="limited").range == y4m.FULL
    hl = b"YUV4MPEG2 W8 H8 XCOLORRANGE=LIMITED\n"
    assert y4m.read_header(io.BytesIO(hl), range="full").range == y4m.LIMITED


@pytest.mark.parametrize("seed", [0, 1])
def test_frames_through_a_stream_that_returns_1_to_7_bytes_per_call(seed):
    rng = np.random.default_rng(seed)
    header = b"YUV4MPEG2 W6 H4 F24:1 C420jpeg\n"
    frames = [rng.integers(0, 256, 36, dtype=np.uint8) for _ in range(3)]
    lines = [b"FRAME\n", b"FRAME Ixyz Xfoo=bar\n", b"FRAME\n"]
    src = Dribble(_stream(header, frames, lines), seed)
    fmt = y4m.read_header(src)
    assert fmt.frame_bytes == 36
    buf = np.zeros(36, dtype=np.uint8)
    for f, line in zip(frames, lines):
        assert y4m.read_frame_into(src, buf, fmt) == line              # parameters preserved
        assert np.array_equal(buf, f)
    assert y4m.read_frame_into(src, buf, fmt) is None and not fmt.truncated      # a clean end
    out = io.BytesIO()
    y4m.write_header(out, fmt)
    for f, line in zip(frames, lines):
        y4m.write_frame(out, line, f)
    assert out.getvalue() == _stream(header, frames, lines)


@pytest.mark.parametrize("cut", [1, 17, 36 + 3, 36 + 6, 36 + 7 + 20])
def test_truncated_last_frame_is_the_end_and_sets_the_flag(cut):
    """the stream stops `cut` bytes into the frames: inside the first frame's bytes, inside the second FRAME line, right
    after it, inside the second frame"""
    header = b"YUV4MPEG2 W6 H4 C420jpeg\n"
    frames = [np.full(36, 7, dtype=np.uint8), np.full(36, 9, dtype=np.uint8)]
    data = _stream(header, frames)
    for src in (io.BytesIO(data[:len(header) + 6 + cut]), Dribble(data[:len(header) + 6 + cut])):
        fmt = y4m.read_header(src)
        buf, complete = np.zeros(36, dtype=np.uint8), 0
        while y4m.read_frame_into(src, buf, fmt) is not None:
            complete += 1
        assert complete == (1 if cut >= 36 else 0) and fmt.truncated


def test_garbage_where_a_frame_line_belongs():
    src = io.BytesIO(b"YUV4MPEG2 W2 H2\nFRAME\n" + bytes(6) + b"JUNK\n" + bytes(6))
    fmt = y4m.read_header(src)
    buf = np.zeros(6, dtype=np.uint8)
    assert y4m.read_frame_into(src, buf, fmt) == b"FRAME\n"
    with pytest.raises(y4m.Y4MError, match="JUNK"):
        y4m.read_frame_into(src, buf, fmt)


@pytest.mark.parametrize("header,token", [
    (b"YUV4MPEG W8 H8\n", "YUV4MPEG2"), (b"\x89PNG\r\n\x1a\n", "YUV4MPEG2"), (b"", "YUV4MPEG2"),
    (b"YUV4MPEG2 H8 F25:1\n", "W"), (b"YUV4MPEG2 W8 F25:1\n", "H"),
    (b"YUV4MPEG2 W8 H8 It\n", "It"), (b"YUV4MPEG2 W8 H8 Ib\n", "Ib"), (b"YUV4MPEG2 W8 H8 Im\n", "Im"),
    (b"YUV4MPEG2 W8 H8 C422\n", "C422"), (b"YUV4MPEG2 W8 H8 C411\n", "C411"), (b"YUV4MPEG2 W8 H8 Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W8 H8 C444alpha\n", "C444alpha"), (b"YUV4MPEG2 W8 H8 C420p10\n", "C420p10"),
    (b"YUV4MPEG2 W8 H8 C444p12\n", "C444p12"), (b"YUV4MPEG2 W8 H8 C422p16\n", "C422p16"), (b"YUV4MPEG2 W8 H8 Cmono16\n", "Cmono16"),
    (b"YUV4MPEG2 W8 H8 C420foo\n", "C420foo"), (b"YUV4MPEG2 W7 H8 C420jpeg\n", "W7"), (b"YUV4MPEG2 W8 H8 Fabc\n", "Fabc"),
])
def test_refusals_name_the_token(header, token):
    with pytest.raises(y4m.Y4MError) as e:
        y4m.read_header(io.BytesIO(header))
    assert token in str(e.value)


def test_parser_defaults_and_dash_for_both_ends():
    from vfi_amd.fusion_net import interpolate_stream as st
    a = st.parser.parse_args([])
    assert (a.input, a.output, a.matrix, a.range, a.keep_rate, a.frames_in_flight) == ("-", "-", "bt709", "limited", False, 2)
    assert (a.gpu_id, a.adacof_kernel_size, a.adacof_dilation, a.model) == (0, 5, 1, 1)
    assert a.adacof_model == "vfi_amd.fusion_net.fusion_adacofnet"
    a = st.parser.parse_args(["--input", "-", "--output", "-", "--matrix", "bt601", "--range", "full", "--keep_rate",
                              "--frames_in_flight", "3", "--checkpoint", "f.pt", "--phase_net_checkpoint", "p.pt"])
    assert (a.input, a.output, a.matrix, a.range, a.keep_rate, a.frames_in_flight) == ("-", "-", "bt601", "full", True, 3)
    assert (a.checkpoint, a.phase_net_checkpoint) == ("f.pt", "p.pt")
    a = st.parser.parse_args(["--input", "a.y4m", "--output", "b.y4m"])
    assert (a.input, a.output) == ("a.y4m", "b.y4m")
    with pytest.raises(SystemExit):
        st.parser.parse_args(["--matrix", "bt2020"])


def test_a_size_that_is_no_multiple_of_8_is_refused_before_anything_else():
    import types
    from vfi_amd.fusion_net import interpolate_stream as st
    dst = io.BytesIO()
    with pytest.raises(ValueError, match="multiples of 8"):
        st.interpolate_stream(types.SimpleNamespace(gpu_id=0), io.BytesIO(b"YUV4MPEG2 W96 H70 C420jpeg\n"), dst, runners=[None])
    assert dst.getvalue() == b""


# ------------------------------------------------------------------------------------------- the C ABI, without a device

INVALID, SHAPE, UNSUPPORTED = -1, -2, -4


def test_abi_argument_validation_needs_no_gpu():
    import vfi_amd
    h = vfi_amd.lib()
    one = ctypes.c_void_p(16)
    fmt = lambda *v: ctypes.addressof(keep.setdefault(v, (ctypes.c_int * 4)(*v)))
    keep = {}
    ok = fmt(0, 0, 0, 0)
    dec = lambda frame=one, hh=8, ww=8, f=ok, rgb=one, la=one, lb=one: h.vfi_yuv_to_rgb(frame, hh, ww, f, rgb, la, lb, None)
    enc = lambda rgb=one, hh=8, ww=8, f=ok, frame=one: h.vfi_rgb_to_yuv(rgb, hh, ww, f, frame, None)
    # null pointers
    assert dec(frame=None) == INVALID and dec(f=None) == INVALID
    assert enc(rgb=None) == INVALID and enc(frame=None) == INVALID and enc(f=None) == INVALID
    # all three outputs NULL; every other combination passes this check and is stopped by the next one only
    assert dec(rgb=None, la=None, lb=None) == INVALID and b"NULL" in h.vfi_last_error()
    for outs in ((one, None, None), (None, one, None), (None, None, one), (one, one, None), (None, one, one), (one, None, one)):
        assert dec(hh=65536, ww=65536, rgb=outs[0], la=outs[1], lb=outs[2]) == UNSUPPORTED
    # sizes
    for fn in (dec, enc):
        assert fn(hh=0) == INVALID and fn(ww=0) == INVALID and fn(hh=-2) == INVALID
        assert fn(hh=7) == SHAPE and fn(ww=9) == SHAPE and b"even" in h.vfi_last_error()       # odd sizes in 4:2:0
        for bad in ((2, 0, 0, 0), (-1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, -1, 0), (0, 0, 0, 2), (1, 0, 0, 7)):
            assert fn(f=fmt(*bad)) == INVALID, bad
        assert fn(hh=65536, ww=32768) == UNSUPPORTED and fn(hh=46342, ww=46342) == UNSUPPORTED      # H * W >= 2^31
        assert fn(hh=65536, ww=32768, f=fmt(1, 1, 1, 1)) == UNSUPPORTED


# ------------------------------------------------------------------------------------------- the restatements themselves

def _flat(h, w, y, cb, cr, fmt):
    n = YR.frame_bytes(h, w, fmt)
    f = np.empty(n, dtype=np.uint8)
    f[:h * w] = y
    c = (n - h * w) // 2
    f[h * w:h * w + c], f[h * w + c:] = cb, cr
    return f


@pytest.mark.parametrize("fmt", [f for f in YR.FORMATS_420 + YR.FORMATS_444 if f[3] == YR.LIMITED], ids=YR.fmt_id)
def test_restated_decode_of_black_and_white(fmt):
    for dtype, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        black = YR.yuv_to_rgb(_flat(4, 6, 16, 128, 128, fmt), 4, 6, fmt, dtype)
        white = YR.yuv_to_rgb(_flat(4, 6, 235, 128, 128, fmt), 4, 6, fmt, dtype)
        assert np.abs(black).max() <= tol and np.abs(white - 1).max() <= tol


@pytest.mark.parametrize("matrix", [YR.BT709, YR.BT601])
def test_restated_full_range_444_encode_of_decode_is_the_identity_on_every_grey_byte(matrix):
    fmt = (YR.S444, YR.CENTRE, matrix, YR.FULL)
    frame = np.concatenate([np.arange(256, dtype=np.uint8), np.full(512, 128, dtype=np.uint8)])
    for dtype in (np.float64, np.float32):
        rgb = YR.yuv_to_rgb(frame, 16, 16, fmt, dtype)
        assert np.array_equal(YR.rgb_to_yuv(rgb, fmt, dtype), frame)


def test_restated_lab_is_the_oracles():
    import torch
    from oracle import color_cpu
    rgb = np.random.default_rng(2).random((3, 6, 8)).astype(np.float32)
    rgb[:, 0, :] = (np.arange(8, dtype=np.float32) + 8) / 255          # around the sRGB knee (10.3 / 255)
    rgb[:, 1, :] = (np.arange(8, dtype=np.float32) + 19) / 255         # a grey crosses the cube-root knee between 23 and 24
    assert torch.equal(torch.from_numpy(YR.rgb2lab(rgb, np.float64)).float(), color_cpu.rgb2lab_single(torch.from_numpy(rgb)))


def test_restated_upsampling_weights_and_clamps():
    c = np.array([[0, 100], [200, 40]], dtype=np.uint8)
    up = YR.upsample_chroma(c, 4, 4, (YR.S420, YR.CENTRE, 0, 0), np.float64)
    assert up[0, 0] == 0 and up[0, 3] == 100 and up[3, 0] == 200 and up[3, 3] == 40        # every index clamps at a corner
    assert up[0, 1] == 0.75 * 0 + 0.25 * 100 and up[0, 2] == 0.25 * 0 + 0.75 * 100
    assert up[1, 0] == 0.75 * 0 + 0.25 * 200 and up[2, 0] == 0.25 * 0 + 0.75 * 200
    left = YR.upsample_chroma(c, 4, 4, (YR.S420, YR.LEFT, 0, 0), np.float64)
    assert list(left[0]) == [0, 50, 100, 100] and list(left[3]) == [200, 120, 40, 40]


def test_restated_quantiser_ties_limits_and_nan():
    fmt = (YR.S444, 0, 0, YR.LIMITED)
    v = np.array([15.2, 16.5, 17.49999, 235.5,            # Y: 16 ... 235
                  300.0, np.nan, 100.5, 239.5,            # Cb: 16 ... 240
                  240.5, -5.0, np.nan, 128.49], dtype=np.float64)
    assert list(YR.quantise(v, 2, 2, fmt)) == [16, 17, 17, 235, 240, 16, 101, 240, 240, 16, 16, 128]
    full = (YR.S444, 0, 0, YR.FULL)
    assert list(YR.quantise(np.array([-0.6, 254.5, 255.7, np.nan, 0.5, 1e9], dtype=np.float32), 1, 2, full)) == [0, 255, 255, 0, 1, 255]
