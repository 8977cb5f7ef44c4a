"""YUV4MPEG2 (`.y4m`) streams on the host: header and frame framing, nothing else (no torch, no device).

A stream is `YUV4MPEG2 W<w> H<h> [F<num>:<den>] [I<c>] [A<n>:<d>] [C<tag>] [X<...>]*\\n`, then per frame a line `FRAME[ params]\\n`
followed by the frame's planes: H * W luma bytes, then Cb, then Cr.  What the pixels mean (subsampling, chroma siting,
matrix, range) is four small integers that `vfi_amd.ops.yuv_to_rgb` / `rgb_to_yuv` take: `Y4MFormat.yuv`.

8-bit progressive 4:2:0 and 4:4:4 are built; every other tag is refused by name with what it would need.
"""

MAGIC = b"YUV4MPEG2"

# VFI_YUV_* of include/vfi_hip.h (restated: this module imports nothing of the library)
YUV_420, YUV_444 = 0, 1
SITING_CENTRE, SITING_LEFT = 0, 1
BT709, BT601 = 0, 1
LIMITED, FULL = 0, 1
MATRICES = {"bt709": BT709, "bt601": BT601}
RANGES = {"limited": LIMITED, "full": FULL}

# C tag -> (subsampling, horizontal chroma siting); a header without a C tag means C420jpeg (the format's default)
C_TAGS = {"C420jpeg": (YUV_420, SITING_CENTRE), "C420paldv": (YUV_420, SITING_CENTRE), "C420mpeg2": (YUV_420, SITING_LEFT),
          "C420": (YUV_420, SITING_LEFT), "C444": (YUV_444, SITING_CENTRE)}
_NOT_BUILT = (("C422", "4:2:2 needs a horizontal-only chroma resampler"), ("C411", "4:1:1 needs a 4x horizontal chroma resampler"),
              ("C440", "4:4:0 needs a vertical-only chroma resampler"), ("Cmono", "mono needs a luma-only path"),
              ("C444alpha", "alpha needs a fourth plane"))
MAX_HEADER = 4096          # bytes of a header or FRAME line before it counts as garbage


class Y4MError(ValueError):
    """The stream is not YUV4MPEG2, or is a flavour of it that is not built."""


def _refuse_c_tag(tag):
    if any(tag.endswith(s) for s in ("p9", "p10", "p12", "p14", "p16")):
        raise Y4MError(f"{tag}: more than 8 bits per sample needs 16-bit planes and kernels")
    for name, why in _NOT_BUILT:
        if tag == name or (name != "C444alpha" and tag.startswith(name)):
            raise Y4MError(f"{tag}: {why}")
    raise Y4MError(f"{tag}: unknown colour space tag (built: {', '.join(sorted(C_TAGS))})")


class Y4MFormat:
    """A parsed header.  width, height; rate = (num, den) or None; interlace, aspect, c_tag: the I, A and C tokens without
    their letter, None where absent; x_tokens: the X... tokens verbatim; tokens: every token after the magic, verbatim and
    in order; subsampling, siting, matrix, range: the four integers of the kernels; truncated: set by read_frame_into."""

    def __init__(self, width, height, rate=None, interlace=None, aspect=None, c_tag=None, x_tokens=(), tokens=None,
                 matrix="bt709", range="limited"):
        self.width, self.height = int(width), int(height)
        self.rate, self.interlace, self.aspect, self.c_tag = rate, interlace, aspect, c_tag
        self.x_tokens = list(x_tokens)
        tag = "C" + c_tag if c_tag is not None else "C420jpeg"
        if tag not in C_TAGS:
            _refuse_c_tag(tag)
        self.subsampling, self.siting = C_TAGS[tag]
        if self.width <= 0 or self.height <= 0:
            raise Y4MError(f"W{self.width} H{self.height}: sizes must be positive")
        if self.subsampling == YUV_420 and (self.width % 2 or self.height % 2):
            raise Y4MError(f"W{self.width} H{self.height}: {tag} needs even sizes")
        self.matrix = MATRICES[matrix] if isinstance(matrix, str) else int(matrix)
        self.range = RANGES[range] if isinstance(range, str) else int(range)
        for t in self.x_tokens:                                # the header's own word on the range wins
            if t.upper() == "XCOLORRANGE=FULL":
                self.range = FULL
            elif t.upper() == "XCOLORRANGE=LIMITED":
                self.range = LIMITED
        if tokens is None:
            tokens = [f"W{self.width}", f"H{self.height}"]
            tokens += [f"F{rate[0]}:{rate[1]}"] if rate else []
            tokens += [f"I{interlace}"] if interlace is not None else []
            tokens += [f"A{aspect}"] if aspect is not None else []
            tokens += [f"C{c_tag}"] if c_tag is not None else []
            tokens += self.x_tokens
        self.tokens = list(tokens)
        self.truncated = False

    @property
    def yuv(self):
        return (self.subsampling, self.siting, self.matrix, self.range)

    @property
    def frame_bytes(self):
        w, h = self.width, self.height
        return w * h + 2 * ((w // 2) * (h // 2) if self.subsampling == YUV_420 else w * h)


def _read_line(stream, what):
    """Bytes up to and including the next newline, read one byte at a time (a pipe cannot seek back); b"" at a clean end."""
    line = bytearray()
    while True:
        b = stream.read(1)
        if not b:
            return bytes(line)
        line += b
        if b == b"\n":
            return bytes(line)
        if len(line) > MAX_HEADER:
            raise Y4MError(f"{what}: no newline within {MAX_HEADER} bytes")


def read_header(stream, matrix="bt709", range="limited"):
    """Parses the stream's first line -> Y4MFormat.  matrix / range: the caller's word on what the header cannot say."""
    line = _read_line(stream, "header")
    if not line.startswith(MAGIC) or not line.endswith(b"\n") or line[len(MAGIC):len(MAGIC) + 1] not in (b" ", b"\n"):
        raise Y4MError(f"no YUV4MPEG2 magic: the stream starts with {line[:16]!r}")
    tokens = line[len(MAGIC):-1].decode("ascii", "replace").split()
    width = height = rate = interlace = aspect = c_tag = None
    x_tokens = []
    for t in tokens:
        key, val = t[0], t[1:]
        try:
            if key == "W":
                width = int(val)
            elif key == "H":
                height = int(val)
            elif key == "F":
                num, den = val.split(":")
                rate = (int(num), int(den))
            elif key == "I":
                interlace = val
            elif key == "A":
                aspect = val
            elif key == "C":
                c_tag = val
            elif key == "X":
                x_tokens.append(t)
            else:
                raise Y4MError(f"{t}: unknown header token")
        except ValueError as e:
            if isinstance(e, Y4MError):
                raise
            raise Y4MError(f"{t}: malformed header token") from None
    if width is None:
        raise Y4MError("header has no W token")
    if height is None:
        raise Y4MError("header has no H token")
    if interlace not in (None, "p", "?"):
        raise Y4MError(f"I{interlace}: interlaced material needs field-aware chroma siting and is not built")
    return Y4MFormat(width, height, rate, interlace, aspect, c_tag, x_tokens, tokens, matrix, range)


def header_line(fmt, rate=None):
    """The header of `fmt` as bytes: its tokens verbatim, the F token replaced by `rate` = (num, den) where given (added
    after H when the input had none)."""
    tokens = list(fmt.tokens)
    if rate is not None:
        f = f"F{int(rate[0])}:{int(rate[1])}"
        at = [i for i, t in enumerate(tokens) if t[0] == "F"]
        if at:
            tokens[at[0]] = f
        else:
            at = [i for i, t in enumerate(tokens) if t[0] == "H"]
            tokens.insert(at[0] + 1 if at else len(tokens), f)
    return MAGIC + b" " + " ".join(tokens).encode("ascii") + b"\n"


def write_header(stream, fmt, rate=None):
    stream.write(header_line(fmt, rate))


def read_frame_into(stream, buf, fmt=None):
    """Reads one frame into `buf` (a writable buffer of exactly the frame's size).  -> the `FRAME...` line verbatim (with its
    newline), or None at the end of the stream.  Short reads (a pipe) are looped over.  A last frame that stops short -- in
    its line or in its bytes -- is reported as the end, with `fmt.truncated` set where a Y4MFormat is given."""
    line = _read_line(stream, "FRAME line")
    if not line:
        return None
    if not line.endswith(b"\n"):
        if b"FRAME".startswith(line[:5]) or line.startswith(b"FRAME"):
            if fmt is not None:
                fmt.truncated = True
            return None
        raise Y4MError(f"expected FRAME, got {line[:16]!r}")
    if not line.startswith(b"FRAME") or line[5:6] not in (b" ", b"\n"):
        raise Y4MError(f"expected FRAME, got {line[:16]!r}")
    view = memoryview(buf).cast("B")
    got, n = 0, len(view)
    readinto = getattr(stream, "readinto", None)
    while got < n:
        if readinto is not None:
            k = readinto(view[got:])
        else:
            chunk = stream.read(n - got)
            k = len(chunk)
            view[got:got + k] = chunk
        if not k:
            if fmt is not None:
                fmt.truncated = True
            return None
        got += k
    return line


def index_clip(path, matrix="bt709", range="limited"):
    """Random access to a clip on disk -> (Y4MFormat, offsets): the byte offset of each complete frame's data.  `path` is a
    file name or a seekable binary stream.  The FRAME lines are walked with seeks (a FRAME line may carry parameters, so
    frames are not equidistant in general); no frame data is read.  A last frame that stops short -- in its line or in its
    bytes -- is left out and sets `fmt.truncated`.  A stream that cannot seek raises Y4MError."""
    if not hasattr(path, "read"):
        with open(path, "rb") as stream:
            return index_clip(stream, matrix, range)
    stream = path
    seekable = getattr(stream, "seekable", None)
    if seekable is None or not seekable():
        raise Y4MError("index_clip needs a stream that can seek (a file, not a pipe)")
    fmt = read_header(stream, matrix, range)
    at = stream.tell()
    end = stream.seek(0, 2)
    n = fmt.frame_bytes
    offsets = []
    while at < end:
        stream.seek(at)
        line = _read_line(stream, "FRAME line")
        if not line.endswith(b"\n"):
            if b"FRAME".startswith(line[:5]) or line.startswith(b"FRAME"):
                fmt.truncated = True
                break
            raise Y4MError(f"expected FRAME, got {line[:16]!r}")
        if not line.startswith(b"FRAME") or line[5:6] not in (b" ", b"\n"):
            raise Y4MError(f"expected FRAME, got {line[:16]!r}")
        data = at + len(line)
        if data + n > end:
            fmt.truncated = True
            break
        offsets.append(data)
        at = data + n
    return fmt, offsets


def write_frame(stream, frame_line, buf):
    stream.write(frame_line)
    stream.write(memoryview(buf).cast("B"))
