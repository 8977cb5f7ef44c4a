"""Host checks (no device) of the clip loop's rate factor and scene-cut options: the threshold
arithmetic of vfi_amd.fusion_net.scene against hand-computed values, the command line's parser, the argument validation
of vfi_luma_sad / vfi_frame_pick through ctypes, and the factors run_recursive and interpolate_stream refuse."""
import ctypes
import io
import types

import pytest

from vfi_amd.fusion_net import scene

INVALID, UNSUPPORTED = -1, -4


def test_min_sad_is_the_ceiling_of_threshold_times_255_n_over_100():
    assert scene.min_sad(5, 64 * 96) == 78336                  # 5 * 255 * 6144 / 100 = 78336 exactly
    assert scene.min_sad(5, 7) == 90                           # 89.25
    assert scene.min_sad(2.5, 3) == 20                         # 19.125
    assert scene.min_sad(10, 1920 * 1080) == 52876800
    assert scene.min_sad(0.1, 1000) == 255                     # one tenth, not the float above it (which would give 256)
    assert scene.min_sad(100, 10) == 2550 and scene.min_sad(101, 10) == 2576      # above 100: no pair reaches it
    assert scene.min_sad(0, 99) == 0 and scene.min_sad(-3, 99) == 0
    assert isinstance(scene.min_sad(5.0, 6144), int)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            scene.min_sad(5, bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            scene.min_sad(bad, 10)


def test_score_is_min_of_the_mean_difference_and_its_change():
    n = 100                                                    # sad = 255 is 1 %
    assert scene.score(2550, None, n) == 10.0                  # the first pair: m_prev = 0
    assert scene.score(2550, 0, n) == 10.0
    assert scene.score(2550, 1275, n) == 5.0                   # min(10, |10 - 5|)
    assert scene.score(1275, 2550, n) == 5.0                   # sad < sad_prev: min(5, |5 - 10|), no wrap
    assert scene.score(255, 2550, n) == 1.0                    # min(1, 9)
    assert scene.score(2550, 2550, n) == 0.0
    assert scene.score(0, 2550, n) == 0.0


def test_min_sad_and_score_agree_at_the_threshold():
    """score >= threshold exactly where min(sad, |sad - prev|) >= min_sad, on both sides of it"""
    for thr, n in ((5, 6144), (10, 2073600), (2.5, 3), (0.1, 1000), (7.6, 6144)):
        m = scene.min_sad(thr, n)
        assert scene.score(m, None, n) >= thr > scene.score(m - 1, None, n)
        assert scene.score(m + 50, 50, n) >= thr > scene.score(m + 49, 50, n)
        assert scene.score(50, m + 50, n) < thr or m <= 50


def test_parser_defaults_and_the_two_new_options():
    from vfi_amd.fusion_net import interpolate_stream as st
    a = st.parser.parse_args([])
    assert a.factor == 2 and a.scene_threshold is None
    # the existing defaults
    assert (a.input, a.output, a.matrix, a.range, a.keep_rate, a.frames_in_flight) == ("-", "-", "bt709", "limited", False, 2)
    assert (a.gpu_id, a.adacof_kernel_size, a.adacof_dilation, a.model) == (0, 5, 1, 1)
    a = st.parser.parse_args(["--factor", "8", "--scene_threshold", "7.5", "--keep_rate"])
    assert a.factor == 8 and a.scene_threshold == 7.5 and a.keep_rate
    assert st.parser.parse_args(["--factor", "4"]).factor == 4
    for bad in (["--factor", "3"], ["--factor", "1"], ["--factor", "16"], ["--scene_threshold", "high"]):
        with pytest.raises(SystemExit):
            st.parser.parse_args(bad)
    text = st.parser.format_help()
    assert "ffmpeg" in text and "10" in text and "no footage" in " ".join(text.split())


def test_interpolate_stream_refuses_another_factor_before_it_reads_or_writes():
    from vfi_amd.fusion_net import interpolate_stream as st
    dst = io.BytesIO()
    with pytest.raises(ValueError, match="factor"):
        st.interpolate_stream(types.SimpleNamespace(gpu_id=0, factor=3), io.BytesIO(b""), dst, runners=[None])
    assert dst.getvalue() == b""


def test_run_recursive_refuses_another_factor_before_anything_runs():
    from vfi_amd.fusion_net.interpolate_twoframe import FusionInterpolator
    runner = object.__new__(FusionInterpolator)                # no models, no device: the check comes first
    for bad in (3, 1, 0, 16, 2.5, None):
        with pytest.raises(ValueError, match="factor"):
            runner.run_recursive(None, None, None, bad)


def test_abi_argument_validation_needs_no_gpu():
    import vfi_amd
    h = vfi_amd.lib()
    one, two, w1, w2 = (ctypes.c_void_p(v) for v in (4096, 8192, 16, 24))
    sad = lambda a=one, b=two, n=64, out=w1: h.vfi_luma_sad(a, b, n, out, None)
    pick = lambda d=one, s=two, n=64, cur=w1, prev=w2, m=5, cut=w2: h.vfi_frame_pick(d, s, n, cur, prev, m, cut, None)
    # null pointers
    assert sad(a=None) == INVALID and sad(b=None) == INVALID and sad(out=None) == INVALID
    assert b"null" in h.vfi_last_error()
    assert pick(d=None) == INVALID and pick(s=None) == INVALID
    assert pick(cur=None) == INVALID                           # sad must be there; sad_prev and cut may be NULL, which the
    assert pick(cur=None, prev=None, cut=None) == INVALID      # GPU tests run
    # sizes
    for fn in (sad, pick):
        assert fn(n=0) == INVALID and fn(n=-1) == INVALID and fn(n=-(1 << 40)) == INVALID
        assert fn(n=1 << 31) == UNSUPPORTED and fn(n=1 << 40) == UNSUPPORTED
        assert b"2^31" in h.vfi_last_error()
    assert pick(n=1 << 31, prev=None, cut=None, m=0) == UNSUPPORTED


def test_ops_refuse_host_tensors_and_wrong_dtypes():
    import torch
    from vfi_amd import ops
    a = torch.zeros(16, dtype=torch.uint8)
    w = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ops.VfiLibraryError, match="HIP device"):
        ops.luma_sad(a, a, 16)
    with pytest.raises(ops.VfiLibraryError, match="HIP device"):
        ops.frame_pick(a, a, w, None, 5)
    with pytest.raises(ops.VfiLibraryError, match="bad size"):
        ops.luma_sad(a, a, 0)
    with pytest.raises(ops.VfiLibraryError, match="unsigned 64-bit"):
        ops.frame_pick(a, a, w, None, -1)
