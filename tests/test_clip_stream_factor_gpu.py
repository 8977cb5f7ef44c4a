"""The clip loop's rate factor and scene-cut option on the GPU (vfi_amd.fusion_net.interpolate_stream with `factor` and
`scene_threshold`, FusionInterpolator.run_recursive).  Seeded weights and synthetic frames as in
tests/test_clip_stream_gpu.py; frames are 64x96, C420jpeg, limited range."""
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import PKG_DIR, ROOT
from vfi_amd import ops
from vfi_amd.fusion_net import interpolate_stream as st
from vfi_amd.fusion_net import scene, y4m

pytestmark = pytest.mark.gpu

H, W = 64, 96
HEADER = b"YUV4MPEG2 W96 H64 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n"
FMT = (ops.YUV_420, ops.YUV_SITING_CENTRE, ops.YUV_BT709, ops.YUV_LIMITED)
LINES = [b"FRAME\n", b"FRAME Xnote=1\n", b"FRAME\n", b"FRAME Ip\n", b"FRAME\n"]
THRESHOLD = 5


@pytest.fixture(scope="module")
def weights():
    from oracle import pipeline_cpu
    return pipeline_cpu.seeded_weights(0)


@pytest.fixture(scope="module")
def runners(weights, device):
    from vfi_amd.adacof.models import Model
    from vfi_amd.fusion_net.fusion_net import FusionNet
    from vfi_amd.fusion_net.interpolate_twoframe import FusionInterpolator
    adacof = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    adacof.load(weights["adacof"]); adacof.eval()
    fusion = FusionNet().to(device); fusion.load_state_dict(weights["fusionnet"]); fusion.eval()
    return [FusionInterpolator(adacof, fusion, weights["phasenet"], device) for _ in range(2)]


def synth_frame(seed, i, device):
    from oracle import synth
    f = synth.translating_pair(seed, H, W, shift=(1.5 * i, -1.0 * i))[2]
    return ops.rgb_to_yuv(torch.from_numpy(np.ascontiguousarray(f)).to(device), FMT).cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def frames(device):
    """five frames of one scene, as Y4M bytes"""
    return [synth_frame(3, i, device) for i in range(5)]


@pytest.fixture(scope="module")
def cut_frames(frames, device):
    """three frames of that scene, then two of another: the cut is pair 2"""
    return frames[:3] + [synth_frame(7, i, device) for i in (3, 4)]


def clip(frames, n=None):
    n = len(frames) if n is None else n
    return HEADER + b"".join(LINES[i] + frames[i] for i in range(n))


def parse(data):
    src = io.BytesIO(data)
    fmt = y4m.read_header(src)
    out = []
    while True:
        buf = bytearray(fmt.frame_bytes)
        line = y4m.read_frame_into(src, buf, fmt)
        if line is None:
            break
        out.append((line, bytes(buf)))
    assert not fmt.truncated and src.read() == b""
    return fmt, out


def run(data, runners, fif=2, **kw):
    args = types.SimpleNamespace(gpu_id=0, matrix="bt709", range="limited", **{"keep_rate": False, **kw})
    dst = io.BytesIO()
    n = st.interpolate_stream(args, io.BytesIO(data), dst, runners=runners[:max(1, fif)], frames_in_flight=fif)
    return n, dst.getvalue(), args


def decode(b, device):
    rgb, lab, _ = ops.yuv_to_rgb(torch.frombuffer(bytearray(b), dtype=torch.uint8).to(device), H, W, FMT, rgb=True, lab=(True, None))
    return rgb, lab


def header_line(data):
    return data.split(b"\n", 1)[0] + b"\n"


# ------------------------------------------------------------------------------------------------------------ the rate

def test_run_recursive_is_the_composition_of_run_prepared_with_clamp_and_rgb2lab(frames, runners, device):
    r = runners[0]
    (a, la), (b, lb) = decode(frames[0], device), decode(frames[2], device)
    lab12 = torch.cat((la, lb), 0)
    keep = lab12.clone()
    mid = r.run_prepared(a, b, lab12)["final"][0]
    held = mid.clone()
    m = mid.clamp(0.0, 1.0)
    lm = ops.rgb2lab(m)
    q1 = r.run_prepared(a, m, torch.cat((la, lm), 0))["final"][0]
    q3 = r.run_prepared(m, b, torch.cat((lm, lb), 0))["final"][0]
    assert torch.equal(mid, held)                                     # a result survives later calls on its runner
    got = r.run_recursive(a, b, lab12, 4)
    assert len(got) == 3 and all(tuple(t.shape) == (3, H, W) for t in got)
    for name, x, y in zip(("1/4", "1/2", "3/4"), got, (q1, mid, q3)):
        assert torch.equal(x, y), name
    assert torch.equal(got[1], held) and torch.equal(lab12, keep)     # lab12 is read, never written
    assert not torch.equal(q1, mid) and not torch.equal(q3, mid)
    two = r.run_recursive(a, b, lab12, 2)
    assert len(two) == 1 and torch.equal(two[0], mid)
    with pytest.raises(ValueError, match="factor"):
        r.run_recursive(a, b, lab12, 3)


@pytest.fixture(scope="module")
def three4(frames, runners):
    return run(clip(frames, 3), runners, 2, factor=4)


def check_interpolated(out, frames, factor, runner, device):
    """the frames between the originals against rgb_to_yuv of run_recursive, computed sequentially on one runner"""
    for k in range(len(frames) - 1):
        (a, la), (b, lb) = decode(frames[k], device), decode(frames[k + 1], device)
        refs = runner.run_recursive(a, b, torch.cat((la, lb), 0), factor)
        for j, final in enumerate(refs, 1):
            line, data = out[factor * k + j]
            assert line == b"FRAME\n"
            ref = ops.rgb_to_yuv(final, FMT).cpu().numpy().astype(np.int64)
            got = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
            assert np.abs(got - ref).max() <= 1, (k, j)
            assert data != frames[k] and data != frames[k + 1]       # (not a copy of an original)


def test_three_frames_at_factor_4(three4, frames, runners, device):
    n, data, args = three4
    assert n == 6 and not args.truncated and args.scene_cuts == []
    fmt, out = parse(data)
    assert len(out) == 9 and fmt.rate == (120000, 1001)
    assert header_line(data) == HEADER.replace(b"F30000:1001", b"F120000:1001")       # every other token verbatim
    for i in range(3):                                                # originals byte for byte, with their own FRAME lines
        assert out[4 * i] == (LINES[i], frames[i])
    check_interpolated(out, frames[:3], 4, runners[0], device)


def test_factor_4_does_not_depend_on_frames_in_flight(three4, frames, runners):
    n, data, _ = run(clip(frames, 3), runners, 1, factor=4)
    assert n == 6 and data == three4[1]


def test_two_frames_at_factor_8(frames, runners, device):
    n, data, _ = run(clip(frames, 2), runners, 2, factor=8)
    fmt, out = parse(data)
    assert n == 7 and len(out) == 9 and fmt.rate == (240000, 1001)
    assert out[0] == (LINES[0], frames[0]) and out[8] == (LINES[1], frames[1])
    check_interpolated(out, frames[:2], 8, runners[0], device)


def test_keep_rate_leaves_the_rate_alone_at_factor_4(frames, runners, three4):
    n, data, _ = run(clip(frames, 2), runners, 2, factor=4, keep_rate=True)
    assert n == 3 and data.startswith(HEADER)                         # the input's header, F included
    assert parse(data)[1] == parse(three4[1])[1][:5]


def test_factor_2_given_explicitly_is_the_call_without_it(frames, runners):
    plain = run(clip(frames, 3), runners, 2)
    assert plain[0] == 2 and len(parse(plain[1])[1]) == 5
    assert header_line(plain[1]) == HEADER.replace(b"F30000:1001", b"F60000:1001")
    n, data, _ = run(clip(frames, 3), runners, 2, factor=2)
    assert n == 2 and data == plain[1]
    n, data, args = run(clip(frames, 3), runners, 2, factor=2, scene_threshold=None)
    assert n == 2 and data == plain[1] and args.scene_cuts == []


# ------------------------------------------------------------------------------------------------------- scene cuts

def clip_scores(frames):
    """the scores of a clip's own bytes on the reference arithmetic: numpy sums and scene.score"""
    luma = [np.frombuffer(f, dtype=np.uint8)[:H * W].astype(np.int64) for f in frames]
    sads = [int(np.abs(luma[k + 1] - luma[k]).sum()) for k in range(len(frames) - 1)]
    return [scene.score(sads[k], sads[k - 1] if k else None, H * W) for k in range(len(sads))]


def test_the_clips_are_clear_of_the_threshold(frames, cut_frames):
    """a condition on the inputs, checked without the kernels: every score lies at least 1 point from the threshold, the
    cut above it and everything else below"""
    scores = clip_scores(cut_frames)
    print("scores of the clip with a cut:", scores, "without:", clip_scores(frames))
    assert all(abs(s - THRESHOLD) >= 1 for s in scores + clip_scores(frames))
    assert [s >= THRESHOLD for s in scores] == [False, False, True, False]
    assert not any(s >= THRESHOLD for s in clip_scores(frames))


@pytest.fixture(scope="module")
def cut4(cut_frames, runners):
    return run(clip(cut_frames), runners, 2, factor=4, scene_threshold=THRESHOLD)


def test_a_cut_at_factor_2_repeats_the_first_original(cut_frames, runners):
    plain = run(clip(cut_frames), runners, 2)
    n, data, args = run(clip(cut_frames), runners, 2, scene_threshold=THRESHOLD)
    assert n == 4 and args.scene_cuts == [2]
    assert header_line(data) == header_line(plain[1])
    out, ref = parse(data)[1], parse(plain[1])[1]
    assert len(out) == 9
    assert out[5] == (b"FRAME\n", cut_frames[2])                      # frame 2's bytes exactly, behind a plain FRAME line
    assert ref[5][1] != cut_frames[2]
    for i in range(9):
        if i != 5:
            assert out[i] == ref[i], i                                # every other frame: the run without a threshold
    n1, data1, args1 = run(clip(cut_frames), runners, 1, scene_threshold=THRESHOLD)
    assert (n1, data1, args1.scene_cuts) == (4, data, [2])            # one frame in flight: one stream, the same bytes


def test_a_cut_at_factor_4_repeats_the_nearer_original(cut4, cut_frames, runners):
    n, data, args = cut4
    assert n == 12 and args.scene_cuts == [2]
    plain = run(clip(cut_frames), runners, 2, factor=4)
    out, ref = parse(data)[1], parse(plain[1])[1]
    assert len(out) == 17
    assert out[9] == (b"FRAME\n", cut_frames[2]) and out[10] == (b"FRAME\n", cut_frames[2])      # t = 1/4 and the midpoint
    assert out[11] == (b"FRAME\n", cut_frames[3])                                                # t = 3/4
    for i in range(17):
        if i not in (9, 10, 11):
            assert out[i] == ref[i], i
        else:
            assert out[i] != ref[i], i


def test_no_cut_with_the_threshold_set_changes_nothing(three4, frames, runners):
    n, data, args = run(clip(frames, 3), runners, 2, factor=4, scene_threshold=THRESHOLD)
    assert n == 6 and data == three4[1] and args.scene_cuts == []
    n, data, args = run(clip(frames, 1), runners, 2, factor=4, scene_threshold=THRESHOLD)      # no pair at all
    assert n == 0 and args.scene_cuts == [] and parse(data)[1] == [(LINES[0], frames[0])]


def test_threshold_zero_flags_every_pair(frames, runners):
    n, data, args = run(clip(frames, 3), runners, 2, scene_threshold=0)
    assert n == 2 and args.scene_cuts == [0, 1]
    out = parse(data)[1]
    assert [o[1] for o in out] == [frames[0], frames[0], frames[1], frames[1], frames[2]]


# ------------------------------------------------------------------------------------------------- the command line

def test_command_line_with_both_options_in_a_fresh_child(tmp_path, weights, cut_frames, cut4):
    torch.save(weights["fusionnet"], tmp_path / "fusion_net.pt")
    torch.save(weights["phasenet"], tmp_path / "phase_net.pt")
    torch.save({"epoch": 0, "state_dict": weights["adacof"]}, tmp_path / "ckpt.pth")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG_DIR, ROOT, os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, "-m", "vfi_amd.fusion_net.interpolate_stream", "--input", "-", "--output", "-",
           "--adacof_checkpoint", str(tmp_path / "ckpt.pth"), "--adacof_config", "", "--checkpoint", str(tmp_path / "fusion_net.pt"),
           "--phase_net_checkpoint", str(tmp_path / "phase_net.pt"), "--factor", "4", "--scene_threshold", str(THRESHOLD)]
    p = subprocess.run(cmd, input=clip(cut_frames), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout == cut4[1]                                        # from the first byte: nothing else was printed there
    assert b"12 interpolated frames, 1 scene cuts" in p.stderr
