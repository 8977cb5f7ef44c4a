"""Clip interpolation over a Y4M stream on the GPU (vfi_amd.fusion_net.interpolate_stream): frame
order and pass-through, the interpolated frames against the runner's own output, independence of the number of frames in
flight, `FusionInterpolator.run_prepared` against `__call__`, short and truncated clips, and the command line over pipes.
Seeded weights and synthetic frames as in tests/test_clip_io.py; frames are 64x96, C420jpeg, limited range."""
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
from vfi_amd.fusion_net import y4m

pytestmark = pytest.mark.gpu

H, W = 64, 96
HEADER = b"YUV4MPEG2 W96 H64 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n"
FMT = (ops.YUV_420, ops.YUV_SITING_CENTRE, ops.YUV_BT709, ops.YUV_LIMITED)
LINES = [b"FRAME\n", b"FRAME Xnote=1\n", b"FRAME\n", b"FRAME Ip\n", b"FRAME\n"]


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
    return [FusionInterpolator(adacof, fusion, weights["phasenet"], device) for _ in range(3)]


@pytest.fixture(scope="module")
def frames(device):
    """five source frames as Y4M bytes"""
    from oracle import synth
    out = []
    for i in range(5):
        f = synth.translating_pair(3, H, W, shift=(1.5 * i, -1.0 * i))[2]
        out.append(ops.rgb_to_yuv(torch.from_numpy(np.ascontiguousarray(f)).to(device), FMT).cpu().numpy().tobytes())
    return out


def clip(frames, n=None, lines=LINES, header=HEADER):
    n = len(frames) if n is None else n
    return header + b"".join(lines[i] + frames[i] for i in range(n))


def parse(data):
    """-> (Y4MFormat, [(FRAME line, bytes)]) of a whole stream; nothing may be left over"""
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
    args = types.SimpleNamespace(gpu_id=0, matrix="bt709", range="limited", keep_rate=False, **kw)
    dst = io.BytesIO()
    n = st.interpolate_stream(args, io.BytesIO(data), dst, runners=runners[:max(1, fif)], frames_in_flight=fif)
    return n, dst.getvalue(), args


@pytest.fixture(scope="module")
def five(frames, runners):
    return run(clip(frames), runners, 2)


def test_five_frames_order_pass_through_and_interpolated_frames(five, frames, runners, device):
    n, data, args = five
    assert n == 4 and not args.truncated
    fmt, out = parse(data)
    assert len(out) == 9
    assert fmt.rate == (60000, 1001)
    assert data.split(b"\n", 1)[0] + b"\n" == HEADER.replace(b"F30000:1001", b"F60000:1001")      # every other token verbatim
    for i in range(5):                                                # originals at even positions, byte for byte, own FRAME lines
        assert out[2 * i] == (LINES[i], frames[i])
    # interpolated frame k against the runner's own output for that pair, computed sequentially on one runner
    dec = lambda b: ops.yuv_to_rgb(torch.frombuffer(bytearray(b), dtype=torch.uint8).to(device), H, W, FMT, rgb=True, lab=(True, None))
    for k in range(4):
        assert out[2 * k + 1][0] == b"FRAME\n"
        (rgb1, lab1, _), (rgb2, lab2, _) = dec(frames[k]), dec(frames[k + 1])
        final = runners[0].run_prepared(rgb1, rgb2, torch.cat((lab1, lab2), 0))["final"][0]
        ref = ops.rgb_to_yuv(final, FMT).cpu().numpy().astype(np.int64)
        got = np.frombuffer(out[2 * k + 1][1], dtype=np.uint8).astype(np.int64)
        assert np.abs(got - ref).max() <= 1, k
        assert np.abs(got - np.frombuffer(frames[k], dtype=np.uint8)).max() > 1          # (not a copy of an original)


@pytest.mark.parametrize("fif", [1, 3])
def test_output_does_not_depend_on_frames_in_flight(fif, five, frames, runners):
    n, data, _ = run(clip(frames), runners, fif)
    assert n == 4 and data == five[1]


def test_run_prepared_is_call_without_the_lab_conversion(frames, runners, device):
    from oracle import synth
    a, _, b = (torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in synth.translating_pair(7, H, W))
    want = runners[0](a, b, output_baseline=True)
    lab12 = torch.cat((ops.rgb2lab(a), ops.rgb2lab(b)), 0)
    keep = lab12.clone()
    got = runners[0].run_prepared(a, b, lab12, output_baseline=True)
    assert set(got) == set(want) and "baseline" in got
    for name in want:
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(lab12, keep)                                   # read, never written
    with pytest.raises(ValueError):
        runners[0].run_prepared(a, b, lab12[:3])


def test_one_frame_and_no_frame(frames, runners):
    n, data, args = run(clip(frames, 1), runners)
    assert n == 0 and not args.truncated
    fmt, out = parse(data)
    assert out == [(LINES[0], frames[0])] and fmt.rate == (60000, 1001)
    n, data, args = run(HEADER, runners)
    assert n == 0 and data == HEADER.replace(b"F30000:1001", b"F60000:1001") and not args.truncated


def test_keep_rate(frames, runners, five):
    args = types.SimpleNamespace(gpu_id=0, keep_rate=True)
    dst = io.BytesIO()
    assert st.interpolate_stream(args, io.BytesIO(clip(frames, 2)), dst, runners=runners[:2]) == 1
    data = dst.getvalue()
    assert data.startswith(HEADER)                                    # the input's header, F included
    assert parse(data)[1] == parse(five[1])[1][:3]


def test_a_size_that_is_no_multiple_of_8_raises_before_any_launch(runners):
    """70 rows: valid 4:2:0, but FusionNet pools three times by 2.  Nothing is written and no kernel runs: the runners'
    per-size state is not even created."""
    sizes = [set(r._per_size) for r in runners]
    dst = io.BytesIO()
    data = b"YUV4MPEG2 W96 H70 C420jpeg\n" + (b"FRAME\n" + bytes(96 * 70 * 3 // 2)) * 2
    with pytest.raises(ValueError, match="multiples of 8"):
        st.interpolate_stream(types.SimpleNamespace(gpu_id=0), io.BytesIO(data), dst, runners=runners[:2])
    assert dst.getvalue() == b"" and [set(r._per_size) for r in runners] == sizes


def test_truncated_stream_finishes_the_complete_frames(frames, runners, five):
    data = clip(frames, 3) + LINES[3] + frames[3][:len(frames[3]) // 2]
    n, got, args = run(data, runners)
    assert n == 2 and args.truncated
    fmt, out = parse(got)
    assert len(out) == 5 and out == parse(five[1])[1][:5]


def test_command_line_over_pipes_in_a_fresh_child(tmp_path, weights, frames, five):
    torch.save(weights["fusionnet"], tmp_path / "fusion_net.pt")
    torch.save(weights["phasenet"], tmp_path / "phase_net.pt")
    torch.save({"epoch": 0, "state_dict": weights["adacof"]}, tmp_path / "ckpt.pth")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG_DIR, ROOT, os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, "-m", "vfi_amd.fusion_net.interpolate_stream", "--input", "-", "--output", "-",
           "--adacof_checkpoint", str(tmp_path / "ckpt.pth"), "--adacof_config", "", "--checkpoint", str(tmp_path / "fusion_net.pt"),
           "--phase_net_checkpoint", str(tmp_path / "phase_net.pt")]
    p = subprocess.run(cmd, input=clip(frames), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout.startswith(y4m.MAGIC)                             # nothing else was printed there
    assert p.stdout == five[1]
    assert b"4 interpolated frames" in p.stderr
