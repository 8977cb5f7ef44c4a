"""GPU parity of the fp32-MFMA convolution (through the C ABI) against a plain PyTorch fp32
CPU reference of the same op (the op the oracle networks are built from)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vfi_amd import ops

pytestmark = pytest.mark.gpu


def _ref(x, w, b, ks, pad_mode, act, res=None, bn=None):
    p = (ks - 1) // 2
    if p and pad_mode == "reflect":
        y = F.conv2d(F.pad(x, (p,) * 4, mode="reflect"), w, b)
    else:
        y = F.conv2d(x, w, b, padding=p)
    if bn is not None:
        g, beta, mean, var, eps = bn
        y = F.batch_norm(y, mean, var, g, beta, training=False, eps=eps)
    y = {None: lambda t: t, "relu": F.relu, "elu": F.elu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](y)
    return y if res is None else y + res


CASES = [
    # n, cin, cout, h, w, ks, pad, act
    (1, 6, 32, 24, 40, 3, "zeros", "relu"),       # KernelEstimation first layer (Cin tail 6 -> 8)
    (2, 32, 64, 17, 33, 3, "zeros", "relu"),      # ragged tile edges, batch 2
    (1, 64, 25, 16, 32, 3, "zeros", None),        # head output (Cout tail 25 -> 32)
    (1, 25, 25, 19, 21, 3, "zeros", None),
    (1, 64, 1, 16, 16, 3, "zeros", "sigmoid"),    # occlusion head
    (3, 88, 64, 23, 31, 3, "reflect", "elu"),     # PhaseNet 3x3 reflect block, batch = colour
    (3, 81, 64, 9, 15, 1, "reflect", "elu"),      # PhaseNet 1x1 block
    (3, 64, 8, 9, 15, 1, "zeros", "tanh"),        # prediction map
    (1, 2, 64, 5, 7, 1, "zeros", "elu"),          # PhaseNet block 0 on the low residual
    (1, 18, 32, 24, 40, 5, "reflect", "relu"),    # FusionNet encoder 5x5
    (1, 128, 64, 12, 20, 5, "reflect", None),     # FusionNet decoder 5x5
    (1, 32, 3, 24, 40, 1, "zeros", None),
    (1, 128, 128, 10, 12, 3, "reflect", None),    # bottleneck
    (1, 256, 512, 8, 8, 3, "zeros", "relu"),      # deep U-Net level, many chunks
    (1, 3, 64, 3, 3, 3, "reflect", None),         # tiny image, smaller than one tile
]


@pytest.mark.parametrize("n,cin,cout,h,w,ks,pad,act", CASES)
def test_conv_matches_torch_cpu(n, cin, cout, h, w, ks, pad, act, device):
    g = torch.Generator().manual_seed(cin * 1000 + cout + h)
    x = torch.randn((n, cin, h, w), generator=g)
    wgt = torch.randn((cout, cin, ks, ks), generator=g) / (cin * ks * ks) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    ref = _ref(x, wgt, b, ks, pad, act)
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d(x.to(device), pc, pad, act)
    torch.cuda.synchronize()
    err = (out.cpu() - ref).abs().max().item()
    assert err <= 2e-5, err


@pytest.mark.parametrize("n,cin,cout,h,w,act", [(3, 64, 8, 96, 128, "tanh"), (1, 64, 1, 64, 68, "tanh"), (1, 32, 3, 80, 100, None),
                                                (2, 70, 5, 66, 64, "elu"), (1, 7, 8, 64, 64, "relu"), (1, 64, 9, 72, 96, None),
                                                (3, 64, 8, 74, 83, "tanh"), (2, 16, 16, 70, 61, "sigmoid")])
def test_conv1x1_streaming_kernel_matches_torch_cpu(n, cin, cout, h, w, act, device):
    """1x1 layers with <= 16 output channels and an even number of >= 4096 pixels take conv1x1_stream_kernel (csrc/vfi_conv.hip;
    four pixels per thread, two where the plane size is no multiple of four; the last case -- an odd plane -- stays on the matrix cores):
    PhaseNet's prediction maps (phase_net.py:190-207), read from and written into channel slices of the 72-channel block buffer."""
    g = torch.Generator().manual_seed(cin * 100 + cout + h)
    wide_in = torch.randn((n, cin + 9, h, w), generator=g)
    wgt = torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    ref = _ref(wide_in[:, 4:4 + cin], wgt, b, 1, "zeros", act)
    pc = ops.PackedConv(wgt, b, device=device)
    xin = wide_in.to(device)
    wide_out = torch.full((n, cout + 4, h, w), 7.0, device=device)
    ops.conv2d(xin[:, 4:4 + cin], pc, "zeros", act, out=wide_out[:, 4:])
    torch.cuda.synchronize()
    assert (wide_out[:, 4:].cpu() - ref).abs().max().item() <= 2e-5
    assert (wide_out[:, :4] == 7.0).all()          # the neighbouring channels of the slice are untouched


BIG_CASES = [
    # 3x3 layers the F(4x4,3x3) Winograd kernel takes (csrc/vfi_conv_winograd4.hip: >= 2000 items of a 16x64 tile x 32 couts,
    # Cin >= 16)
    # n, cin, cout, h, w, pad, act
    (1, 16, 32, 512, 2048, "zeros", "relu"),      # exact tiles
    (2, 18, 40, 250, 2044, "reflect", None),      # ragged tile rows / columns, Cin and Cout tails, two channel blocks
    (1, 17, 64, 500, 1026, "zeros", "elu"),       # row length not a multiple of 4: element-wise stores
]


@pytest.mark.parametrize("n,cin,cout,h,w,pad,act", BIG_CASES)
def test_large_plain_conv_matches_torch_cpu(n, cin, cout, h, w, pad, act, device):
    g = torch.Generator().manual_seed(cin * 1000 + cout + h)
    x = torch.randn((n, cin, h, w), generator=g)
    wgt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    ref = _ref(x.double(), wgt.double(), b.double(), 3, pad, act)
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d(x.to(device), pc, pad, act)
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    # the larger Winograd tile costs about a decimal digit: rms 2e-6, maximum 3e-5 of the output rms
    assert err.max().item() <= 1e-4 and err.pow(2).mean().sqrt().item() <= 5e-6, (err.max().item(), err.pow(2).mean().sqrt().item())


def test_f4x4_kernel_on_small_and_ragged_shapes(device):
    # VFI_CONV_WINOGRAD4=2 sends EVERY 3x3 layer through the F(4x4) kernel (the library reads the switch once per process,
    # hence the child process): 60 random shapes -- tiles on both image borders, partial tiles, Cin / Cout tails,
    # zero / reflect padding, residuals, all activations -- against float64 (tools/fuzz_conv.py)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VFI_CONV_WINOGRAD4="2")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_conv.py"), "17", "60"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])          # (non-zero on any FAIL line, too)
    assert not re.search(r"^FAIL", r.stdout, flags=re.M), r.stdout[-2000:]    # no case failed: non-finite outputs included
    m = re.search(r"worst abs error ([0-9.e+-]+)", r.stdout)
    assert m and float(m.group(1)) <= 1e-4, r.stdout[-2000:]


@pytest.mark.parametrize("n,cin,cout,h,w,pad,act,variant", [
    (1, 64, 64, 272, 1920, "zeros", "relu", "plain"),       # the 1080p U-Net / PhaseNet shape class: 16 chunks per item
    (3, 64, 64, 100, 1920, "reflect", "elu", "residual"),   # PhaseNet block with its residual, ragged tile rows
    (2, 64, 64, 132, 1920, "zeros", "relu", "residual"),    # decoder skip layer: the ReLU-specialised residual instantiation, residual rows requested one channel ahead
    (1, 28, 25, 544, 1920, "zeros", None, "plain"),         # head layer: 7 chunks (odd: both body parities end an item), Cout tail
    (2, 32, 64, 256, 1024, "zeros", "relu", "pool"),        # pooled second output
    (1, 16, 96, 512, 2048, "reflect", "tanh", "plain"),     # three channel blocks, 4 chunks: items shorter than the ring
])
def test_f4x4_m32_kernel_equals_m16_kernel_bit_for_bit(n, cin, cout, h, w, pad, act, variant, device, monkeypatch):
    """conv3x3_winograd4m_kernel (one wave per SIMD, 32 output channels per wave, hand-scheduled chunk body) performs the
    arithmetic of conv3x3_winograd4_kernel in the same order: where the row length is a multiple of the 64-column tile the
    two must agree bit for bit (VFI_CONV_WINOGRAD4M selects per call).  Also against float64 with the F(4x4) tolerance."""
    from vfi_amd import _lib
    g = torch.Generator().manual_seed(cin * 7 + cout + h)
    x = torch.randn((n, cin, h, w), generator=g)
    wgt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    res = torch.randn((n, cout, h, w), generator=g) if variant == "residual" else None
    pc = ops.PackedConv(wgt, b, device=device)
    xd, rd = x.to(device), None if res is None else res.to(device)

    def run():
        if variant == "pool":
            return ops.conv2d_pool2(xd, pc, False, pad, act)
        return (ops.conv2d(xd, pc, pad, act, residual=rd),)

    assert _lib.lib().vfi_conv2d_algo(n, cin, h, w, cout, 3, int(res is not None), int(variant == "pool"), ops.ACT[act]) == 2, "shape must take the F(4x4) path"
    monkeypatch.setenv("VFI_CONV_WINOGRAD4M", "0")
    old = [t.clone() for t in run()]
    monkeypatch.setenv("VFI_CONV_WINOGRAD4M", "1")
    new = run()
    torch.cuda.synchronize()
    for a_, b_ in zip(old, new):
        assert torch.equal(a_, b_), (a_ - b_).abs().max().item()
    ref = _ref(x.double(), wgt.double(), b.double(), 3, pad, act, res=None if res is None else res.double())
    err = (new[0].cpu().double() - ref).abs()
    assert err.max().item() <= 1e-4 and err.pow(2).mean().sqrt().item() <= 5e-6, (err.max().item(), err.pow(2).mean().sqrt().item())


def test_large_conv_with_trained_weight_statistics(device):
    """A PhaseNet-class 64 -> 64 3x3 reflect / ELU layer on the F(4x4) kernel with the statistics of the TRAINED phase_net.pt
    instead of default init (tests/golden/trained_weight_stats.json, layer 7): weight std 0.03-0.04 with outliers up to
    0.5, BatchNorm folded with running variances of ~0.05 (a x4-x6 gain per channel), inputs distributed like ELU outputs.
    F(4x4)'s error depends on the operand range (its transforms multiply by up to 8, and ELU outputs are not zero-mean):
    measured on these statistics 2.5e-4 at worst for an output rms of 1.23 -- 2.5x the unit-variance cases' 1e-4; the
    bound is 5e-4 / 2e-5 (max / rms) of the output rms.  End to end the same statistics cost PhaseNet's 720p branch 25 dB
    (107 dB instead of 132 dB against the oracle, tests/test_pipeline_gpu.py), far inside the 60 dB bar."""
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_weight_stats.json")) as f:
        st = json.load(f)["phasenet"]
    n, c, h, w = 3, 64, 270, 1920
    g = torch.Generator().manual_seed(11)

    def draw(key):
        d = st[key]
        return (torch.randn(d["shape"], generator=g, dtype=torch.float64) * d["std"] + d["mean"]).clamp_(d["min"], d["max"]).float()
    wgt, b = draw("layers.7.feature_map.3.weight"), draw("layers.7.feature_map.3.bias")
    bn = (draw("layers.7.feature_map.1.weight"), draw("layers.7.feature_map.1.bias"), draw("layers.7.feature_map.1.running_mean"),
          draw("layers.7.feature_map.1.running_var"), 1e-5)
    assert list(wgt.shape) == [64, 64, 3, 3]
    x = F.elu(torch.randn((n, c, h, w), generator=g) * 2.0)                         # (what the previous block hands over)
    ref = _ref(x.double(), wgt.double(), b.double(), 3, "reflect", "elu", bn=tuple(t.double() if torch.is_tensor(t) else t for t in bn))
    pc = ops.PackedConv(wgt, b, bn=bn, device=device)
    assert _lib_algo(n, c, c, h, w, "elu") == 2, "shape must take the F(4x4) path"
    out = ops.conv2d(x.to(device), pc, "reflect", "elu")
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    rms = ref.pow(2).mean().sqrt().item()
    erms = err.pow(2).mean().sqrt().item()
    print("trained-statistics conv: output rms %.3f, error rms %.3g max %.3g" % (rms, erms, err.max().item()), flush=True)
    assert err.max().item() <= 5e-4 * max(1.0, rms) and erms <= 2e-5 * max(1.0, rms), (rms, erms, err.max().item())


def _lib_algo(n, cin, cout, h, w, act, residual=False, pooled=False):
    from vfi_amd import _lib
    return _lib.lib().vfi_conv2d_algo(n, cin, h, w, cout, 3, int(residual), int(pooled), ops.ACT[act])


def test_large_conv_with_residual_matches_torch_cpu(device):
    # the residual variant of the F(4x4) Winograd kernel (PhaseNet blocks at full resolution): act(conv + b) + residual
    n, cin, cout, h, w = 2, 16, 64, 270, 1920
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, cin, h, w), generator=g)
    res = torch.randn((n, cout, h, w), generator=g)
    wgt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    ref = _ref(x.double(), wgt.double(), b.double(), 3, "reflect", "elu", res=res.double())
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d(x.to(device), pc, "reflect", "elu", residual=res.to(device))
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    assert err.max().item() <= 1e-4 and err.pow(2).mean().sqrt().item() <= 5e-6, (err.max().item(), err.pow(2).mean().sqrt().item())


def test_conv_bn_fold_residual_and_channel_slices(device):
    g = torch.Generator().manual_seed(0)
    n, h, w = 2, 20, 36
    wide = torch.randn((n, 100, h, w), generator=g)
    x = wide[:, 10:74]                                     # 64-channel slice of a wider tensor
    wgt = torch.randn((64, 64, 3, 3), generator=g) / 24
    b = torch.randn((64,), generator=g) * 0.1
    bn = (torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1,
          torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5, 1e-5)
    res = torch.randn((n, 64, h, w), generator=g)
    ref = _ref(x, wgt, b, 3, "reflect", "elu", res=res, bn=bn)
    pc = ops.PackedConv(wgt, b, bn=bn, device=device)
    dwide = wide.to(device)
    dout = torch.zeros((n, 96, h, w), device=device)
    ops.conv2d(dwide[:, 10:74], pc, "reflect", "elu", residual=res.to(device), out=dout[:, 16:80])
    torch.cuda.synchronize()
    assert (dout[:, 16:80].cpu() - ref).abs().max().item() <= 3e-5
    assert dout[:, :16].abs().max().item() == 0 and dout[:, 80:].abs().max().item() == 0


def test_conv_is_exact_on_integer_data(device):
    # fp32 MFMA is an exact fp32 fma chain: small-integer data must give the exact integer result
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (1, 16, 16, 40), generator=g).float()
    wgt = torch.randint(-2, 3, (32, 16, 3, 3), generator=g).float()
    ref = F.conv2d(x, wgt, None, padding=1)
    out = ops.conv2d(x.to(device), ops.PackedConv(wgt, None, device=device), "zeros", None)
    assert torch.equal(out.cpu(), ref)


def test_conv_full_size_linearity_720p(device):
    # BASELINE-size property (no CPU oracle): conv(a*x1 + x2) == a*conv(x1) + conv(x2) (bias-free)
    g = torch.Generator().manual_seed(2)
    h, w = 736, 1280
    x1 = torch.randn((1, 32, h, w), generator=g).to(device)
    x2 = torch.randn((1, 32, h, w), generator=g).to(device)
    wgt = torch.randn((32, 32, 3, 3), generator=g) / 17
    pc = ops.PackedConv(wgt, None, device=device)
    y1, y2 = ops.conv2d(x1, pc), ops.conv2d(x2, pc)
    y12 = ops.conv2d(2.0 * x1 + x2, pc)
    # (the layer takes the F(4x4) kernel since the round-4 selection rule: 1e-4 at worst per output, three outputs combined)
    assert (y12 - (2.0 * y1 + y2)).abs().max().item() <= 3e-4
    # and a window of the full-size launch against the CPU reference
    ref = F.conv2d(x1[:, :, 100:140, 200:300].cpu(), wgt, None, padding=1)
    assert (y1[:, :, 101:139, 201:299].cpu() - ref[:, :, 1:-1, 1:-1]).abs().max().item() <= 1e-4


def test_conv_argument_errors(device):
    pc = ops.PackedConv(torch.zeros(8, 4, 3, 3), None, device=device)
    with pytest.raises(ops.VfiLibraryError):
        ops.conv2d(torch.zeros(1, 5, 8, 8, device=device), pc)          # channel mismatch
    with pytest.raises(ops.VfiLibraryError):
        ops.conv2d(torch.zeros(1, 4, 8, 8), pc)                         # CPU tensor: no fallback
    with pytest.raises(ops.VfiLibraryError):
        ops.conv2d(torch.zeros(1, 4, 1, 8, device=device), pc, "reflect")  # reflect pad >= size


@pytest.mark.parametrize("n,cin,cout,hs,ws,act", [(1, 25, 25, 24, 40, None), (2, 64, 64, 9, 17, "relu"),
                                                   (1, 64, 1, 16, 16, "sigmoid"), (1, 128, 128, 8, 12, "relu")])
def test_conv_fused_upsample_matches_torch(n, cin, cout, hs, ws, act, device):
    # Upsample(x2, bilinear, align_corners=True) -> conv3x3 (+act, +skip) in one launch
    g = torch.Generator().manual_seed(cin + hs)
    x = torch.randn((n, cin, hs, ws), generator=g)
    wgt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    res = torch.randn((n, cout, 2 * hs, 2 * ws), generator=g)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    ref = _ref(up, wgt, b, 3, "zeros", act, res=res)
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d(x.to(device), pc, "zeros", act, residual=res.to(device), upsample2x=True)
    assert (out.cpu() - ref).abs().max().item() <= 3e-5


@pytest.mark.parametrize("n,c2,cd,hs,ws,h,w", [(3, 72, 16, 17, 24, 24, 34), (1, 72, 16, 9, 15, 12, 22), (2, 64, 24, 20, 30, 29, 43)])
def test_conv_resized_prefix_matches_torch(n, c2, cd, hs, ws, h, w, device):
    # conv over [bilinear_resize(x2, align_corners=False) | x[:, c2:]] == PhaseNet's block input (phase_net.py:138-141)
    g = torch.Generator().manual_seed(h * w)
    x2 = torch.randn((n, c2, hs, ws), generator=g)
    direct = torch.randn((n, cd, h, w), generator=g)
    wgt = torch.randn((64, c2 + cd, 3, 3), generator=g) / ((c2 + cd) * 9) ** 0.5
    b = torch.randn((64,), generator=g) * 0.1
    full = torch.cat((F.interpolate(x2, size=(h, w), mode="bilinear", align_corners=False), direct), 1)
    ref = _ref(full, wgt, b, 3, "reflect", "elu")
    x = torch.full((n, c2 + cd, h, w), float("nan"))            # the prefix channels of x must never be read
    x[:, c2:] = direct
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d_resized_prefix(x.to(device), x2.to(device), pc, "reflect", "elu")
    assert (out.cpu() - ref).abs().max().item() <= 3e-5


# The 3x3 layers run the Winograd F(2x2,3x3) kernel: interior tiles fetch 16-byte pieces, image-border tiles per element;
# float4 stores need W % 4 == 0 and full tiles; long channel loops with few tiles are split over K; the activation is a
# template parameter, a residual selects another instantiation.
WINOGRAD_CASES = [
    # n, cin, cout, h, w, pad, act, residual
    (1, 64, 64, 24, 160, "zeros", "relu", False),      # 5 tile columns: interior (16-byte) and border tiles, full tiles
    (2, 40, 96, 40, 128, "reflect", "elu", False),     # three channel blocks, reflect rows / columns
    (1, 64, 64, 21, 131, "zeros", None, False),        # odd width: element-wise stores, ragged last tile
    (1, 30, 25, 33, 98, "reflect", "tanh", False),     # W % 4 = 2, channel tails on both sides
    (3, 64, 64, 16, 96, "reflect", "elu", True),       # residual instantiation (PhaseNet block)
    (1, 16, 32, 16, 64, "zeros", "sigmoid", True),
    (1, 512, 512, 12, 20, "zeros", "relu", False),     # split-K range (few tiles, 128 chunks)
    (2, 256, 128, 9, 40, "reflect", None, False),
    (1, 512, 96, 9, 15, "zeros", "elu", False),        # split-K with H*W % 4 != 0: element-wise reduce kernel
    (1, 4, 32, 8, 32, "zeros", None, False),           # a single chunk per item
    (1, 3, 3, 2, 2, "reflect", None, False),           # smallest reflect-padded image
]


@pytest.mark.parametrize("n,cin,cout,h,w,pad,act,residual", WINOGRAD_CASES)
def test_winograd_conv_matches_torch_cpu(n, cin, cout, h, w, pad, act, residual, device):
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + w)
    x = torch.randn((n, cin, h, w), generator=g)
    wgt = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    res = torch.randn((n, cout, h, w), generator=g) if residual else None
    ref = _ref(x.double(), wgt.double(), b.double(), 3, pad, act, None if res is None else res.double()).float()
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d(x.to(device), pc, pad, act, residual=None if res is None else res.to(device))
    torch.cuda.synchronize()
    # fp32 Winograd: the transforms add a few roundings to the direct sum (values are O(1))
    assert (out.cpu() - ref).abs().max().item() <= 3e-5


def test_winograd_conv_channel_slices_and_batch_strides(device):
    # input and output are channel slices of wider tensors (PhaseNet's concatenated block inputs): only the batch
    # stride is free; what lies outside the slices must stay untouched
    g = torch.Generator().manual_seed(5)
    big_in = torch.randn((2, 80, 16, 96), generator=g).to(device)
    big_out = torch.full((2, 100, 16, 96), 7.0, device=device)
    wgt = torch.randn((48, 40, 3, 3), generator=g) / 19.0
    b = torch.randn((48,), generator=g) * 0.1
    pc = ops.PackedConv(wgt, b, device=device)
    ops.conv2d(big_in[:, 24:64], pc, "reflect", "relu", out=big_out[:, 20:68])
    torch.cuda.synchronize()
    ref = _ref(big_in[:, 24:64].cpu().double(), wgt.double(), b.double(), 3, "reflect", "relu").float()
    assert (big_out[:, 20:68].cpu() - ref).abs().max().item() <= 3e-5
    assert (big_out[:, :20] == 7.0).all() and (big_out[:, 68:] == 7.0).all()


def test_winograd_conv_is_deterministic(device):
    g = torch.Generator().manual_seed(9)
    x = torch.randn((2, 64, 40, 160), generator=g).to(device)
    wgt = torch.randn((64, 64, 3, 3), generator=g) / 24.0
    pc = ops.PackedConv(wgt, torch.zeros(64), device=device)
    first = ops.conv2d(x, pc, "zeros", "relu").clone()
    for _ in range(5):
        ops.conv2d(torch.randn_like(x), pc, "zeros", None)          # other data through the same kernel in between
        assert torch.equal(ops.conv2d(x, pc, "zeros", "relu"), first)


def test_winograd_conv_one_chunk_items_keep_their_bias(device):
    # Cin <= 4: every work item is a single chunk, so the DMA cursor runs several items (and their bias fetches) ahead
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 3, 64, 256), generator=g)
    wgt = torch.randn((96, 3, 3, 3), generator=g) / 5.0
    b = torch.randn((96,), generator=g)
    pc = ops.PackedConv(wgt, b, device=device)
    out = ops.conv2d(x.to(device), pc, "zeros", None)
    torch.cuda.synchronize()
    assert (out.cpu() - _ref(x.double(), wgt.double(), b.double(), 3, "zeros", None).float()).abs().max().item() <= 3e-5


@pytest.mark.parametrize("n,cin,cout,h,w,ks,is_max,pad", [(2, 6, 32, 64, 96, 3, False, "zeros"), (1, 64, 128, 40, 72, 3, True, "reflect"),
                                                         (1, 32, 64, 37, 51, 3, False, "zeros"), (1, 512, 512, 8, 12, 3, False, "zeros"),
                                                         (1, 18, 32, 40, 72, 5, True, "reflect"),
                                                         # large enough for the F(4x4) Winograd kernel, ragged / odd sizes
                                                         (1, 16, 32, 512, 2048, 3, False, "zeros"), (2, 18, 40, 251, 2046, 3, True, "reflect")])
def test_conv_with_fused_pooling_equals_conv_then_pool(n, cin, cout, h, w, ks, is_max, pad, device):
    # vfi_conv2d_pool2: the pooled tensor written by the Winograd epilogue (3x3 ReLU layers in one piece), or by a pooling
    # pass behind split-K / direct layers -- bit-identical to conv2d followed by pool2 either way; odd sizes floor
    g = torch.Generator().manual_seed(h * w + cin)
    x = torch.randn((n, cin, h, w), generator=g).to(device)
    wgt = torch.randn((cout, cin, ks, ks), generator=g) / (ks * cin ** 0.5)
    pc = ops.PackedConv(wgt, torch.randn((cout,), generator=g), device=device)
    y, q = ops.conv2d_pool2(x, pc, is_max, pad, "relu")
    y_ref = ops.conv2d(x, pc, pad, "relu")
    assert torch.equal(y, y_ref)
    assert q.shape == (n, cout, h // 2, w // 2) and torch.equal(q, ops.pool2(y_ref, is_max))
