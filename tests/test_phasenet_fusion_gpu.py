"""PhaseNet with three and four input images on the MI355X: the level head's entry points
(vfi_phasenet_emit_n, vfi_phasenet_emit_low_n, vfi_phasenet_predict_n) at their edge shapes, the block-input layout of
Pyramid.filter(concat_frames=3 | 4, pred_channels=...), the coarse-to-fine walk against the float64 restatement
(tests/phasenet_fusion_ref.py, itself held against the reference's outputs by test_phasenet_fusion_host.py), architecture.PhaseNet,
PyramidFusionInterpolator, and the unchanged two-image route.

Tolerances.  Head kernels: glue_ref.assert_close (from the float32 and float64 formulas alone).  The one-pass head: equal bit for
bit to vfi_conv2d(tanh) + vfi_phasenet_emit_n where both stream, 2e-6 where the library falls back to the matrix-core 1x1 kernel
(the two-image test's figure; vfi_conv2d is called as that fall-back calls it, without a split-K workspace -- with one, the
kernel sums in another order, and at (1, 65, 67) the phase output of num_img = 3 and 4 came out 2.09e-6 apart, pi times the 6.6e-7
of pred; that figure is printed, not asserted).  The walk: 1e-4 * max(1, |ref|max) per output tensor, the two-image test's bound; a tensor may
exceed it only up to 4 x what the float32 torch-CPU restatement loses against float64 (section 14's rule).  architecture.PhaseNet:
2e-4 * max(1, |ref|max) against the restatement fed the product's own analysis outputs, through a float64 synthesis.
"""
import functools
import math
import types

import numpy as np
import pytest
import torch

import phasenet_fusion_ref as FR
import pyramid_grad_ref as PR
from glue_ref import assert_close, nan_wide
from oracle import pipeline_cpu, pyramid_cpu, synth
from test_glue_ops_gpu import _gen, _pred_like
from test_phasenet_fusion_host import FIX, layout_vals, same_vals
from vfi_amd import _lib, ops
from vfi_amd._lib import VfiLibraryError
from vfi_amd.phase_net.architecture import PhaseNet as ArchPhaseNet
from vfi_amd.phase_net.phase_net import PhaseNet
from vfi_amd.train import utils
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.values import DecompValues

pytestmark = pytest.mark.gpu
S2 = math.sqrt(2)


def _maxerr(a, b):
    return float((torch.as_tensor(a).detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


# ---- vfi_phasenet_emit_n / vfi_phasenet_emit_low_n ------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_emit_n_matches_the_formulas(hw, n, num_img, device):
    g = _gen(n, hw, num_img)
    p_band = FR.pred_channels(num_img)[1]
    pred = _pred_like((n, p_band, 1, hw), g)
    read = 12 if num_img == 3 else 8                       # the amplitude planes the blends read
    amp_in = torch.rand((n, read, 1, hw), generator=g)
    mx = torch.rand((n,), generator=g) * 3 + 0.1
    _, wide_p = nan_wide((n, 64 + p_band, 1, hw), device)
    pd = wide_p[:, 64:]
    pd.copy_(pred)
    # the block input [feature 64 | pred | phase 4F | amp 4F]; for four images the planes 8..15 stay NaN: never read
    _, wide_a = nan_wide((n, 64 + p_band + 8 * num_img, 1, hw), device)
    ad = wide_a[:, 64 + p_band + 4 * num_img:]
    ad[:, :read].copy_(amp_in)
    phase, amp = ops.phasenet_emit_n(pd, ad, mx.to(device), num_img)
    p32, a32 = FR.emit_n(pred, amp_in, mx, num_img)
    p64, a64 = FR.emit_n(pred.double(), amp_in.double(), mx.double(), num_img)
    rs = lambda t: t.reshape(-1, 1, 1, hw)
    assert_close(phase, rs(p32), rs(p64), f"phasenet_emit_n phase num_img={num_img} n={n} hw={hw}")
    assert_close(amp, rs(a32), rs(a64), f"phasenet_emit_n amp num_img={num_img} n={n} hw={hw}")
    if num_img == 2:
        p2, a2 = ops.phasenet_emit(pd, ad, mx.to(device))
        assert torch.equal(phase, p2) and torch.equal(amp, a2)


@pytest.mark.parametrize("num_img", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 4, 1023, 4100])
def test_emit_low_n_matches_the_formulas(hw, n, num_img, device):
    g = _gen(n, hw, num_img, 2)
    p_low = FR.pred_channels(num_img)[0]
    pred = _pred_like((n, p_low, 1, hw), g)
    read = 3 if num_img == 3 else 2
    low_in = torch.randn((n, read, 1, hw), generator=g)
    mx = torch.rand((n,), generator=g) * 3 + 0.1
    _, wide_p = nan_wide((n, 64 + p_low, 1, hw), device)
    pd = wide_p[:, 64:]
    pd.copy_(pred)
    _, wide_l = nan_wide((n, num_img + 2, 1, hw), device)
    ld = wide_l[:, 1:1 + num_img]                          # for four images the planes 2 and 3 stay NaN: never read
    ld[:, :read].copy_(low_in)
    low = ops.phasenet_emit_low_n(pd, ld, mx.to(device), num_img)
    assert_close(low, FR.emit_low_n(pred, low_in, mx, num_img), FR.emit_low_n(pred.double(), low_in.double(), mx.double(), num_img),
                 f"phasenet_emit_low_n num_img={num_img} n={n} hw={hw}")
    if num_img == 2:
        assert torch.equal(low, ops.phasenet_emit_low(pd, ld, mx.to(device)))


def test_head_wrappers_check_their_shapes(device):
    z = lambda *s: torch.zeros(s, device=device)
    with pytest.raises(VfiLibraryError):
        ops.phasenet_emit_n(z(1, 8, 2, 2), z(1, 12, 2, 2), z(1), 3)           # three images predict 12 channels
    with pytest.raises(VfiLibraryError):
        ops.phasenet_emit_n(z(1, 8, 2, 2), z(1, 8, 2, 2), z(1), 4)            # four images carry 16 amplitude planes
    with pytest.raises(VfiLibraryError):
        ops.phasenet_emit_low_n(z(1, 1, 2, 2), z(1, 3, 2, 2), z(1), 3)
    with pytest.raises(VfiLibraryError):
        ops.phasenet_emit_n(z(1, 8, 2, 2), z(1, 20, 2, 2), z(1), 5)


# ---- vfi_phasenet_predict_n -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [2, 3, 4])
@pytest.mark.parametrize("n,h,w", [(3, 96, 128), (2, 74, 83), (3, 9, 15), (1, 65, 67)])
def test_predict_n_equals_conv_then_emit_n(n, h, w, num_img, device):
    """16-byte streaming, 8-byte streaming (H*W = 2 mod 4), a small level and an odd plane (both fall back inside the library),
    on channel slices of the block buffers: [feature 64 | pred P] and the 88- / 100- / 104-channel block input."""
    g = torch.Generator().manual_seed(h * w + n)              # (test_nets_gpu.py's draw: at two images, its very operands)
    p = FR.pred_channels(num_img)[1]
    fp = torch.randn((n, 64 + p, h, w), generator=g).to(device)
    x = torch.rand((n, 64 + p + 8 * num_img, h, w), generator=g).to(device)
    assert x.shape[1] == {2: 88, 3: 100, 4: 104}[num_img]
    amp_in = x[:, 64 + p + 4 * num_img:]
    if num_img == 4:
        amp_in[:, 8:] = float("nan")                       # the warped sides' amplitudes: the blend must not read them
    mx = (torch.rand((n,), generator=g) + 0.5).to(device)
    pc = ops.PackedConv(torch.randn((p, 64, 1, 1), generator=g) / 8.0, torch.randn((p,), generator=g) * 0.1, device=device)
    ref_fp = fp.clone()
    # vfi_conv2d(act = tanh) as the library's own fall-back calls it: without a split-K workspace
    _lib.call("vfi_conv2d", ref_fp.data_ptr(), ref_fp.stride(0), pc.packed.data_ptr(), pc.bias.data_ptr(), None, 0,
              ref_fp[:, 64:].data_ptr(), ref_fp.stride(0), n, 64, h, w, p, 1, 0, 3, None, 0, _lib.stream_ptr())
    p_ref, a_ref = ops.phasenet_emit_n(ref_fp[:, 64:], amp_in, mx, num_img)
    pred, p_out, a_out = ops.phasenet_predict_n(fp[:, :64], pc, amp_in, mx, num_img, pred=fp[:, 64:])
    torch.cuda.synchronize()
    assert pred.data_ptr() == fp[:, 64:].data_ptr()
    assert torch.equal(fp[:, :64], ref_fp[:, :64])                       # the features are only read
    assert torch.isfinite(p_out).all() and torch.isfinite(a_out).all()
    if h * w >= 4096 and (h * w) % 2 == 0:      # the streaming kernels: the same FMA chain over the channels in both
        assert torch.equal(fp[:, 64:], ref_fp[:, 64:]) and torch.equal(p_out, p_ref) and torch.equal(a_out, a_ref)
    else:
        for got, ref in ((fp[:, 64:], ref_fp[:, 64:]), (p_out, p_ref), (a_out, a_ref)):
            assert (got - ref).abs().max().item() <= 2e-6
        # measured, not asserted: the same composition through ops.conv2d, which hands vfi_conv2d its split-K workspace (another
        # fp32 summation order of the matrix-core kernel; the two orders differ by up to 6.6e-7 in pred, pi times that in phase)
        ws_fp = fp.clone()
        ops.conv2d(ws_fp[:, :64], pc, "zeros", "tanh", out=ws_fp[:, 64:])
        p_ws, a_ws = ops.phasenet_emit_n(ws_fp[:, 64:], amp_in, mx, num_img)
        print(f"predict_n num_img={num_img} {(n, h, w)}: against the split-K composition pred {_maxerr(fp[:, 64:], ws_fp[:, 64:]):.3e} "
              f"phase {_maxerr(p_out, p_ws):.3e} amp {_maxerr(a_out, a_ws):.3e}")
    if num_img == 2:
        fp2 = ref_fp.clone()
        fp2[:, 64:] = 0
        _, p2, a2 = ops.phasenet_predict(fp2[:, :64], pc, amp_in, mx, pred=fp2[:, 64:])
        assert torch.equal(fp2[:, 64:], fp[:, 64:]) and torch.equal(p2, p_out) and torch.equal(a2, a_out)


def test_predict_n_rejects_bad_arguments_before_any_launch(device):
    n, h, w = 1, 8, 8
    fp, x, mx = torch.zeros((n, 72, h, w), device=device), torch.zeros((n, 88, h, w), device=device), torch.ones((n,), device=device)
    pc = ops.PackedConv(torch.zeros((8, 64, 1, 1)), torch.zeros((8,)), device=device)
    po, ao = torch.full((n, 4, h, w), 7.0, device=device), torch.full((n, 4, h, w), 7.0, device=device)
    lib = _lib.lib()
    args = lambda feat, num_img: (feat, fp.stride(0), pc.packed.data_ptr(), pc.bias.data_ptr(), x[:, 80:].data_ptr(), x.stride(0),
                                  mx.data_ptr(), fp[:, 64:].data_ptr(), fp.stride(0), po.data_ptr(), ao.data_ptr(), n, 64, h, w, num_img,
                                  _lib.stream_ptr())
    assert lib.vfi_phasenet_predict_n(*args(fp.data_ptr(), 5)) == -4 and b"num_img 5" in lib.vfi_last_error()
    assert lib.vfi_phasenet_predict_n(*args(fp.data_ptr(), 1)) == -4
    assert lib.vfi_phasenet_predict_n(*args(None, 3)) == -1
    assert lib.vfi_phasenet_emit_n(fp[:, 64:].data_ptr(), fp.stride(0), x[:, 80:].data_ptr(), x.stride(0), mx.data_ptr(), po.data_ptr(),
                                   ao.data_ptr(), n, h * w, 0, _lib.stream_ptr()) == -4
    assert lib.vfi_phasenet_emit_low_n(None, 1, x.data_ptr(), x.stride(0), mx.data_ptr(), po.data_ptr(), n, h * w, 3,
                                       _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((po == 7.0).all()) and bool((ao == 7.0).all())           # nothing ran


# ---- layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", [3, 4])
def test_layout_helpers_at_three_and_four_match_the_reference(num, device):
    g = np.load(FIX)
    h, w, height, c = (int(v) for v in g[f"layout{num}_shape"])
    sep = utils.separate_vals(layout_vals(g, f"layout{num}_vals_", device), num)
    for i, s in enumerate(sep):
        same_vals(s, layout_vals(g, f"layout{num}_sep{i}_"))
    same_vals(utils.get_concat_layers_inf(types.SimpleNamespace(height=height, nbands=4), sep), layout_vals(g, f"layout{num}_cat_"))


def _lab_like_images(seed, count, h, w, device):
    """`count` channel-images with the textures of synth.translating_pair, each shifted differently."""
    imgs = [torch.from_numpy(synth.translating_pair(seed + i, h, w, shift=(1.5 + i, -0.75 * i))[i % 3]) for i in range((count + 2) // 3)]
    return torch.cat(imgs, 0)[:count].contiguous().to(device)


@pytest.mark.parametrize("frames", [3, 4])
def test_concat_layout_of_three_and_four_frames(frames, device):
    h, w = 64, 96
    height = utils.calc_pyr_height(torch.empty(3, h, w, device="meta"))
    img = _lab_like_images(11, 3 * frames, h, w, device)
    pyr = Pyramid(height, 4, S2, device)
    pc = FR.pred_channels(frames)
    want = utils.get_concat_layers_inf(pyr, utils.separate_vals(pyr.filter(img), frames))
    got, bufs, amp_max = pyr.filter(img, concat_frames=frames, phase_scale=1.0 / math.pi, amp_max_eps=1e-8, pred_channels=pc)
    assert got.high_level.shape == (3, frames, h, w) and got.low_level.shape[:2] == (3, frames)
    assert torch.equal(got.high_level, want.high_level) and torch.equal(got.low_level, want.low_level)
    assert amp_max.shape == (height - 2, 3)
    for k in range(height - 2):
        assert got.phase[k].shape[1] == 4 * frames
        assert torch.equal(got.amplitude[k], want.amplitude[k])
        assert (got.phase[k] - want.phase[k] / math.pi).abs().max().item() <= 1e-6
        p = pc[0] if k == 0 else pc[1]
        assert bufs[k].shape[1] == 64 + p + 8 * frames
        assert got.phase[k].data_ptr() == bufs[k][:, 64 + p:].data_ptr()
        assert got.amplitude[k].data_ptr() == bufs[k][:, 64 + p + 4 * frames:].data_ptr()
        assert torch.equal(amp_max[k], ops.batch_max(got.amplitude[k], 1e-8)), k


def test_default_pred_channels_leave_two_frames_as_they_were(device):
    h, w = 64, 96
    height = utils.calc_pyr_height(torch.empty(3, h, w, device="meta"))
    img = _lab_like_images(12, 6, h, w, device)
    pyr = Pyramid(height, 4, S2, device)
    a, bufs_a, max_a = pyr.filter(img, concat_frames=2, phase_scale=1.0 / math.pi, amp_max_eps=1e-8)
    b, bufs_b, max_b = pyr.filter(img, concat_frames=2, phase_scale=1.0 / math.pi, amp_max_eps=1e-8, pred_channels=(1, 8))
    assert [t.shape for t in bufs_a] == [t.shape for t in bufs_b] and bufs_a[0].shape[1] == 81 and bufs_a[1].shape[1] == 88
    assert torch.equal(max_a, max_b) and torch.equal(a.high_level, b.high_level) and torch.equal(a.low_level, b.low_level)
    for x, y in zip(a.phase + a.amplitude, b.phase + b.amplitude):
        assert torch.equal(x, y)
    with pytest.raises(VfiLibraryError, match="at most 16"):
        pyr.filter(torch.zeros((18, h, w), device=device), concat_frames=6)


# ---- the walk ------------------------------------------------------------------------------------------------------------
WALK_SHAPES = {"fixture": (2, 12, 16, 10), "32x48": (3, 32, 48, 6), "96x112": (3, 96, 112, 10)}      # n, h, w, height


def _state(kind, num_img):
    return FR.net_state(23, num_img) if kind == "seeded" else FR.trained_like_state(29, num_img)


@functools.lru_cache(maxsize=None)
def _walk_reference(shape, kind, num_img):
    """Raw inputs and the float64 / float32 torch-CPU restated outputs, computed once per configuration and left unchanged."""
    n, h, w, height = WALK_SHAPES[shape]
    inp = FR.raw_inputs(23 + num_img, n, h, w, height, num_img)
    sd = _state(kind, num_img)
    out = {}
    with torch.no_grad():
        for dtype in (torch.float64, torch.float32):
            low, phases, amps = FR.walk(FR.params(sd, dtype), FR.normalize(FR.to_dtype(inp, dtype)), height - 2, num_img)
            out[dtype] = [low] + phases + amps
    return inp, sd, out


def _device_vals(inp, device):
    d = lambda t: t.to(device)
    return DecompValues(torch.zeros(inp["high_shape"], device=device), [d(p) for p in inp["phase"]], [d(a) for a in inp["amp"]],
                        d(inp["low"]))


_WORST = {}


@pytest.mark.parametrize("num_img", [3, 4])
@pytest.mark.parametrize("kind", ["seeded", "trained"])
@pytest.mark.parametrize("shape", list(WALK_SHAPES))
def test_walk_matches_the_float64_restatement(shape, kind, num_img, device):
    n, h, w, height = WALK_SHAPES[shape]
    L = height - 2
    inp, sd, ref = _walk_reference(shape, kind, num_img)
    net = PhaseNet(types.SimpleNamespace(height=height, nbands=4), device, num_img=num_img)
    net.load_state_dict(sd)
    net.eval()
    normed = net.normalize_vals(_device_vals(inp, device))
    out = net(normed)
    assert out.high_level.shape == (n, 1, h, w) and not bool(out.high_level.any())
    got = [out.low_level] + list(out.phase[::-1]) + list(out.amplitude[::-1])          # coarsest first, as the restatement
    names = ["low"] + [f"phase{i}" for i in range(L)] + [f"amp{i}" for i in range(L)]
    for name, t, r64, r32 in zip(names, got, ref[torch.float64], ref[torch.float32]):
        assert t.shape == r64.shape, name
        scale = max(1.0, float(r64.abs().max()))
        err, lost32 = _maxerr(t, r64), _maxerr(r32, r64)
        key = (num_img, kind)
        _WORST[key] = max(_WORST.get(key, (0.0, "")), (err / scale, f"{shape} {name}"))
        assert err <= max(1e-4 * scale, 4 * lost32), (name, err, scale, lost32)
    print(f"walk num_img={num_img} {kind} {shape}: worst err / max(1, |ref|max) so far {_WORST[(num_img, kind)][0]:.3e} "
          f"({_WORST[(num_img, kind)][1]})")
    if shape == "fixture" and kind == "seeded":     # the same inputs and weights as the reference's own run
        g = np.load(FIX)
        assert int(g["seed"]) == 23
        for i in range(L):
            for got_t, key in ((out.phase[i], f"n{num_img}_out_phase{i}"), (out.amplitude[i], f"n{num_img}_out_amp{i}")):
                want = g[key]
                assert np.abs(got_t.cpu().numpy() - want).max() <= 1e-4 * max(1.0, float(np.abs(want).max())), key
        assert np.abs(out.low_level.cpu().numpy() - g[f"n{num_img}_out_low"]).max() <= 1e-4 * max(1.0, float(np.abs(g[f"n{num_img}_out_low"]).max()))
    # the values may also arrive without the concat fast path (plain DecompValues): the same bits
    plain = DecompValues(normed.high_level, [p.contiguous() for p in normed.phase], [a.contiguous() for a in normed.amplitude],
                         normed.low_level)
    out2 = net(plain)
    assert torch.equal(out.low_level, out2.low_level)
    for a, b in zip(out.phase + out.amplitude, out2.phase + out2.amplitude):
        assert torch.equal(a, b)


@pytest.mark.parametrize("num_img", [3, 4])
def test_walk_protocol_and_partial_levels(num_img, device):
    n, h, w, height = WALK_SHAPES["32x48"]
    inp, sd, ref = _walk_reference("32x48", "seeded", num_img)
    net = PhaseNet(types.SimpleNamespace(height=height, nbands=4), device, num_img=num_img)
    net.load_state_dict(sd)
    dv = _device_vals(inp, device)
    with pytest.raises(RuntimeError):
        net(dv)                                     # normalize_vals must come first
    out = net(net.normalize_vals(dv), m=2)          # phase_net.py:107-110,91-93
    L = height - 2
    assert all(out.phase[k] == 0 and out.amplitude[k] == 0 for k in range(L - 2))
    r64 = ref[torch.float64]
    for k in range(2):                              # the two coarsest levels are those of the full walk
        assert _maxerr(out.phase[L - 1 - k], r64[1 + k]) <= 1e-4 * max(1.0, float(r64[1 + k].abs().max()))
        assert _maxerr(out.amplitude[L - 1 - k], r64[1 + L + k]) <= 1e-4 * max(1.0, float(r64[1 + L + k].abs().max()))
    with pytest.raises(NotImplementedError, match="training of the fusion variants"):
        net.fine_tune()
    with pytest.raises(NotImplementedError):
        PhaseNet(types.SimpleNamespace(height=height, nbands=4), device, num_img=5)


# ---- architecture.PhaseNet -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_img", [3, 4])
def test_architecture_phasenet_with_three_and_four_images(num_img, device):
    h, w = 64, 96
    height = utils.calc_pyr_height(torch.empty(3, h, w, device="meta"))
    L = height - 2
    img = _lab_like_images(21, 3 * (num_img + 1), h, w, device)           # the inputs, then a target
    sd = FR.net_state(7, num_img)
    net = ArchPhaseNet(height, device, num_img=num_img, scale_factor=S2, nbands=4)
    net.core.load_state_dict(sd)
    spec = pyramid_cpu.PyramidSpec(h, w, height)
    d = lambda t: t.detach().cpu().double()
    P = FR.params(sd)

    def restated(vals_list, m, target):
        cat = utils.get_concat_layers_inf(net.pyr, vals_list)
        inp = FR.normalize({"low": d(cat.low_level), "phase": [d(p) for p in cat.phase], "amp": [d(a) for a in cat.amplitude]})
        with torch.no_grad():
            low, phases, amps = FR.walk(P, inp, m, num_img)
        ph, am = [0] * (L - m) + phases[::-1], [0] * (L - m) + amps[::-1]           # finest first
        if target is not None:                      # architecture.py:58-60: exchange_vals(.., 0, calc_pyr_height - m), which
            for k in range(0, min(height - m, L)):  # covers the L - m levels the walk left out (and two more)
                ph[k], am[k] = d(target.phase[k]), d(target.amplitude[k])
        return PR.reconstruct64(spec, PR.polar_to_coeff(torch.zeros((3, 1, h, w), dtype=torch.float64), ph, am, low))

    # m = None: the fused route (the analysis writes the block-input buffers)
    pred, vals_pred, target = net(img[:3 * num_img])
    assert target is None and pred.shape == (3, h, w) and len(vals_pred.phase) == L
    ref = restated(utils.separate_vals(net.pyr.filter(img[:3 * num_img]), num_img), L, None)
    err, scale = _maxerr(pred, ref), max(1.0, float(ref.abs().max()))
    print(f"architecture num_img={num_img} m=None: err {err:.3e} / scale {scale:.3f}")
    assert err <= 2e-4 * scale
    # m = 2 with a target: the hierarchical form (every band level then comes from the target; m = 5 keeps three predicted)
    vals_list = utils.separate_vals(net.pyr.filter(img), num_img + 1)
    for m in (2, 5):
        pred_m, vals_m, tgt = net(img, m=m)
        assert tgt is not None and pred_m.shape == (3, h, w)
        ref_m = restated(vals_list[:-1], m, vals_list[-1])
        err, scale = _maxerr(pred_m, ref_m), max(1.0, float(ref_m.abs().max()))
        print(f"architecture num_img={num_img} m={m}: err {err:.3e} / scale {scale:.3f}")
        assert err <= 2e-4 * scale


# ---- PyramidFusionInterpolator ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _adacof(device):
    from vfi_amd.adacof.models import Model
    net = Model(types.SimpleNamespace(model="vfi_amd.fusion_net.fusion_adacofnet", kernel_size=5, dilation=1, gpu_id=0))
    net.load(pipeline_cpu.seeded_weights(0)["adacof"])
    net.eval()
    return net


@pytest.mark.parametrize("model", [1, 2])
def test_pyramid_fusion_interpolator_equals_its_steps(model, device):
    from vfi_amd.fusion_net.interpolate_pyramid_fusion import PyramidFusionInterpolator
    h, w = 64, 96
    num_img = {1: 4, 2: 3}[model]
    a0, _, a2 = (torch.from_numpy(x).to(device) for x in synth.translating_pair(7, h, w))
    adacof = _adacof(device)
    sd = FR.net_state(13, num_img)
    runner = PyramidFusionInterpolator(adacof, model, sd, device)
    out = runner(a0, a2)
    assert set(out) == {"fusion_pred", "ada_pred", "flow_var_map"}
    assert out["fusion_pred"].shape == (1, 3, h, w) and torch.isfinite(out["fusion_pred"]).all()
    # the same steps from the public pieces
    with torch.no_grad():
        o1, o2, ada, mask = adacof(a0.unsqueeze(0), a2.unsqueeze(0))
        images = (a0, a2, o1[0], o2[0]) if model == 1 else (a0, a2, ada[0])
        lab = torch.cat([ops.rgb2lab(t) for t in images], 0)
        height = utils.calc_pyr_height(torch.empty(3, h, w, device="meta"))
        pyr = Pyramid(height, 4, np.sqrt(2), device)
        pyr.set_full_size(h, w)
        net = PhaseNet(pyr, device, num_img=num_img)
        net.load_state_dict(sd)
        vals, bufs, amp_max = pyr.filter(lab, concat_frames=num_img, phase_scale=1.0 / math.pi, amp_max_eps=net.eps,
                                         pred_channels=net.pred_channels)
        vp = net(net.normalize_vals(vals, concat=bufs, amp_max=amp_max))
        want = ops.lab2rgb(pyr.inv_filter(DecompValues(0, vp.phase, vp.amplitude, vp.low_level))).unsqueeze(0)
    assert torch.equal(out["ada_pred"], ada) and torch.equal(out["flow_var_map"], mask)
    assert torch.equal(out["fusion_pred"], want)
    assert torch.equal(runner(a0, a2)["fusion_pred"], want)                  # the cached per-size state gives the same frame
    high = runner(a0, a2, high_level=True)["fusion_pred"]
    assert torch.isfinite(high).all() and not torch.equal(high, want)
    with pytest.raises(ValueError):
        PyramidFusionInterpolator(adacof, 3, sd, device)


# ---- the two-image route is untouched ----------------------------------------------------------------------------------------
def test_two_image_forward_issues_the_same_calls_as_before(device):
    import phasenet_walk_ref as W
    n, h, w, height = 3, 32, 48, 6
    net = PhaseNet(types.SimpleNamespace(height=height, nbands=4), device)
    net.load_state_dict(W.net_state(3))
    inp = FR.raw_inputs(5, n, h, w, height, 2)
    normed = net.normalize_vals(_device_vals(inp, device))
    net(normed)                                      # builds the packs
    _lib.PROFILE = rec = _lib.Recorder()
    try:
        net(normed)
    finally:
        _lib.PROFILE = None
    calls = [row[0] for row in rec.rows]
    assert calls.count("vfi_phasenet_predict") == height - 2 and calls.count("vfi_phasenet_emit_low") == 1
    assert not [c for c in calls if c.endswith("_n")]
    # ... and the fusion variants issue the new ones
    net3 = PhaseNet(types.SimpleNamespace(height=height, nbands=4), device, num_img=3)
    net3.load_state_dict(FR.net_state(3, 3))
    normed3 = net3.normalize_vals(_device_vals(FR.raw_inputs(5, n, h, w, height, 3), device))
    net3(normed3)
    _lib.PROFILE = rec = _lib.Recorder()
    try:
        net3(normed3)
    finally:
        _lib.PROFILE = None
    calls = [row[0] for row in rec.rows]
    assert calls.count("vfi_phasenet_emit_low_n") == 1 and "vfi_phasenet_predict" not in calls and "vfi_phasenet_emit_low" not in calls
    assert calls.count("vfi_phasenet_predict_n") == height - 2
