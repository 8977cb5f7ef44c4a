"""Pyramid calls of more images than a plan holds.

A plan's workspace holds at most 16 images; the library walks a longer call in slices of that many, each through the passes
of a call of that size, with a plane map that addresses the caller's tensors of the whole call.  So a call of N images must
give, bit for bit, what the same function gives on [0:16], [16:32], [32:N] of the same Pyramid object (same plan, same slice
boundaries: which small levels an analysis batches depends on a slice's image count), and must stay within the float64
bounds of tests/test_pyramid_gpu.py, test_pyramid_backward_gpu.py and test_pyramid_analysis_backward_gpu.py.

Frames, from tests/test_pyramid_paths_gpu.py: 128x100 and 100x128 at height 10 (wave rows and both wave column passes,
Bluestein forms, small levels batched by multi_levels), 7x45 (generic engine only) and 31x13.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import pyramid_cpu, synth
from vfi_amd._lib import VfiLibraryError
from vfi_amd.steerable.SCFpyr_PyTorch import BAND_MAJOR, COMPLEX_COEFF, Plan
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.values import DecompValues

import pyramid_ana_grad_ref as ana_ref
import pyramid_grad_ref as syn_ref

pytestmark = pytest.mark.gpu

S2 = math.sqrt(2)
NB = 4
FRAMES = [(128, 100, 10), (100, 128, 10), (7, 45, 3), (31, 13, 4)]
IDS = [f"{h}x{w}" for h, w, _ in FRAMES]
CAP = 16                       # images per slice of the plans that Pyramid / SCFpyr_PyTorch build for N >= 16


@functools.lru_cache(maxsize=None)
def _pyr(height, device):
    """One Pyramid per height for the whole module: the bit-identity cases need the plan of the long call."""
    return Pyramid(height, NB, S2, device)


@functools.lru_cache(maxsize=None)
def _spec(h, w, height):
    return pyramid_cpu.PyramidSpec(h, w, height)


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).random(tuple(shape), dtype=np.float32))


def _randn(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(shape)).astype(np.float32))


def _slices(n, cap=CAP):
    return [(a, min(a + cap, n)) for a in range(0, n, cap)]


def _to(v, device):
    return DecompValues(v.high_level.to(device), [p.to(device) for p in v.phase], [a.to(device) for a in v.amplitude], v.low_level.to(device))


def _cut(v, a, b):
    """images [a, b) of per-image values"""
    return DecompValues(v.high_level[a:b], [p[a * NB:b * NB] for p in v.phase], [x[a * NB:b * NB] for x in v.amplitude], v.low_level[a:b])


def _flat(v):
    return [v.high_level, *v.phase, *v.amplitude, v.low_level]


def _cat_vals(parts):
    return [torch.cat(ts, 0) for ts in zip(*(_flat(p) for p in parts))]


def _assert_equal(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and not torch.isnan(a).any(), (what, i)
        assert torch.equal(a, b), (what, i, float((a - b).abs().max()))


# ---- 1. bit identity, per-image layout ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 32, 33])
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_per_image_calls_equal_their_slices(frame, n, device):
    h, w, height = frame
    pyr = _pyr(height, device)
    img = _rand((n, h, w), 1).to(device)
    whole = pyr.filter(img)
    assert pyr.pyr.plan(h, w, n).max_images == CAP
    _assert_equal(_flat(whole), _cat_vals([pyr.filter(img[a:b]) for a, b in _slices(n)]), "filter")
    v = _to(synth.synthetic_vals(3, n, h, w, height), device)
    _assert_equal([pyr.inv_filter(v)], [torch.cat([pyr.inv_filter(_cut(v, a, b)) for a, b in _slices(n)], 0)], "inv_filter")
    for mask, hi, lo in ((1, True, False), ((1 << (height - 2)) - 2, False, True)):
        _assert_equal([pyr.band_filter(img, mask, keep_high=hi, keep_low=lo)],
                      [torch.cat([pyr.band_filter(img[a:b], mask, keep_high=hi, keep_low=lo) for a, b in _slices(n)], 0)], "band_filter")


@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_band_filter_pair_equals_its_slices_of_eight(frame, n, device):
    h, w, height = frame
    pyr = _pyr(height, device)
    a_img, b_img = _rand((n, h, w), 2).to(device), _rand((n, h, w), 3).to(device)
    full = (1 << (height - 2)) - 1
    sa, sb = dict(level_mask=full & 3, keep_low=True), dict(level_mask=full & ~3, keep_high=True)
    whole = pyr.band_filter_pair(a_img, sa, b_img, sb)
    assert pyr.pyr.plan(h, w, 2 * n).max_images == CAP
    parts = [pyr.band_filter_pair(a_img[a:b], sa, b_img[a:b], sb) for a, b in _slices(n, CAP // 2)]
    _assert_equal([whole], [torch.cat(parts, 0)], "band_filter_pair")
    # ... and it is the sum of the two single filters (float64 bound of test_pyramid_gpu.py's band filter, once per term)
    two = pyr.band_filter(a_img, sa["level_mask"], keep_low=True) + pyr.band_filter(b_img, sb["level_mask"], keep_high=True)
    assert float((whole - two).abs().max()) <= 4e-5


# ---- 2. bit identity, complex band-major layout (build / reconstruct) -------------------------------------------------------------
def _coeff_cat(parts):
    nlev = len(parts[0]) - 2
    return [torch.cat([p[0] for p in parts], 0)] + [[torch.cat([p[1 + k][b] for p in parts], 0) for b in range(NB)] for k in range(nlev)] + \
        [torch.cat([p[-1] for p in parts], 0)]


def _coeff_flat(c):
    return [c[0]] + [b for lv in c[1:-1] for b in lv] + [c[-1]]


@pytest.mark.parametrize("n", [17, 33])
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_build_and_reconstruct_equal_their_slices(frame, n, device):
    """A band-major tensor's bands lie N planes apart -- the call's N, not the slice's."""
    h, w, height = frame
    scf = _pyr(height, device).pyr
    x = _rand((n, 1, h, w), 4).to(device)
    whole = scf.build(x)
    assert tuple(whole[1][0].shape) == (n, h, w, 2)
    _assert_equal(_coeff_flat(whole), _coeff_flat(_coeff_cat([scf.build(x[a:b]) for a, b in _slices(n)])), "build")
    # arbitrary (non-analytic) coefficients
    coeff = [_randn(whole[0].shape, 5).to(device)] + [[_randn(b.shape, 10 * k + i).to(device) for i, b in enumerate(lv)]
                                                       for k, lv in enumerate(whole[1:-1])] + [_randn(whole[-1].shape, 6).to(device)]
    cut = lambda a, b: [coeff[0][a:b]] + [[z[a:b] for z in lv] for lv in coeff[1:-1]] + [coeff[-1][a:b]]
    _assert_equal([scf.reconstruct(coeff)], [torch.cat([scf.reconstruct(cut(a, b)) for a, b in _slices(n)], 0)], "reconstruct")
    # the gradients of both, through the same layout
    leaf = x.clone().requires_grad_()
    gz = [_randn(t.shape, 30 + i).to(device) for i, t in enumerate(_coeff_flat(whole))]
    torch.autograd.backward(_coeff_flat(scf.build(leaf)), gz)
    parts = []
    for a, b in _slices(n):
        lf = x[a:b].clone().requires_grad_()
        torch.autograd.backward(_coeff_flat(scf.build(lf)), [g[a:b] for g in gz])
        parts.append(lf.grad)
    _assert_equal([leaf.grad], [torch.cat(parts, 0)], "build backward")
    g = _randn((n, h, w), 7).to(device)
    leaves = [t.clone().requires_grad_() for t in _coeff_flat(coeff)]
    unflat = lambda f: [f[0]] + [list(f[1 + k * NB:1 + (k + 1) * NB]) for k in range(height - 2)] + [f[-1]]
    got = torch.autograd.grad(scf.reconstruct(unflat(leaves)), leaves, g)
    parts = []
    for a, b in _slices(n):
        lv = [t[a:b].clone().requires_grad_() for t in _coeff_flat(coeff)]
        parts.append(torch.autograd.grad(scf.reconstruct(unflat(lv)), lv, g[a:b]))
    _assert_equal(list(got), [torch.cat(ts, 0) for ts in zip(*parts)], "reconstruct backward")


# ---- direct calls on a Plan ---------------------------------------------------------------------------------------------------------
def _new(shape, device, pad=0):
    """-> (tensor, its NaN-filled container, pad): the tensor sits `pad` leading-axis entries inside the container"""
    box = torch.full((shape[0] + 2 * pad, *shape[1:]), float("nan"), dtype=torch.float32, device=device)
    return box[pad:pad + shape[0]], box, pad


def _assert_canaries(pairs, what):
    for i, (t, box, pad) in enumerate(pairs):
        assert not torch.isnan(t).any(), (what, i, "NaN inside")
        assert box.shape[0] == t.shape[0] + 2 * pad and pad > 0
        assert bool(torch.isnan(box[:pad]).all()) and bool(torch.isnan(box[pad + t.shape[0]:]).all()), (what, i, "write outside the output")


def _plan_analyze(plan, img, table=None, flags=0, pad=0):
    """Plan.analyze into fresh outputs -> (flat outputs [high, phase.., amp.., low], their (tensor, container, pad) triples)"""
    n, nlev, dev = img.shape[0], plan.height - 2, img.device
    last = (2,) if flags & COMPLEX_COEFF else ()
    pairs = [_new((n, plan.h, plan.w), dev, pad)]
    pairs += [_new((n * NB, *plan.sizes[k], *last), dev, pad * NB) for k in range(nlev)]
    if not flags & COMPLEX_COEFF:
        pairs += [_new((n * NB, *plan.sizes[k]), dev, pad * NB) for k in range(nlev)]
    pairs.append(_new((n, *plan.sizes[nlev]), dev, pad))
    outs = [p[0] for p in pairs]
    amp = outs[1 + nlev:1 + 2 * nlev] if not flags & COMPLEX_COEFF else None
    plan.analyze(img, outs[0], outs[1:1 + nlev], amp, table, outs[-1], 1.0, (1 << nlev) - 1, flags)
    return outs, pairs


# ---- 3. small capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_plan_of_six_images_walks_thirteen(frame, device):
    h, w, height = frame
    plan = Plan(h, w, height, NB, S2, 6, device)
    nlev = height - 2
    img = _rand((13, h, w), 8).to(device)
    whole, _ = _plan_analyze(plan, img)
    cat = lambda parts: [torch.cat(ts, 0) for ts in zip(*parts)]
    _assert_equal(whole, cat([_plan_analyze(plan, img[a:b])[0] for a, b in _slices(13, 6)]), "analyze 6/6/1")
    # N = 6 and N = 1 are one slice each, as they always were: the first and the last slice of the walk
    six, one = _plan_analyze(plan, img[:6])[0], _plan_analyze(plan, img[12:])[0]
    per = lambda t: t.shape[0] // 13
    _assert_equal(six, [t[:6 * per(t)] for t in whole], "N = 6")
    _assert_equal(one, [t[12 * per(t):] for t in whole], "N = 1")
    canary = _new((13, h, w), device, 1)
    out = canary[0]
    plan.synthesize(whole[0], whole[1:1 + nlev], whole[1 + nlev:1 + 2 * nlev], None, whole[-1], (1 << nlev) - 1, 0, out)
    _assert_canaries([canary], "synthesize")
    parts = []
    for a, b in _slices(13, 6):
        o = torch.empty((b - a, h, w), dtype=torch.float32, device=device)
        plan.synthesize(whole[0][a:b], [t[a * NB:b * NB] for t in whole[1:1 + nlev]], [t[a * NB:b * NB] for t in whole[1 + nlev:1 + 2 * nlev]],
                        None, whole[-1][a:b], (1 << nlev) - 1, 0, o)
        parts.append(o)
    _assert_equal([out], [torch.cat(parts, 0)], "synthesize 6/6/1")
    psnr = 10 * math.log10(1.0 / max(float(((out - img) ** 2).mean()), 1e-30))
    assert psnr >= 90.0, psnr
    # filters: slices of 6, and of 3 images of each set for the pair
    fa = plan.band_filter(img, 1, True, False)
    _assert_equal([fa], [torch.cat([plan.band_filter(img[a:b].contiguous(), 1, True, False) for a, b in _slices(13, 6)], 0)], "band_filter 6/6/1")
    other = _rand((13, h, w), 9).to(device)
    fp = plan.band_filter_pair(img, (1, True, False), other, (2, False, True))
    _assert_equal([fp], [torch.cat([plan.band_filter_pair(img[a:b].contiguous(), (1, True, False), other[a:b].contiguous(), (2, False, True))
                                    for a, b in _slices(13, 3)], 0)], "band_filter_pair 3/3/3/3/1")


# ---- 4. a caller's plane_index ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_plane_index_table_of_twenty_images(frame, device):
    """The table has N entries per level -- the call's N -- and a different permutation at every level."""
    h, w, height = frame
    n, nlev = 20, height - 2
    plan = _pyr(height, device).pyr.plan(h, w, n)
    img = _rand((n, h, w), 11).to(device)
    plain, _ = _plan_analyze(plan, img)
    perms = [np.random.default_rng(50 + k).permutation(n) for k in range(nlev)]
    table = [int(perms[k][d]) * NB for k in range(nlev) for d in range(n)]
    got, pairs = _plan_analyze(plan, img, table=table, pad=1)
    _assert_canaries(pairs, "analyze with a table")
    assert torch.equal(got[0], plain[0]) and torch.equal(got[-1], plain[-1])
    for k in range(nlev):
        src = torch.from_numpy(perms[k]).to(device)
        for j in (1 + k, 1 + nlev + k):              # image d's planes land at slot perms[k][d]
            a, b = got[j].view(n, NB, *plan.sizes[k]), plain[j].view(n, NB, *plan.sizes[k])
            assert torch.equal(a[src], b), (k, j)
    mask = (1 << nlev) - 1
    want = torch.empty((n, h, w), dtype=torch.float32, device=device)
    plan.synthesize(plain[0], plain[1:1 + nlev], plain[1 + nlev:1 + 2 * nlev], None, plain[-1], mask, 0, want)
    canary = _new((n, h, w), device, 1)
    out = canary[0]
    plan.synthesize(got[0], got[1:1 + nlev], got[1 + nlev:1 + 2 * nlev], table, got[-1], mask, 0, out)
    _assert_canaries([canary], "synthesize with a table")
    assert torch.equal(out, want)


# ---- 5. float64 parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_seventeen_images_against_float64(frame, device):
    h, w, height = frame
    n, spec, pyr = 17, _spec(h, w, height), _pyr(height, device)
    img = _rand((n, h, w), 1)
    high, phase, amp, low = ana_ref.analyze64(spec, img)
    got = pyr.filter(img.to(device))
    err_h, err_l = (got.high_level.cpu() - high).abs().max().item(), (got.low_level.cpu() - low).abs().max().item()
    print(f"{h}x{w}: high err {err_h:.2e}, low err {err_l:.2e}")
    assert err_h <= 2e-5
    assert err_l <= 2e-5 * max(1.0, low.abs().max().item())
    for k in range(height - 2):                      # test_pyramid_gpu.py::test_filter_matches_oracle's criterion
        a, p = got.amplitude[k].cpu().double(), got.phase[k].cpu().double()
        scale = max(1e-3, amp[k].max().item())
        err_a = (a - amp[k]).abs().max().item()
        err_z = (torch.polar(a, p) - torch.polar(amp[k], phase[k])).abs().max().item()
        print(f"{h}x{w} level {k}: amplitude err {err_a / scale:.2e}, coefficient err {err_z / scale:.2e} of the largest amplitude")
        assert err_a <= 3e-5 * scale and err_z <= 5e-5 * scale, k
        assert got.phase[k].abs().max().item() <= math.pi + 1e-6
    v = synth.synthetic_vals(3, n, h, w, height)
    want = syn_ref.reconstruct64(spec, syn_ref.polar_to_coeff(v.high_level.double(), [p.double() for p in v.phase],
                                                              [a.double() for a in v.amplitude], v.low_level.double()))
    err = (pyr.inv_filter(_to(v, device)).cpu() - want).abs().max().item()
    print(f"{h}x{w}: synthesis err {err:.2e}, max|image| {want.abs().max().item():.2e}")
    assert err <= 1e-4 * max(1.0, want.abs().max().item())
    rec = pyr.inv_filter(got).cpu()
    psnr = 10 * math.log10(1.0 / max(float(((rec - img) ** 2).mean()), 1e-30))
    assert psnr >= 90.0, psnr


# ---- 6. gradients -----------------------------------------------------------------------------------------------------------------------------------
def _close(got, want, what, rel=1e-4):
    """|got - want| <= rel * max|want|: the criterion of test_pyramid_backward_gpu.py / test_pyramid_analysis_backward_gpu.py"""
    want = want.double()
    err, scale = float((got.detach().double().cpu() - want).abs().max()), float(want.abs().max())
    print(f"{what}: max|err| {err:.3e}, max|grad| {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= rel * scale, f"{what}: max|err| {err:.3e} vs max|grad| {scale:.3e}"


@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_synthesis_backward_of_eighteen_images(frame, device):
    h, w, height = frame
    n, spec, pyr = 18, _spec(h, w, height), _pyr(height, device)
    v = synth.synthetic_vals(7, n, h, w, height)
    g = _randn((n, h, w), 5)
    leaf = lambda t: t.to(device).requires_grad_()

    def grads(a, b):
        c = _cut(v, a, b)
        leaves = [leaf(t) for t in _flat(c)]
        L = height - 2
        out = pyr.inv_filter(DecompValues(leaves[0], leaves[1:1 + L], leaves[1 + L:1 + 2 * L], leaves[-1]))
        assert out.grad_fn is not None
        return torch.autograd.grad(out, leaves, g[a:b].to(device))
    got = grads(0, n)
    _assert_equal(list(got), [torch.cat(ts, 0) for ts in zip(*(grads(a, b) for a, b in _slices(n)))], "Synthesis backward")
    rhi, rb, rlo = syn_ref.adjoint64(spec, g)
    L = spec.nlev
    _close(got[0].squeeze(1), rhi, f"{h}x{w} high")
    _close(got[-1].squeeze(1), rlo, f"{h}x{w} low")
    for k in range(L):
        wp, wa = syn_ref.polar_grads(rb[k], v.phase[k], v.amplitude[k])
        _close(got[1 + k], wp, f"{h}x{w} phase level {k}")
        _close(got[1 + L + k], wa, f"{h}x{w} amplitude level {k}")


@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_analysis_backward_of_eighteen_images(frame, device):
    h, w, height = frame
    n, spec, pyr = 18, _spec(h, w, height), _pyr(height, device)
    s = 1.0 / math.pi
    base = _rand((n, h, w), 2).to(device)
    img = base.clone().requires_grad_()
    v = pyr.filter(img, phase_scale=s)
    assert v.high_level.grad_fn is not None
    up = [_randn(t.shape, 60 + i) for i, t in enumerate(_flat(v))]
    torch.autograd.backward(_flat(v), [t.to(device) for t in up])
    parts = []
    for a, b in _slices(n):
        part = base[a:b].clone().requires_grad_()
        pv = pyr.filter(part, phase_scale=s)
        cut = _flat(_cut(DecompValues(up[0], up[1:1 + spec.nlev], up[1 + spec.nlev:1 + 2 * spec.nlev], up[-1]), a, b))
        torch.autograd.backward(_flat(pv), [t.to(device) for t in cut])
        parts.append(part.grad)
    _assert_equal([img.grad], [torch.cat(parts, 0)], "Analysis backward")
    # the GPU's own fp32 (phase, amplitude) go to the reference: the check is not conditioned by 1/A of values that differ
    L = spec.nlev
    G = [ana_ref.level_bands(ana_ref.polar_to_coeff_grad(up[1 + k], up[1 + L + k], v.phase[k].detach().cpu(), v.amplitude[k].detach().cpu(), s), n)
         for k in range(L)]
    _close(img.grad, ana_ref.analysis_adjoint64(spec, up[0].squeeze(1), G, up[-1].squeeze(1)), f"{h}x{w} image gradient")


@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_band_filter_backward_of_eighteen_images(frame, device):
    """The filters are self-adjoint: the gradient is the same filter applied to the upstream gradient."""
    h, w, height = frame
    n, pyr = 18, _pyr(height, device)
    a_img, b_img = _rand((n, h, w), 12).to(device), _rand((n, h, w), 13).to(device)
    g = _randn((n, h, w), 14).to(device)
    x = a_img.clone().requires_grad_()
    out = pyr.band_filter(x, 1, keep_high=True)
    assert out.grad_fn is not None
    out.backward(g)
    want = torch.cat([pyr.band_filter(g[a:b], 1, keep_high=True) for a, b in _slices(n)], 0)
    _assert_equal([x.grad], [want], "BandFilter backward")
    sa, sb = dict(level_mask=1, keep_high=True), dict(level_mask=2, keep_low=True)
    xa, xb = a_img.clone().requires_grad_(), b_img.clone().requires_grad_()
    pyr.band_filter_pair(xa, sa, xb, sb).backward(g)
    _assert_equal([xa.grad], [want], "BandFilter pair backward, first set")
    _assert_equal([xb.grad], [torch.cat([pyr.band_filter(g[a:b], 2, keep_low=True) for a, b in _slices(n)], 0)], "BandFilter pair backward, second set")
    # float64: <x, F y> = <F x, y> for a self-adjoint F
    lhs = float((a_img.double() * x.grad.double()).sum())
    rhs = float((out.detach().double() * g.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(rhs)), (lhs, rhs)


# ---- 7. output canaries ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, BAND_MAJOR | COMPLEX_COEFF], ids=["per-image", "band-major-complex"])
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_outputs_inside_nan_buffers_keep_their_surroundings(frame, flags, device):
    """A slice that writes with a wrong base lands outside its output, or leaves NaNs inside it."""
    h, w, height = frame
    n, nlev = 19, height - 2
    plan = _pyr(height, device).pyr.plan(h, w, n)
    img = _rand((n, h, w), 15).to(device)
    outs, pairs = _plan_analyze(plan, img, flags=flags, pad=2)
    _assert_canaries(pairs, "analyze")
    canary = _new((n, h, w), device, 2)
    out = canary[0]
    amp = outs[1 + nlev:1 + 2 * nlev] if not flags & COMPLEX_COEFF else None
    plan.synthesize(outs[0], outs[1:1 + nlev], amp, None, outs[-1], (1 << nlev) - 1, flags, out)
    _assert_canaries([canary], "synthesize")
    psnr = 10 * math.log10(1.0 / max(float(((out - img) ** 2).mean()), 1e-30))
    assert psnr >= 90.0, psnr


# ---- 8. what stays capped ----------------------------------------------------------------------------------------------------------------------------------
def test_analyze_max_keeps_the_capacity_of_one_slice(device):
    h, w, height = 31, 13, 4
    plan = Plan(h, w, height, NB, S2, 6, device)
    nlev, n = height - 2, 8
    img = _rand((n, h, w), 16).to(device)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=device)
    high, low = nan(n, h, w), nan(n, *plan.sizes[nlev])
    phase, amp = [nan(n * NB, *plan.sizes[k]) for k in range(nlev)], [nan(n * NB, *plan.sizes[k]) for k in range(nlev)]
    amp_max, amp_max3 = nan(nlev, 4), nan(nlev, 3)
    with pytest.raises(VfiLibraryError, match="N=8"):
        plan.analyze(img, high, phase, amp, None, low, 1.0, (1 << nlev) - 1, 0, amp_max=amp_max, groups=4, eps=1e-8)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in [high, low, amp_max, *phase, *amp])
    with pytest.raises(VfiLibraryError):
        plan.multi_levels(7, (1 << nlev) - 1)
    assert plan.multi_levels(6, (1 << nlev) - 1) == plan.multi_levels(6, (1 << nlev) - 1)
    # within the capacity it answers as before
    plan.analyze(img[:6], high[:6], [p[:6 * NB] for p in phase], [a[:6 * NB] for a in amp], None, low[:6], 1.0, (1 << nlev) - 1, 0,
                 amp_max=amp_max3, groups=3, eps=1e-8)
    assert not torch.isnan(amp_max3).any() and torch.isnan(amp_max).all() and torch.isnan(high[6:]).all() and not torch.isnan(high[:6]).any()
    with pytest.raises(VfiLibraryError, match="at most 16"):
        Pyramid(height, NB, S2, device).filter(_rand((18, h, w), 17).to(device), concat_frames=2)
