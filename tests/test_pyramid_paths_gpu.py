"""Every wave-engine instantiation of the pyramid's passes, run on the GPU against float64.

A level's row pass, analysis column pass and synthesis column pass each pick one of the configurations of
csrc/vfi_wfft_configs.h (plain or in Bluestein's form) or fall back to the generic LDS engine, and each of the eight pass
files (csrc/vfi_pyrw_*.hip) instantiates its own kernel per configuration.  FRAMES is a set of small frames that, between
them, send every reachable (pass file, engine length, plain / Bluestein) through forward analysis, forward synthesis and
both backward passes; which path a size takes is read from the library (Plan.pass_info / Plan.multi_levels), never
restated here.  A full analysis batches its small levels onto the generic engine (multi_levels), so every level it would
batch also runs once alone, with a single-level mask.  References: the float64 restatements tests/pyramid_ana_grad_ref.py
(analysis and its adjoint) and tests/pyramid_grad_ref.py (synthesis and its adjoint), which the host tests pin against the
oracle; bounds: those of tests/test_pyramid_gpu.py, test_pyramid_backward_gpu.py and test_pyramid_analysis_backward_gpu.py."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG_DIR
from oracle import pyramid_cpu, synth
from vfi_amd.train.pyramid import Pyramid
from vfi_amd.values import DecompValues

import pyramid_ana_grad_ref as ana_ref
import pyramid_grad_ref as syn_ref

S2 = math.sqrt(2)

# (H, W, pyramid height, N, claims): claims = (size index, pass, engine length, Bluestein) that the frame is on the table
# for -- size index k < height-2 is band level k, height-2 the low residual, height-1 the frame itself; every test asserts
# them through the queries before it compares anything.  Skinny frames keep the long lengths cheap; N = 3 gives N * 4 * h
# rows, not a multiple of the 8 .. 64 lines per batch of the row configurations wherever h allows it, and the widths leave a
# partial last batch of columns.  The first six are there for the generic engine (test_generic_engine_kinds).
FRAMES = [
    (400, 23, 6, 3, [(0, 'rows', 48, 1), (1, 'ana_cols', 768, 1), (1, 'syn_cols', 768, 1), (2, 'rows', 12, 0), (3, 'ana_cols', 384, 1), (3, 'syn_cols', 384, 1), (5, 'rows', 48, 1)]),
    (1000, 12, 4, 3, [(1, 'ana_cols', 1536, 1), (1, 'syn_cols', 1536, 1), (3, 'rows', 12, 0)]),
    (128, 100, 10, 3, [(0, 'ana_cols', 128, 0), (0, 'syn_cols', 128, 0), (1, 'rows', 192, 1), (1, 'ana_cols', 192, 1), (1, 'syn_cols', 192, 1), (2, 'ana_cols', 64, 0), (2, 'syn_cols', 64, 0), (3, 'ana_cols', 96, 1), (3, 'syn_cols', 96, 1), (4, 'ana_cols', 32, 0), (4, 'syn_cols', 32, 0), (5, 'ana_cols', 48, 1), (5, 'syn_cols', 48, 1), (6, 'rows', 32, 1), (6, 'ana_cols', 16, 0), (6, 'syn_cols', 16, 0), (7, 'ana_cols', 12, 0), (7, 'syn_cols', 12, 0), (8, 'rows', 16, 1), (9, 'ana_cols', 128, 0)]),
    (100, 128, 10, 3, [(0, 'rows', 128, 0), (2, 'rows', 64, 0), (3, 'rows', 96, 1), (4, 'rows', 32, 0), (6, 'rows', 16, 0), (6, 'ana_cols', 32, 1), (6, 'syn_cols', 32, 1), (8, 'ana_cols', 16, 1), (9, 'rows', 128, 0)]),
    (1087, 16, 4, 3, [(2, 'ana_cols', 1536, 1), (3, 'rows', 16, 0)]),
    (16, 2039, 4, 3, [(1, 'rows', 3072, 1), (2, 'rows', 2048, 1), (3, 'ana_cols', 16, 0)]),
    (7, 16, 3, 3, [(0, 'ana_cols', 16, 1), (0, 'syn_cols', 16, 1)]),
    (7, 30, 3, 3, [(0, 'rows', 30, 0), (2, 'rows', 30, 0)]),
    (7, 45, 3, 3, [(0, 'rows', 45, 0), (1, 'rows', 32, 0), (2, 'rows', 45, 0)]),
    (45, 7, 3, 3, [(0, 'rows', 16, 1), (0, 'ana_cols', 45, 0), (0, 'syn_cols', 45, 0), (1, 'ana_cols', 32, 0), (2, 'ana_cols', 45, 0)]),
    (31, 13, 4, 3, [(0, 'ana_cols', 64, 1), (0, 'syn_cols', 64, 1), (3, 'rows', 32, 1), (3, 'ana_cols', 64, 1)]),
    (11, 40, 3, 3, [(0, 'rows', 40, 0), (0, 'ana_cols', 24, 1), (0, 'syn_cols', 24, 1), (1, 'rows', 64, 1), (2, 'rows', 40, 0), (2, 'ana_cols', 24, 1)]),
    (7, 67, 3, 3, [(1, 'rows', 48, 0), (2, 'rows', 192, 1)]),
    (7, 80, 3, 3, [(0, 'rows', 80, 0), (1, 'rows', 128, 1), (2, 'rows', 80, 0)]),
    (7, 136, 3, 3, [(0, 'rows', 384, 1), (1, 'rows', 256, 1), (2, 'rows', 384, 1)]),
    (12, 128, 4, 3, [(2, 'rows', 64, 0), (3, 'ana_cols', 12, 0)]),
    (7, 226, 3, 3, [(0, 'rows', 512, 1), (1, 'rows', 160, 0), (2, 'rows', 512, 1)]),
    (135, 15, 4, 3, [(0, 'rows', 15, 0), (0, 'ana_cols', 135, 0), (0, 'syn_cols', 135, 0), (1, 'rows', 24, 1), (1, 'ana_cols', 96, 0), (1, 'syn_cols', 96, 0), (2, 'ana_cols', 192, 1), (3, 'rows', 15, 0), (3, 'ana_cols', 135, 0)]),
    (128, 16, 4, 3, [(2, 'ana_cols', 64, 0)]),
    (23, 240, 6, 3, [(0, 'rows', 240, 0), (2, 'rows', 120, 0), (4, 'rows', 60, 0), (5, 'rows', 240, 0), (5, 'ana_cols', 48, 1)]),
    (512, 12, 4, 3, [(0, 'ana_cols', 512, 0), (0, 'syn_cols', 512, 0), (2, 'ana_cols', 256, 0), (3, 'ana_cols', 512, 0)]),
    (540, 12, 4, 3, [(0, 'ana_cols', 540, 0), (0, 'syn_cols', 540, 0), (2, 'ana_cols', 270, 0), (3, 'ana_cols', 540, 0)]),
    (359, 24, 6, 3, [(0, 'rows', 24, 0), (1, 'ana_cols', 512, 1), (1, 'syn_cols', 512, 1), (2, 'ana_cols', 180, 0), (2, 'syn_cols', 180, 0), (3, 'ana_cols', 256, 1), (3, 'syn_cols', 256, 1), (4, 'ana_cols', 90, 0), (5, 'rows', 24, 0), (5, 'ana_cols', 768, 1)]),
    (13, 769, 4, 3, [(0, 'rows', 2048, 1), (1, 'rows', 1536, 1), (2, 'rows', 1024, 1), (3, 'ana_cols', 32, 1)]),
    (7, 1536, 3, 3, [(0, 'rows', 1536, 0), (1, 'rows', 3072, 1), (2, 'rows', 1536, 0)]),
    (13, 960, 4, 3, [(0, 'rows', 960, 0), (2, 'rows', 480, 0), (3, 'rows', 960, 0)]),
    (7, 2048, 3, 3, [(0, 'rows', 2048, 0), (2, 'rows', 2048, 0)]),
    (720, 23, 6, 3, [(0, 'ana_cols', 720, 0), (0, 'syn_cols', 720, 0), (1, 'ana_cols', 1024, 1), (1, 'syn_cols', 1024, 1), (2, 'ana_cols', 360, 0), (2, 'syn_cols', 360, 0), (4, 'ana_cols', 180, 0), (5, 'ana_cols', 720, 0)]),
    (768, 30, 6, 3, [(0, 'ana_cols', 768, 0), (0, 'syn_cols', 768, 0), (2, 'ana_cols', 384, 0), (2, 'syn_cols', 384, 0), (4, 'ana_cols', 192, 0), (5, 'ana_cols', 768, 0)]),
    (23, 1024, 6, 3, [(0, 'rows', 1024, 0), (2, 'rows', 512, 0), (3, 'rows', 768, 1), (4, 'rows', 256, 0), (5, 'rows', 1024, 0)]),
    (24, 1280, 6, 3, [(0, 'rows', 1280, 0), (0, 'ana_cols', 24, 0), (0, 'syn_cols', 24, 0), (2, 'rows', 640, 0), (3, 'rows', 1024, 1), (4, 'rows', 320, 0), (5, 'rows', 1280, 0), (5, 'ana_cols', 24, 0)]),
    (1080, 33, 7, 3, [(0, 'ana_cols', 1080, 0), (0, 'syn_cols', 1080, 0), (4, 'ana_cols', 270, 0), (4, 'syn_cols', 270, 0), (5, 'ana_cols', 384, 1), (6, 'rows', 96, 1), (6, 'ana_cols', 1080, 0)]),
    (49, 768, 8, 3, [(0, 'rows', 768, 0), (0, 'ana_cols', 128, 1), (0, 'syn_cols', 128, 1), (2, 'rows', 384, 0), (4, 'rows', 192, 0), (6, 'rows', 96, 0), (7, 'rows', 768, 0), (7, 'ana_cols', 128, 1)]),
    (385, 192, 12, 3, [(2, 'rows', 96, 0), (4, 'rows', 48, 0), (11, 'rows', 192, 0), (11, 'ana_cols', 1024, 1)]),
    (227, 640, 12, 3, [(2, 'rows', 320, 0), (4, 'rows', 160, 0), (5, 'rows', 256, 1), (7, 'rows', 128, 1), (9, 'rows', 64, 1), (10, 'rows', 20, 0), (11, 'rows', 640, 0), (11, 'ana_cols', 512, 1)]),
    (48, 3072, 8, 3, [(0, 'rows', 3072, 0), (0, 'ana_cols', 48, 0), (0, 'syn_cols', 48, 0), (6, 'rows', 384, 0), (7, 'rows', 3072, 0), (7, 'ana_cols', 48, 0)]),
    (314, 512, 13, 3, [(2, 'rows', 256, 0), (12, 'rows', 512, 0)]),
    (539, 315, 13, 3, [(8, 'rows', 20, 0), (12, 'rows', 768, 1)]),
    (360, 479, 13, 3, [(4, 'ana_cols', 90, 0), (4, 'syn_cols', 90, 0), (6, 'rows', 60, 0), (11, 'rows', 24, 1), (12, 'ana_cols', 360, 0)]),
    (1536, 115, 10, 3, [(0, 'ana_cols', 1536, 0), (0, 'syn_cols', 1536, 0), (6, 'ana_cols', 192, 0), (6, 'syn_cols', 192, 0), (8, 'ana_cols', 96, 0), (9, 'ana_cols', 1536, 0)]),
    (1024, 179, 11, 3, [(0, 'ana_cols', 1024, 0), (0, 'syn_cols', 1024, 0), (4, 'ana_cols', 256, 0), (4, 'syn_cols', 256, 0), (9, 'ana_cols', 96, 1), (10, 'ana_cols', 1024, 0)]),
    (97, 1920, 10, 3, [(0, 'rows', 1920, 0), (4, 'rows', 480, 0), (8, 'rows', 120, 0), (9, 'rows', 1920, 0), (9, 'ana_cols', 256, 1)]),
    (384, 513, 14, 3, [(13, 'rows', 1536, 1), (13, 'ana_cols', 384, 0)]),
]
IDS = [f"{f[0]}x{f[1]}" for f in FRAMES]

# Instantiations no frame can select.  Bluestein's convolution length (csrc/vfi_fft.h: bluestein_length) holds 2n - 1
# points of a length n with a prime factor above 5; the smallest such n is 7, so the length is at least 16 and the Bluestein
# form of engine length 12 is never asked for, in any pass.  (Length 16 is: a 7-row level.)
PASS_FILES = {"ROW": ("rows_ana", "rows_syn", "rows_grad", "rows_syn_grad", "gen_rows"), "COL": ("cols_ana", "gen_cols"), "SYN": ("cols_syn",)}
UNREACHABLE = {(p, 12, 1) for ps in PASS_FILES.values() for p in ps}


def _engine_lengths():
    """{"ROW" | "COL" | "SYN": [engine lengths]} as csrc/vfi_wfft_configs.h lists them (read as text)."""
    text = open(os.path.join(PKG_DIR, "csrc", "vfi_wfft_configs.h")).read()
    out = {}
    for name in PASS_FILES:
        body = text.split(f"#define VFI_WFFT_{name}_CONFIGS(X)")[1].split("#define")[0]
        out[name] = [int(m) for m in re.findall(r"\bX\((\d+),", body)]
        assert out[name] and len(set(out[name])) == len(out[name]), name
    return out


def _instantiations():
    """Every (pass file, engine length, Bluestein) the pass files instantiate: each configuration of the pass's list, and
    its Bluestein form where csrc/vfi_pyrw_dispatch.h instantiates one (blu_capable: lengths 2^k and 3 * 2^k)."""
    def blu_capable(m):
        while m % 2 == 0:
            m //= 2
        return m in (1, 3)
    return {(p, m, b) for name, passes in PASS_FILES.items() for m in _engine_lengths()[name]
            for b in ((0, 1) if blu_capable(m) else (0,)) for p in passes}


def _plan(pyr, frame):
    h, w, _, n, _ = frame
    return pyr.pyr.plan(h, w, n)


def _multi(plan, frame):
    """levels that the full analysis of the frame batches onto the generic engine; each of them alone is not batched"""
    nlev = frame[2] - 2
    multi = plan.multi_levels(frame[3], (1 << nlev) - 1)
    levels = [k for k in range(nlev) if (multi >> k) & 1]
    for k in levels:
        assert plan.multi_levels(frame[3], 1 << k) == 0, k
    return levels


def _runs(plan, frame):
    """The instantiations the tests below run for this frame, from the plan's own answers: the analysis passes (forward
    analysis, synthesis backward) of every level -- in the full call or alone --, the synthesis passes (forward synthesis,
    analysis backward) of every level, and the plain passes of the low residual's and the frame's transforms."""
    nlev = frame[2] - 2
    _multi(plan, frame)
    runs = set()
    for k in range(nlev):
        r, a, s = (plan.pass_info(k, which) for which in ("rows", "ana_cols", "syn_cols"))
        if r["M"]:
            runs |= {(p, r["M"], r["bluestein"]) for p in ("rows_ana", "rows_syn", "rows_grad", "rows_syn_grad")}
        if a["M"]:
            runs.add(("cols_ana", a["M"], a["bluestein"]))
        if s["M"]:
            runs.add(("cols_syn", s["M"], s["bluestein"]))
    for k in (nlev, nlev + 1):
        r, a = plan.pass_info(k, "rows"), plan.pass_info(k, "ana_cols")
        if r["M"]:
            runs.add(("gen_rows", r["M"], r["bluestein"]))
        if a["M"]:
            runs.add(("gen_cols", a["M"], a["bluestein"]))
    return runs


def _assert_claims(plan, frame):
    for k, which, m, blu in frame[4]:
        info = plan.pass_info(k, which)
        assert (info["M"], info["bluestein"]) == (m, blu), (frame[:2], k, which, info)


def test_table_names_only_configurations_of_the_header():
    lengths = _engine_lengths()
    assert UNREACHABLE <= _instantiations()
    for frame in FRAMES:
        for k, which, m, blu in frame[4]:
            assert 0 <= k <= frame[2] - 1 and m in lengths["ROW" if which == "rows" else "COL" if which == "ana_cols" else "SYN"]


@pytest.mark.gpu
def test_frames_cover_every_instantiation(device):
    """Plan creation only, no launch.  A configuration added to the generator fails here until a frame is added for it."""
    runs = set()
    for frame in FRAMES:
        plan = Pyramid(frame[2], 4, S2, device).pyr.plan(frame[0], frame[1], frame[3])
        _assert_claims(plan, frame)
        runs |= _runs(plan, frame)
    want = _instantiations()
    assert UNREACHABLE <= want and not (runs & UNREACHABLE), sorted(runs & UNREACHABLE)
    assert runs == want - UNREACHABLE, (sorted(want - UNREACHABLE - runs), sorted(runs - want))


@pytest.mark.gpu
def test_generic_engine_kinds(device):
    """The generic LDS engine by kind, each asserted by query."""
    frames = {f[:2]: f for f in FRAMES}
    plan = lambda h, w: Pyramid(frames[h, w][2], 4, S2, device).pyr.plan(h, w, 3)
    sub = lambda info, *keys: tuple(info[k] for k in keys)
    # a smooth length without a wave configuration, on rows and on columns; with it the mixed levels: generic rows under wave
    # columns (T stays dense, the wave column kernels address it with pitch w) and the converse
    p = plan(128, 100)
    assert sub(p.pass_info(0, "rows"), "n", "bluestein", "M") == (100, 0, 0)
    assert sub(p.pass_info(0, "ana_cols"), "M", "tpitch_ana") == (128, 100) and sub(p.pass_info(0, "syn_cols"), "M", "tpitch_syn") == (128, 100)
    # ... and a batched launch of the small levels that holds Bluestein and plain members, for rows and for columns
    multi = p.multi_levels(3, 0xff)
    assert multi == 0xff
    assert {p.pass_info(k, "rows")["bluestein"] for k in range(8)} == {0, 1} == {p.pass_info(k, "ana_cols")["bluestein"] for k in range(8)}
    p = plan(100, 128)
    assert sub(p.pass_info(0, "ana_cols"), "n", "bluestein", "M") == (100, 0, 0) and p.pass_info(0, "syn_cols")["M"] == 0
    assert sub(p.pass_info(0, "rows"), "M", "tpitch_ana", "tpitch_syn") == (128, 128, 128)
    # Bluestein on a power of two (rows) and on 3 * 2^k, whose last stage is the radix-12 one (columns)
    assert sub(plan(16, 2039).pass_info(0, "rows"), "n", "bluestein", "m", "M") == (2039, 1, 4096, 0)
    p = plan(1087, 16)
    assert sub(p.pass_info(0, "ana_cols"), "n", "bluestein", "m", "M") == (1087, 1, 3072, 0) and p.pass_info(0, "syn_cols")["M"] == 0
    assert sub(p.pass_info(1, "ana_cols"), "n", "bluestein", "m", "M") == (769, 1, 2048, 0)
    # level_tiling: 1, 2 and 4 bands per transform call, and a partial last column tile (23 columns in tiles of 8)
    assert sub(plan(1000, 12).pass_info(0, "ana_cols"), "M", "bands") == (0, 1)
    p = plan(400, 23)
    assert sub(p.pass_info(0, "ana_cols"), "M", "bands", "tile") == (0, 2, 8) and sub(p.pass_info(2, "ana_cols"), "M", "bands") == (0, 4)


# ---- references (float64, one per frame, shared by the tests and left unchanged) ------------------------------------
@functools.lru_cache(maxsize=None)
def _spec(h, w, height):
    return pyramid_cpu.PyramidSpec(h, w, height)


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).random(tuple(shape), dtype=np.float32))


def _randn(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(tuple(shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _analysis(h, w, height, n):
    img = _rand((n, h, w), 1)
    return img, ana_ref.analyze64(_spec(h, w, height), img)


def _to(v, device):
    return DecompValues(v.high_level.to(device), [p.to(device) for p in v.phase], [a.to(device) for a in v.amplitude], v.low_level.to(device))


def _level_close(phase, amp, p_ref, a_ref, what):
    """test_pyramid_gpu.py::test_filter_matches_oracle's criterion for one level"""
    a, p = amp.cpu().double(), phase.cpu().double()
    scale = max(1e-3, a_ref.max().item())
    err_a = (a - a_ref).abs().max().item()
    err_z = (torch.polar(a, p) - torch.polar(a_ref, p_ref)).abs().max().item()      # (phase wraps at +-pi are not errors)
    print(f"{what}: amplitude err {err_a / scale:.2e}, coefficient err {err_z / scale:.2e} of the largest amplitude")
    assert err_a <= 3e-5 * scale, what
    assert err_z <= 5e-5 * scale, what
    assert phase.abs().max().item() <= math.pi + 1e-6


def _close(got, want, what, rel=1e-4):
    """|got - want| <= rel * max|want|: the criterion of the gradient tests"""
    want = want.double()
    err = float((got.detach().double().cpu() - want).abs().max())
    scale = float(want.abs().max())
    print(f"{what}: max|err| {err:.3e}, max|grad| {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= rel * scale, f"{what}: max|err| {err:.3e} vs max|grad| {scale:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_filter(frame, device):
    """Forward analysis: the full mask, then every level the full mask batches, alone."""
    h, w, height, n, _ = frame
    pyr = Pyramid(height, 4, S2, device)
    plan = _plan(pyr, frame)
    _assert_claims(plan, frame)
    img, (high, phase, amp, low) = _analysis(h, w, height, n)
    got = pyr.filter(img.to(device))
    assert [tuple(p.shape) for p in got.phase] == [tuple(p.shape) for p in phase]
    err_h, err_l = (got.high_level.cpu() - high).abs().max().item(), (got.low_level.cpu() - low).abs().max().item()
    print(f"{h}x{w}: high err {err_h:.2e}, low err {err_l:.2e} (max|low| {low.abs().max().item():.2e})")
    assert err_h <= 2e-5
    assert err_l <= 2e-5 * max(1.0, low.abs().max().item())
    for k in range(height - 2):
        _level_close(got.phase[k], got.amplitude[k], phase[k], amp[k], f"{h}x{w} level {k}")
    for k in _multi(plan, frame):
        one = pyr.filter(img.to(device), level_mask=1 << k, want_high=False, want_low=False)
        _level_close(one.phase[k], one.amplitude[k], phase[k], amp[k], f"{h}x{w} level {k} alone")


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_inv_filter(frame, device):
    """Forward synthesis of arbitrary (non-analytic) values, and the round trip."""
    h, w, height, n, _ = frame
    pyr = Pyramid(height, 4, S2, device)
    _assert_claims(_plan(pyr, frame), frame)
    v = synth.synthetic_vals(3, n, h, w, height)
    want = syn_ref.reconstruct64(_spec(h, w, height), syn_ref.polar_to_coeff(v.high_level.double(), [p.double() for p in v.phase],
                                                                             [a.double() for a in v.amplitude], v.low_level.double()))
    err = (pyr.inv_filter(_to(v, device)).cpu() - want).abs().max().item()
    print(f"{h}x{w}: synthesis err {err:.2e}, max|image| {want.abs().max().item():.2e}")
    assert err <= 1e-4 * max(1.0, want.abs().max().item())
    img = _analysis(h, w, height, n)[0]
    rec = pyr.inv_filter(pyr.filter(img.to(device))).cpu()
    psnr = 10 * math.log10(1.0 / max(float(((rec - img) ** 2).mean()), 1e-30))
    print(f"{h}x{w}: round trip {psnr:.1f} dB")
    assert psnr >= 90.0


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_synthesis_backward(frame, device):
    """vfi_pyr_synthesize_backward (the analysis passes with the gradient epilogue): every input's gradient at once, then
    the gradients of every level the full call batches, alone."""
    h, w, height, n, _ = frame
    spec = _spec(h, w, height)
    pyr = Pyramid(height, 4, S2, device)
    plan = _plan(pyr, frame)
    _assert_claims(plan, frame)
    v = synth.synthetic_vals(7, n, h, w, height)
    g = _randn((n, h, w), 5)
    leaf = lambda t: t.to(device).requires_grad_()
    high, low = leaf(v.high_level), leaf(v.low_level)
    phase, amp = [leaf(p) for p in v.phase], [leaf(a) for a in v.amplitude]
    out = pyr.inv_filter(DecompValues(high, phase, amp, low))
    grads = torch.autograd.grad(out, [high, low, *phase, *amp], g.to(device))
    rhi, rb, rlo = syn_ref.adjoint64(spec, g)
    want = [syn_ref.polar_grads(rb[k], v.phase[k], v.amplitude[k]) for k in range(spec.nlev)]
    _close(grads[0].squeeze(1), rhi, f"{h}x{w} high")
    _close(grads[1].squeeze(1), rlo, f"{h}x{w} low")
    for k in range(spec.nlev):
        _close(grads[2 + k], want[k][0], f"{h}x{w} phase level {k}")
        _close(grads[2 + spec.nlev + k], want[k][1], f"{h}x{w} amplitude level {k}")
    for k in _multi(plan, frame):      # (only level k's planes require a gradient: the backward's level mask is 1 << k)
        dv = _to(v, device)
        dv.phase[k], dv.amplitude[k] = leaf(v.phase[k]), leaf(v.amplitude[k])
        gp, ga = torch.autograd.grad(pyr.inv_filter(dv), [dv.phase[k], dv.amplitude[k]], g.to(device))
        _close(gp, want[k][0], f"{h}x{w} phase level {k} alone")
        _close(ga, want[k][1], f"{h}x{w} amplitude level {k} alone")


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_analysis_backward(frame, device):
    """vfi_pyr_analyze_backward (the synthesis passes with the gradient prologue), phase scale 1 / pi."""
    h, w, height, n, _ = frame
    spec = _spec(h, w, height)
    pyr = Pyramid(height, 4, S2, device)
    _assert_claims(_plan(pyr, frame), frame)
    s = 1.0 / math.pi
    img = _rand((n, h, w), 2).to(device).requires_grad_()
    v = pyr.filter(img, phase_scale=s)
    dhigh, dlow = _randn(v.high_level.shape, 3), _randn(v.low_level.shape, 4)
    dphi = [_randn(p.shape, 10 + k) for k, p in enumerate(v.phase)]
    damp = [_randn(a.shape, 40 + k) for k, a in enumerate(v.amplitude)]
    torch.autograd.backward([v.high_level, *v.phase, *v.amplitude, v.low_level], [t.to(device) for t in [dhigh, *dphi, *damp, dlow]])
    # the GPU's own fp32 (phase, amplitude) go to the reference: the check is not conditioned by 1/A of values that differ
    G = [ana_ref.level_bands(ana_ref.polar_to_coeff_grad(dphi[k], damp[k], v.phase[k].detach().cpu(), v.amplitude[k].detach().cpu(), s), n)
         for k in range(spec.nlev)]
    _close(img.grad, ana_ref.analysis_adjoint64(spec, dhigh.squeeze(1), G, dlow.squeeze(1)), f"{h}x{w} image gradient")


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_band_filter(frame, device):
    """The plain R2C, column and C2R passes at the frame's own size: the finest level and the high residual, kept."""
    h, w, height, n, _ = frame
    spec = _spec(h, w, height)
    pyr = Pyramid(height, 4, S2, device)
    _assert_claims(_plan(pyr, frame), frame)
    img = _analysis(h, w, height, n)[0]
    high, bands, low = ana_ref.build64(spec, img)
    coeff = [high] + [[torch.view_as_real(z if k == 0 else torch.zeros_like(z)) for z in lv] for k, lv in enumerate(bands)] + [torch.zeros_like(low)]
    want = syn_ref.reconstruct64(spec, coeff)
    err = (pyr.band_filter(img.to(device), level_mask=1, keep_high=True).cpu() - want).abs().max().item()
    print(f"{h}x{w}: band filter err {err:.2e}")
    assert err <= 2e-5
