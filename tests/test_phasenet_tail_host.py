"""Host-side check of the tile geometry of vfi_phasenet_level_tail (csrc/vfi_phasenet_tail.h).  hipcc --cuda-host-only: no GPU
involved."""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_every_source_pixel_has_one_owning_tile_inside_its_window(tmp_path):
    """tile_span, compiled for the host with the address and undefined-behaviour sanitizers, over the 15 level pairs of a 1080p
    and of a 720p pyramid and 400 random up-scalings of at most x2, then over what the entry point accepts beyond those (20 pairs
    of exact scale 1, x2, x3, x8 and the GPU tests' shapes, 1500 random pairs of ratio 1..8 per axis): every source pixel owned
    by exactly one target tile, inside that tile's source window; windows within the kernel's LDS planes; every bilinear tap
    inside the window (tests/native/phasenet_tail_check.cpp)."""
    exe = str(tmp_path / "phasenet_tail_check")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "fusion-method-for-video-frame-interpolation_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "phasenet_tail_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "checked 1950 level pairs, 0 violations" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
