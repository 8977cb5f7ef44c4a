"""SCFpyr_PyTorch.plan: how many images it asks the library for (no GPU: the library call is replaced by a recorder).

A plan's max_images is the number of images one slice of a call holds, 16 at most; the library walks a
longer call in slices.  So a call of n images needs a plan of min(max(n, 6), 16), and a cached plan is replaced only when
that number grows."""
import contextlib

import torch

from vfi_amd import _lib
from vfi_amd.steerable import SCFpyr_PyTorch as S


def _recorder(monkeypatch):
    created = []

    def call(name, *args, work=None):
        if name == "vfi_pyr_plan_create":
            created.append(args[:6])
            assert 1 <= args[5] <= 16, "vfi_pyr_plan_create refuses max_images above 16"
        elif name == "vfi_pyr_plan_level_size":
            args[2]._obj.value, args[3]._obj.value = 8, 8
        else:
            raise AssertionError(f"unexpected library call {name}")
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(S.Plan, "__del__", lambda self: None)
    return created


def test_plan_asks_for_one_slice_and_rebuilds_only_on_growth(monkeypatch):
    created = _recorder(monkeypatch)
    scf = S.SCFpyr_PyTorch(height=5, nbands=4, scale_factor=2, device="cuda:0")
    asked = lambda: [c[5] for c in created]
    p1 = scf.plan(64, 96, 1)
    assert asked() == [6] and p1.max_images == 6 and created[0][:4] == (64, 96, 5, 4)
    assert scf.plan(64, 96, 6) is p1 and scf.plan(64, 96, 3) is p1 and asked() == [6]
    p9 = scf.plan(64, 96, 9)
    assert p9 is not p1 and asked() == [6, 9]
    assert scf.plan(64, 96, 7) is p9 and asked() == [6, 9]                   # never shrinks
    p16 = scf.plan(64, 96, 17)
    assert asked() == [6, 9, 16] and p16.max_images == 16
    for n in (16, 18, 72, 96, 120, 300, 1, 33):                                # a whole training batch: the same plan
        assert scf.plan(64, 96, n) is p16
    assert asked() == [6, 9, 16]
    # another frame size has its own plan; a first call of a whole batch asks for 16 at once
    assert scf.plan(32, 48, 72).max_images == 16 and asked() == [6, 9, 16, 16]
    assert scf.plan(32, 48, 2).max_images == 16 and asked() == [6, 9, 16, 16]
    assert scf.plan(64, 96, 4) is p16
