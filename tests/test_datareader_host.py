"""vfi_amd/train/datareader.py without a GPU: the parameter draw against a line-by-line restatement of reference
src/train/datareader.py:45-69, the reference face (`__getitem__`) against crop / flip / swap of `raw`, and TripletLoader with
`ops.triplet_batch_prepare` replaced by a recorder (device "cpu": no pinned memory, no events)."""
import ctypes
import random
import sys

import numpy as np
import pytest
import torch

import train_batch_ref as TR
from vfi_amd import _lib, ops
from vfi_amd.train import datareader as D


@pytest.fixture(scope="module")
def vimeo(tmp_path_factory):
    return TR.write_triplets(str(tmp_path_factory.mktemp("vimeo")), 7, 10, 14, seed=3)


def _seed(s):
    random.seed(s)
    torch.manual_seed(s)


def _states():
    return random.getstate(), torch.get_rng_state()


@pytest.mark.parametrize("crop,aug_s,aug_t", [((6, 9), True, True), ((6, 9), False, True), ((6, 9), True, False),
                                              ((10, 14), True, True), (None, True, True), ((6, 9), False, False),
                                              ((10, 9), True, True)])
def test_draw_consumes_the_generators_as_the_reference(vimeo, crop, aug_s, aug_t):
    ds = D.DBreader_Vimeo90k(vimeo, random_crop=crop, augment_s=aug_s, augment_t=aug_t)
    _seed(11)
    got = [ds.draw(10, 14) for _ in range(50)]
    got_states = _states()
    _seed(11)
    want = [TR.reference_draw(10, 14, crop, aug_s, aug_t) for _ in range(50)]
    want_states = _states()
    assert got == want
    assert got_states[0] == want_states[0] and torch.equal(got_states[1], want_states[1])
    if crop is not None and crop != (10, 14):
        assert len({g[:2] for g in got}) > 1
    flags = {g[2] for g in got}
    assert flags <= set(range(8)) and (len(flags) > 1) == (aug_s or aug_t)


def test_nothing_is_drawn_that_the_reference_does_not_draw(vimeo):
    # the crop is the frame: no torch draw; no augmentation: no coin
    ds = D.DBreader_Vimeo90k(vimeo, random_crop=(10, 14), augment_s=False, augment_t=False)
    _seed(5)
    before = _states()
    assert [ds.draw(10, 14) for _ in range(5)] == [(0, 0, 0)] * 5
    after = _states()
    assert before[0] == after[0] and torch.equal(before[1], after[1])
    # spatial augmentation off: one coin per draw, and only `random`'s
    ds = D.DBreader_Vimeo90k(vimeo, random_crop=(10, 14), augment_s=False, augment_t=True)
    _seed(5)
    draws = [ds.draw(10, 14) for _ in range(20)]
    assert torch.equal(torch.get_rng_state(), before[1])
    random.seed(5)
    assert draws == [(0, 0, D.SWAP if random.random() < 0.5 else 0) for _ in range(20)]
    with pytest.raises(ValueError):
        D.DBreader_Vimeo90k(vimeo, random_crop=(11, 14)).draw(10, 14)


def test_directory_walk_and_raw(vimeo):
    ds = D.DBreader_Vimeo90k(vimeo)
    assert len(ds) == 7 and list(ds.triplet_list) == sorted(ds.triplet_list)
    assert ds.triplet_list[0].endswith("/sequences/00001/0001") and ds.triplet_list[6].endswith("/sequences/00004/0001")
    frames = ds.raw(2)
    assert len(frames) == 3 and all(f.dtype == np.uint8 and f.shape == (10, 14, 3) for f in frames)
    from PIL import Image
    assert np.array_equal(frames[1], np.asarray(Image.open(ds.triplet_list[2] + "/im2.png")))
    small = D.DBreader_Vimeo90k(vimeo, resize=(5, 7)).raw(0)
    assert all(f.shape == (5, 7, 3) for f in small)


@pytest.mark.parametrize("crop", [(6, 9), None])
def test_getitem_is_crop_flip_swap_of_raw(vimeo, crop):
    ds = D.DBreader_Vimeo90k(vimeo, random_crop=crop)
    seen = set()
    for trial in range(24):
        index = trial % len(ds)
        _seed(100 + trial)
        triple = ds[index]
        _seed(100 + trial)
        i, j, flags = ds.draw(10, 14)
        seen.add(flags)
        h, w = crop or (10, 14)
        want = TR.prepare_ref(np.stack(ds.raw(index))[None], [[i, j, flags]], h, w)      # slots [first, last, middle]
        assert all(t.dtype == torch.float32 and tuple(t.shape) == (3, h, w) for t in triple)
        assert torch.equal(triple[0], TR.to_float(want[0, 0])) and torch.equal(triple[2], TR.to_float(want[1, 0]))
        assert torch.equal(triple[1], TR.to_float(want[2, 0]))
    assert len(seen) >= 6
    # and the class works under a stock DataLoader as the reference's does
    _seed(1)
    batches = list(torch.utils.data.DataLoader(dataset=ds, batch_size=3, shuffle=True, num_workers=0))
    assert [b[0].shape[0] for b in batches] == [3, 3, 1] and len(batches[0]) == 3


def _record(monkeypatch):
    calls = []

    def prepare(src, params, size, rgb=True, lab=True):
        assert src.dtype == torch.uint8 and params.dtype == torch.int32 and not params.is_cuda
        calls.append((src.clone(), params.clone(), tuple(size), rgb, lab))
        b, (h, w) = src.shape[0], size
        return torch.zeros((3, b, 3, h, w)), torch.zeros((3, 3 * b, h, w))
    monkeypatch.setattr(ops, "triplet_batch_prepare", prepare)
    return calls


def test_loader_does_not_depend_on_the_number_of_workers(vimeo, monkeypatch):
    calls = _record(monkeypatch)
    ds = D.DBreader_Vimeo90k(vimeo, random_crop=(6, 9))
    runs = []
    for workers in (1, 4):
        del calls[:]
        _seed(21)
        loader = D.TripletLoader(ds, 3, shuffle=True, workers=workers, device="cpu")
        assert len(loader) == 3
        batches = list(loader)
        assert len(batches) == 3 and len(calls) == 3
        runs.append([(c[0], c[1], b.paths) for c, b in zip(calls, batches)])
        assert [c[0].shape for c in calls] == [(3, 3, 10, 14, 3), (3, 3, 10, 14, 3), (1, 3, 10, 14, 3)]      # the last batch is short
        assert all(c[2] == (6, 9) for c in calls)
        b0 = batches[0]
        assert b0.img_batch_phase.shape == (27, 6, 9) and b0.lab_target.shape == (9, 6, 9) and b0.rgb_frame2.shape == (3, 3, 6, 9)
        assert torch.equal(b0.params, calls[0][1])
    for (s1, p1, paths1), (s4, p4, paths4) in zip(*runs):
        assert torch.equal(s1, s4) and torch.equal(p1, p4) and paths1 == paths4
    # the staging bytes are the frames of the batch's triplets, in order; the parameters are `draw`'s in sample order
    order = {str(p): k for k, p in enumerate(ds.triplet_list)}
    _seed(21)
    perm = torch.randperm(len(ds)).tolist()
    assert [order[p] for r in runs[0] for p in r[2]] == perm
    want = [ds.draw(10, 14) for _ in range(len(ds))]
    assert [tuple(int(v) for v in row) for r in runs[0] for row in r[1]] == want
    for src, _, paths in runs[0]:
        for n, p in enumerate(paths):
            assert np.array_equal(src[n].numpy(), np.stack(ds.raw(order[p])))
    assert D.TripletLoader(ds, 3, workers=99, device="cpu").workers == 16
    # without shuffling: the dataset's order
    got = [p for b in D.TripletLoader(ds, 4, shuffle=False, workers=2, device="cpu") for p in b.paths]
    assert got == [str(p) for p in ds.triplet_list]


def test_mixed_source_sizes_raise_naming_both(tmp_path, monkeypatch):
    _record(monkeypatch)
    root = TR.write_triplets(str(tmp_path), 3, 10, 14, sizes={1: (10, 16)})
    ds = D.DBreader_Vimeo90k(root, random_crop=(6, 9))
    with pytest.raises(ValueError) as e:
        list(D.TripletLoader(ds, 3, shuffle=False, workers=2, device="cpu"))
    assert "00001/0001" in str(e.value) and "00001/0002" in str(e.value)
    assert len(list(D.TripletLoader(ds, 1, shuffle=False, workers=2, device="cpu"))) == 3      # one size per batch is enough


def test_modules_import_without_torchvision_and_skimage(monkeypatch):
    import importlib.util
    for name in ("torchvision", "skimage", "matplotlib"):
        monkeypatch.setitem(sys.modules, name, None)             # `import torchvision` raises ImportError from here on
    for mod in ("vfi_amd.train.datareader", "vfi_amd.train.trainer", "vfi_amd.train.train", "vfi_amd.fusion_net.trainer",
                "vfi_amd.fusion_net.train"):
        origin = importlib.import_module(mod).__file__
        spec = importlib.util.spec_from_file_location(mod + "_again", origin)     # a second, fresh execution of the file
        spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_argument_checks_of_the_entry_point_need_no_gpu():
    """crop bounds and flags are refused on the host side of the ABI, before anything is enqueued"""
    h = _lib.lib()
    one = ctypes.c_void_p(256)
    blk = 3 * 5 * 7

    def call(params, rgb=one, lab=one, hh=5, ww=7, sb=blk):
        p = (ctypes.c_int * len(params))(*params)
        return h.vfi_triplet_batch_prepare(one, p, rgb, 2 * sb, sb, lab, 2 * sb, sb, len(params) // 3, 9, 13, hh, ww, None)
    assert call([0, 0, 0, 5, 6, 0]) == -1 and b"sample 1" in h.vfi_last_error() and b"rows" in h.vfi_last_error()
    assert call([0, 7, 0]) == -1 and b"columns" in h.vfi_last_error()
    assert call([0, 0, 8]) == -1 and b"flags" in h.vfi_last_error()
    assert call([0, 0, -1]) == -1 and call([-1, 0, 0]) == -1 and call([0, -1, 0]) == -1
    assert call([0, 0, 0], rgb=None, lab=None) == -1 and b"NULL" in h.vfi_last_error()
    assert call([0, 0, 0], hh=10) == -1 and call([0, 0, 0], ww=14) == -1
    assert call([0, 0, 0], sb=blk - 1) == -1 and b"strides" in h.vfi_last_error()
    assert h.vfi_triplet_batch_prepare(None, None, one, blk, blk, one, blk, blk, 1, 9, 13, 5, 7, None) == -1
