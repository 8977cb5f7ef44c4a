"""The two scene-cut entry points on the GPU (vfi_luma_sad, vfi_frame_pick), through ops.luma_sad
and ops.frame_pick: the sum against numpy int64, exactly, at sizes around the 16-byte segment, the wave and the workgroup
and with both buffers at byte offsets that take the segment path and the byte path; the decision on both sides of the
threshold and where unsigned wrap would get it wrong; the replacement byte for byte; guard bytes around every buffer."""
import numpy as np
import pytest
import torch

from vfi_amd import ops

pytestmark = pytest.mark.gpu

PAD = 32                                   # guard bytes on each side of a buffer
GARBAGE = -0x0123456789ABCDEF              # what the output word holds before a call
OFFSETS = [(0, 0), (1, 1), (1, 2), (3, 0)]
FILLS = ["random", "equal", "0-255"]


def planes(n, fill, seed):
    rng = np.random.default_rng(seed)
    if fill == "random":
        return rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    if fill == "equal":
        a = rng.integers(0, 256, n, dtype=np.uint8)
        return a, a.copy()
    return np.zeros(n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)


def guarded(data, off, device, guard=0xA5):
    """-> (storage, view): `data` at byte PAD + off of a storage filled with `guard` (the allocator aligns the storage
    to far more than 16 bytes, so `off` is the view's misalignment)"""
    store = torch.full((PAD + off + len(data) + PAD,), guard, dtype=torch.uint8, device=device)
    view = store[PAD + off:PAD + off + len(data)]
    view.copy_(torch.from_numpy(data))
    assert view.data_ptr() % 16 == off % 16
    return store, view


def guards_intact(store, off, n, guard=0xA5):
    s = store.cpu().numpy()
    return bool((s[:PAD + off] == guard).all() and (s[PAD + off + n:] == guard).all())


def sad_word(device):
    word = torch.tensor([7, GARBAGE, -7], dtype=torch.int64, device=device)
    return word, word[1:2]


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: f"off{o[0]}_{o[1]}")
@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 63, 64, 65, 255, 4097, 64 * 96])
def test_luma_sad_equals_numpy_int64(n, offs, device):
    for fill in FILLS:
        a, b = planes(n, fill, n * 7 + offs[0] * 3 + offs[1])
        want = int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())
        (sa, va), (sb, vb) = guarded(a, offs[0], device), guarded(b, offs[1], device)
        word, out = sad_word(device)
        got = ops.luma_sad(va, vb, n, out=out)
        assert got is out
        first = word.cpu().tolist()
        assert first == [7, want, -7], (fill, first, want)            # exact, whatever the word held; its neighbours untouched
        out.fill_(GARBAGE + 1)
        ops.luma_sad(va, vb, n, out=out)
        assert word.cpu().tolist() == first                           # the same bits again
        assert guards_intact(sa, offs[0], n) and guards_intact(sb, offs[1], n)
        assert np.array_equal(va.cpu().numpy(), a) and np.array_equal(vb.cpu().numpy(), b)
    # a new output tensor, and a count smaller than the buffers: only the first n bytes count
    if n > 1:
        got = ops.luma_sad(va, vb, n - 1)
        assert got.dtype == torch.int64 and tuple(got.shape) == (1,)
        assert int(got.item()) == int(np.abs(a[:n - 1].astype(np.int64) - b[:n - 1].astype(np.int64)).sum())


def test_luma_sad_past_32_bits_and_past_the_block_cap(device):
    """17 MiB of 0 against 255 sum to 4.5e9 > 2^32, the smallest size where a 32-bit total goes wrong; at this size the
    grid is capped and every thread strides.  Once on the segment path, once with random bytes on the byte path."""
    n = 17 << 20
    a, b = planes(n, "0-255", 0)
    (sa, va), (sb, vb) = guarded(a, 0, device), guarded(b, 0, device)
    word, out = sad_word(device)
    ops.luma_sad(va, vb, n, out=out)
    assert word.cpu().tolist() == [7, 255 * n, -7] and 255 * n > 1 << 32
    assert guards_intact(sa, 0, n) and guards_intact(sb, 0, n)
    a, b = planes(n, "random", 1)
    want = int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())
    for offs in ((1, 2), (5, 5)):
        (sa, va), (sb, vb) = guarded(a, offs[0], device), guarded(b, offs[1], device)
        ops.luma_sad(va, vb, n, out=out)
        assert word.cpu().tolist() == [7, want, -7], offs
        assert guards_intact(sa, offs[0], n) and guards_intact(sb, offs[1], n)


# (sad, sad_prev, min_sad, cut): s = min(sad, |sad - prev|) against min_sad
DECISIONS = [
    (1000, None, 1000, True),                   # first pair, s == min_sad exactly
    (1000, None, 1001, False),                  # s == min_sad - 1
    (5000, 5600, 600, True),                    # prev above sad: sad - prev wraps to 2^64 - 600, and min() would pick 5000
    (5000, 5600, 601, False),
    (5000, 4400, 600, True),                    # prev below sad: prev - sad wraps
    (5000, 4400, 601, False),
    (500, 9000, 500, True),                     # sad itself is the smaller
    (500, 9000, 501, False),
    (5 * 10 ** 9, 5 * 10 ** 9 + 600, 600, True),    # words past 32 bits
    (5 * 10 ** 9 + 600, 5 * 10 ** 9, 601, False),
    (0, 0, 0, True),                            # min_sad = 0 always replaces
    (0, None, 0, True),
    (0, None, 1, False),
]


@pytest.mark.parametrize("offs", [(0, 0), (1, 3), (2, 0)], ids=lambda o: f"off{o[0]}_{o[1]}")
@pytest.mark.parametrize("nbytes", [1, 3, 17, 4099, 64 * 96 * 3 // 2])
def test_frame_pick_decides_and_replaces(nbytes, offs, device):
    rng = np.random.default_rng(nbytes + offs[0])
    src = rng.integers(0, 256, nbytes, dtype=np.uint8)
    before = (src + rng.integers(1, 256, nbytes, dtype=np.uint8)).astype(np.uint8)     # differs from src in every byte
    ss, vs = guarded(src, offs[1], device, guard=0x5A)
    word = lambda v: None if v is None else torch.tensor([v], dtype=torch.int64, device=device)
    for i, (sad, prev, min_sad, cut) in enumerate(DECISIONS):
        sd, vd = guarded(before, offs[0], device)
        flag = torch.tensor([-5, 77, -5], dtype=torch.int32, device=device)
        got = ops.frame_pick(vd, vs, word(sad), word(prev), min_sad, cut=flag[1:2])
        assert got.data_ptr() == flag[1:2].data_ptr()
        assert flag.cpu().tolist() == [-5, int(cut), -5], (sad, prev, min_sad)
        assert np.array_equal(vd.cpu().numpy(), src if cut else before), (sad, prev, min_sad)
        assert guards_intact(sd, offs[0], nbytes) and guards_intact(ss, offs[1], nbytes, guard=0x5A)
        if i < 2:                                                     # without the flag: the same bytes
            sd2, vd2 = guarded(before, offs[0], device)
            assert ops.frame_pick(vd2, vs, word(sad), word(prev), min_sad) is None
            assert torch.equal(sd2, sd)
    assert np.array_equal(vs.cpu().numpy(), src)


def test_frame_pick_reads_the_word_luma_sad_wrote(device):
    """the two calls chained on one stream, as the clip loop chains them: no host value in between"""
    n = 64 * 96
    a, b = planes(n, "random", 3)
    want = int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())
    ta, tb = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
    for min_sad, cut in ((want, True), (want + 1, False)):
        dst = torch.zeros(n, dtype=torch.uint8, device=device)
        flag = torch.full((1,), 9, dtype=torch.int32, device=device)
        ops.frame_pick(dst, ta, ops.luma_sad(ta, tb, n), None, min_sad, cut=flag)
        assert int(flag.item()) == int(cut)
        assert torch.equal(dst, ta) if cut else not dst.any()


def test_wrong_arguments_raise_and_write_nothing(device):
    a = torch.zeros(64, dtype=torch.uint8, device=device)
    w = torch.zeros(1, dtype=torch.int64, device=device)
    E = ops.VfiLibraryError
    with pytest.raises(E):
        ops.luma_sad(a, a.cpu(), 64)
    with pytest.raises(E):
        ops.luma_sad(a.float(), a, 64)
    with pytest.raises(E):
        ops.luma_sad(a, a, 65)                                        # more than the buffers hold
    with pytest.raises(E):
        ops.luma_sad(a, a, 64, out=torch.zeros(1, dtype=torch.int32, device=device))
    with pytest.raises(E):
        ops.luma_sad(a, a, 64, out=torch.zeros(2, dtype=torch.int64, device=device))
    dst = torch.full((64,), 3, dtype=torch.uint8, device=device)
    with pytest.raises(E):
        ops.frame_pick(dst, a[:63], w, None, 0)
    with pytest.raises(E):
        ops.frame_pick(dst, a, None, None, 0)
    with pytest.raises(E):
        ops.frame_pick(dst, a, w.int(), None, 0)
    with pytest.raises(E):
        ops.frame_pick(dst, a, w, w.cpu(), 0)
    with pytest.raises(E):
        ops.frame_pick(dst, a, w, None, 0, cut=torch.zeros(1, dtype=torch.int64, device=device))
    with pytest.raises(E):
        ops.frame_pick(dst, a, w, None, 1 << 64)
    assert bool((dst == 3).all())
