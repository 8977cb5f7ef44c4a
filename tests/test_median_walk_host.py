"""Host model of median_walk_kernel (csrc/vfi_image.hip): the stable 1-bit LSD radix rank with skipped constant bits,
the per-wave ballot scatter, the rank table, and the snake walk of one bitset per wave with a (word, popcount-below)
cursor -- step for step as the kernel does them, with the tile, the wave width and the wave count as parameters so that
small images exercise every edge.  Checked against scipy.ndimage.median_filter, which the reference calls."""
import numpy as np
import pytest
from scipy.ndimage import median_filter


def key_of(x):
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)


def float_of(k):
    k = np.uint64(k)
    b = (k & np.uint64(0x7FFFFFFF)) if k & np.uint64(0x80000000) else (~k & np.uint64(0xFFFFFFFF))
    return np.array([b], np.uint64).astype(np.uint32).view(np.float32)[0]


def sym_reflect(i, n):
    if n == 1:
        return 0
    i %= 2 * n
    return i if i < n else 2 * n - 1 - i


def radix_ranks(K, U, lanes, waves):
    """Positions in rank order, exactly as the kernel's passes scatter them (sequence index = wave span, slot, lane)."""
    N = len(K)
    E = N // (lanes * waves)
    vary = 0
    for k in K[:U]:
        vary |= int(k) ^ int(K[0])
    src = np.arange(N)
    for b in range(32):
        if not (vary >> b) & 1:
            continue
        dst = np.full(N, -1)
        bits = ((K[src] >> np.uint64(b)) & np.uint64(1)).astype(int)
        zsum = [int((bits[w * lanes * E:(w + 1) * lanes * E] == 0).sum()) for w in range(waves)]
        ztot = sum(zsum)
        for w in range(waves):
            zi = sum(zsum[:w])
            oi = ztot + w * lanes * E - zi
            for j in range(E):
                idx = w * lanes * E + j * lanes + np.arange(lanes)
                one = bits[idx] == 1
                zb = np.cumsum(~one) - (~one)               # zero lanes below each lane (mbcnt of the ballot)
                d = np.where(one, oi + np.arange(lanes) - zb, zi + zb)
                dst[d] = src[idx]
                nz = int((~one).sum())
                zi += nz
                oi += lanes - nz
        assert (dst >= 0).all() and len(set(dst.tolist())) == N
        src = dst
    return src


def walk_model(img, S, T=8, lanes=16, waves=4):
    H, W = img.shape
    assert S <= lanes and T % waves == 0
    rows = T // waves
    out = np.full((H, W), np.nan, np.float32)
    PW = T + S - 1
    U = PW * PW
    E = -(-U // (lanes * waves))
    N = E * lanes * waves
    lo = S // 2
    need = S * S // 2 + 1
    for y0 in range(0, H, T):
        for x0 in range(0, W, T):
            K = np.full(N, 0xFFFFFFFF, np.uint64)
            for pos in range(U):
                r, c = divmod(pos, PW)
                K[pos] = key_of(img[sym_reflect(y0 - lo + r, H), sym_reflect(x0 - lo + c, W)])
            P = radix_ranks(K, U, lanes, waves)
            R = np.empty(N, int)
            R[P] = np.arange(N)
            Ks = K[P]
            assert (R[:U] < U).all()                       # the padding ranks last
            nwords = N // 32
            cv = min(T, W - x0)
            for wave in range(waves):
                r0 = wave * rows
                rv = min(rows, H - y0 - r0)
                if rv <= 0:
                    continue
                bits = np.zeros(nwords, np.uint64)

                def flip(rk, on):
                    if on:
                        bits[rk >> 5] |= np.uint64(1 << (rk & 31))
                    else:
                        bits[rk >> 5] &= ~np.uint64(1 << (rk & 31)) & np.uint64(0xFFFFFFFF)
                for i in range(S * S):
                    r, c = divmod(i, S)
                    flip(R[(r0 + r) * PW + c], True)
                pc = lambda w: bin(int(w)).count("1")
                cum = np.cumsum([pc(w) for w in bits])
                ptr = int(np.argmax(cum >= need))
                below = int(cum[ptr] - pc(bits[ptr]))
                for j in range(rv):
                    r = r0 + j
                    right = j % 2 == 0
                    for s in range(cv):
                        col = s if right else cv - 1 - s
                        if s > 0 or j > 0:
                            L = np.arange(S)
                            if s == 0:
                                po, pi = (r - 1) * PW + col + L, (r + S - 1) * PW + col + L
                            elif right:
                                po, pi = (r + L) * PW + col - 1, (r + L) * PW + col + S - 1
                            else:
                                po, pi = (r + L) * PW + col + S, (r + L) * PW + col
                            for rk in R[po]:
                                flip(rk, False)
                            for rk in R[pi]:
                                flip(rk, True)
                            below += int(((R[pi] >> 5) < ptr).sum()) - int(((R[po] >> 5) < ptr).sum())
                        while below >= need:
                            ptr -= 1
                            below -= pc(bits[ptr])
                        while below + pc(bits[ptr]) < need:
                            below += pc(bits[ptr])
                            ptr += 1
                        wv, k, bit = int(bits[ptr]), need - below, 0
                        for wd in (16, 8, 4, 2, 1):
                            c = bin(wv & ((1 << wd) - 1)).count("1")
                            if k > c:
                                k -= c
                                wv >>= wd
                                bit += wd
                        assert wv & 1 and k == 1
                        out[y0 + r, x0 + col] = float_of(Ks[ptr * 32 + bit])
    return out


@pytest.mark.parametrize("h,w,S,seed", [(19, 21, 5, 0), (12, 17, 4, 1), (9, 10, 7, 2), (5, 3, 6, 3), (16, 16, 2, 4), (13, 11, 3, 5)])
def test_walk_model_matches_scipy(h, w, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (h, w)).astype(np.float32) * 0.5      # heavy ties
    x[rng.random((h, w)) < 0.2] = -0.0
    x[rng.random((h, w)) < 0.2] = 0.0
    x[0, : w // 2] = rng.standard_normal(w // 2).astype(np.float32)
    got = walk_model(x, S)
    ref = median_filter(x, size=S)
    assert np.array_equal(got, ref)          # a selection: exact (scipy itself does not order -0.0 and +0.0)


def test_walk_model_constant_image_and_signed_zeros():
    x = np.zeros((10, 9), np.float32)
    assert np.array_equal(walk_model(x, 4), median_filter(x, size=4))
    x[::2] = -0.0                                                   # -0.0 sorts below +0.0
    assert np.array_equal(walk_model(x, 3), median_filter(x, size=3))


def test_radix_ranks_are_a_stable_sort():
    rng = np.random.default_rng(7)
    K = key_of(rng.integers(-4, 4, 200).astype(np.float32))
    K = np.concatenate([K, np.full(56, 0xFFFFFFFF, np.uint64)])
    P = radix_ranks(K, 200, 16, 4)
    assert np.array_equal(P, np.argsort(K, kind="stable"))
