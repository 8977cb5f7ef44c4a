// Per-thread bodies of the two scene-cut kernels (vfi_scene.hip): everything that computes an address.  They are plain
// functions of (pointers, size, thread index, thread count), so the same text also compiles as host C++ with
// VFI_SCENE_HOST defined, where a stand-alone program walks them thread by thread over exact-size heap buffers under
// AddressSanitizer (tools/scene_host_check.cpp).  The wave / workgroup reduction, the atomic and the launches stay in
// vfi_scene.hip.
#pragma once
#include <cstdint>

#ifdef VFI_SCENE_HOST
#define VFI_SCENE_FN inline
#else
#define VFI_SCENE_FN __device__ __forceinline__
#endif

namespace vfi_scene {

struct alignas(16) Seg16 { unsigned x, y, z, w; };      // one 16-byte segment: a dwordx4 load or store
struct alignas(4) Seg4 { unsigned x; };

// acc + sum over the four bytes of |a_i - b_i|: one v_sad_u8 on the device
VFI_SCENE_FN unsigned sad4(unsigned a, unsigned b, unsigned acc) {
#ifdef VFI_SCENE_HOST
    for (int k = 0; k < 4; ++k) {
        const int x = (int)((a >> (8 * k)) & 255u), y = (int)((b >> (8 * k)) & 255u);
        acc += (unsigned)(x > y ? x - y : y - x);
    }
    return acc;
#else
    return __builtin_amdgcn_sad_u8(a, b, acc);
#endif
}

VFI_SCENE_FN unsigned sad1(unsigned char a, unsigned char b) { return a > b ? (unsigned)(a - b) : (unsigned)(b - a); }

// Thread g of T: its share of sum |a[i] - b[i]|, i < n.  Where a and b sit equally far off a 16-byte boundary the threads
// stride over the 16-byte segments between the head (the bytes before a's first boundary) and the tail (what is left
// after the last whole segment), and threads 0 ... 14 take one head and one tail byte each (T >= 15); otherwise they
// stride over bytes.  A thread adds fewer than n / T + 18 bytes of 255 each: see the bound at the launch.
VFI_SCENE_FN unsigned sad_partial(const unsigned char *a, const unsigned char *b, long long n, long long g, long long T) {
    unsigned acc = 0;
    if ((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 15) {
        for (long long i = g; i < n; i += T) acc += sad1(a[i], b[i]);
        return acc;
    }
    const long long off = (long long)((16 - (reinterpret_cast<uintptr_t>(a) & 15)) & 15);
    const long long head = off < n ? off : n;
    const long long nseg = (n - head) / 16, tail_at = head + 16 * nseg;
    const Seg16 *va = reinterpret_cast<const Seg16 *>(a + head), *vb = reinterpret_cast<const Seg16 *>(b + head);
    for (long long s = g; s < nseg; s += T) {
        const Seg16 x = va[s], y = vb[s];
        acc = sad4(x.x, y.x, acc);
        acc = sad4(x.y, y.y, acc);
        acc = sad4(x.z, y.z, acc);
        acc = sad4(x.w, y.w, acc);
    }
    if (g < head) acc += sad1(a[g], b[g]);
    if (g < n - tail_at) acc += sad1(a[tail_at + g], b[tail_at + g]);
    return acc;
}

// min(sad, |sad - prev|) >= min_sad, the difference without unsigned wrap in either direction
VFI_SCENE_FN bool is_cut(unsigned long long sad, unsigned long long prev, unsigned long long min_sad) {
    const unsigned long long d = sad > prev ? sad - prev : prev - sad;
    return (sad < d ? sad : d) >= min_sad;
}

// Thread g of T: its share of dst[0, n) = src[0, n).  dst decides the segments: the head runs to its first 16-byte
// boundary, then whole 16-byte stores, then the tail; each byte has one writer.  src is read as one 16-byte load where it
// is as far off as dst, as four dwords where it is a multiple of 4 off, and byte by byte otherwise.  Threads 0 ... 14
// take one head and one tail byte each (T >= 15).
VFI_SCENE_FN void copy_partial(unsigned char *dst, const unsigned char *src, long long n, long long g, long long T) {
    const long long off = (long long)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
    const long long head = off < n ? off : n;
    const long long nseg = (n - head) / 16, tail_at = head + 16 * nseg;
    Seg16 *vd = reinterpret_cast<Seg16 *>(dst + head);
    const unsigned char *sb = src + head;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(sb) & 15);
    for (long long s = g; s < nseg; s += T) {
        Seg16 v;
        if (mis == 0) {
            v = reinterpret_cast<const Seg16 *>(sb)[s];
        } else if ((mis & 3) == 0) {
            const Seg4 *p = reinterpret_cast<const Seg4 *>(sb + 16 * s);
            v.x = p[0].x; v.y = p[1].x; v.z = p[2].x; v.w = p[3].x;
        } else {
            const unsigned char *p = sb + 16 * s;
            unsigned q[4];
            for (int k = 0; k < 4; ++k)
                q[k] = (unsigned)p[4 * k] | (unsigned)p[4 * k + 1] << 8 | (unsigned)p[4 * k + 2] << 16 | (unsigned)p[4 * k + 3] << 24;
            v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
        }
        vd[s] = v;
    }
    if (g < head) dst[g] = src[g];
    if (g < n - tail_at) dst[tail_at + g] = src[tail_at + g];
}

}  // namespace vfi_scene
