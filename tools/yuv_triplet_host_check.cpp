// Host walk of the training-side crop decoder (csrc/vfi_yuv_triplet_body.h over csrc/vfi_yuv_pixel.h), thread by thread over
// exact-size heap buffers, meant to be built with -fsanitize=address,undefined: a source byte read outside the three frames
// or a float stored outside the outputs stops the program.  Per case it also
//   * counts the writers of every output float from the header's index functions (block_of, row_inside, cols_inside,
//     out_row, out_col, store_is_vector): exactly one inside the crop's output, none elsewhere;
//   * compares every output float, bit for bit, with the crop / hflip / vflip / slot choice of a whole-frame decode made with
//     the same decode_block and lab_of, and checks that the padding between slots still holds its sentinel.
// Cases: the source shapes of tests/test_yuv_triplet_batch_gpu.py -- every crop size at every origin for the small ones, the
// test's crop sizes at every origin for the others -- times all eight flag values, frame strides of the frame's bytes and one
// more (the source then one byte off its alignment), and outputs 0 ... 3 floats off 16 bytes (the slot stride padded by as
// many floats).  No device is involved.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DVFI_YUV_HOST \
//       -I fusion-method-for-video-frame-interpolation_amd/csrc tools/yuv_triplet_host_check.cpp -o yuv_triplet_host_check && ./yuv_triplet_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vfi_yuv_triplet_body.h"

#if defined(__SANITIZE_ADDRESS__)
#define VFI_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define VFI_ASAN 1
#endif
#endif
#ifdef VFI_ASAN
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

namespace {

using namespace vfi_yuv;

unsigned rnd_state = 12345u;
unsigned char rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return (unsigned char)(rnd_state >> 24); }

// malloc(n + off) ends exactly at the last byte; the `off` bytes in front (malloc aligns to 16, so `off` is the buffer's
// misalignment) are poisoned by hand, which the sanitizer honours in whole 8-byte granules
struct Exact {
    unsigned char *raw, *p;
    size_t off;
    Exact(size_t n, size_t off_) : raw(static_cast<unsigned char *>(malloc(n + off_))), p(raw + off_), off(off_) { POISON(raw, off); }
    ~Exact() { UNPOISON(raw, off); free(raw); }
    Exact(const Exact &) = delete;
};

const unsigned kSentinel = 0x7FC0BEEFu;
unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

struct Format { int sub, siting, matrix, range; };

template <bool S420, bool LEFT>
void thread_of(const unsigned char *src, int Hs, int Ws, const YuvCoef &k, int ci, int cj, int flags, int frame, int g, float *rgb,
               long long rs, float *lab, long long ls, int h, int w) {
    triplet_thread<S420, LEFT>(src, Hs, Ws, k, ci, cj, flags, frame, g, rgb, rs, lab, ls, h, w);
}

// whole-frame decode with the pieces the kernels share: rgb and lab (3, Hs, Ws)
template <bool S420, bool LEFT>
void whole_frame(const unsigned char *frame, int Hs, int Ws, const YuvCoef &k, std::vector<float> &rgb, std::vector<float> &lab) {
    constexpr int R = S420 ? 2 : 1;
    const size_t hw = (size_t)Hs * Ws;
    rgb.assign(3 * hw, 0.0f);
    lab.assign(3 * hw, 0.0f);
    for (int ry = 0; ry < Hs / R; ++ry)
        for (int x0 = 0; x0 < Ws; x0 += kDecPix) {
            float px[R][kDecPix][3];
            decode_block<S420, LEFT>(frame, Hs, Ws, k, ry, x0, px);
            for (int r = 0; r < R; ++r)
                for (int c = 0; c < kDecPix && x0 + c < Ws; ++c) {
                    float q[3];
                    lab_of(px[r][c], q);
                    for (int p = 0; p < 3; ++p) {
                        rgb[p * hw + (size_t)(ry * R + r) * Ws + x0 + c] = px[r][c][p];
                        lab[p * hw + (size_t)(ry * R + r) * Ws + x0 + c] = q[p];
                    }
                }
        }
}

long long cases = 0, failures = 0;

void fail(const char *what, const Format &f, int Hs, int Ws, int h, int w, int i, int j, int flags, int extra, int off) {
    if (++failures <= 20)
        printf("%s: format (%d,%d,%d,%d) source %dx%d crop %dx%d at (%d,%d) flags %d stride +%d offset %d\n", what, f.sub, f.siting,
               f.matrix, f.range, Hs, Ws, h, w, i, j, flags, extra, off);
}

// one source (three frames at a stride), every listed crop of it
struct Source {
    Format f;
    int Hs, Ws, extra;
    size_t frame_bytes, stride;
    Exact buf;
    std::vector<float> rgb[3], lab[3];
    YuvCoef k;
    Source(const Format &f_, int Hs_, int Ws_, int extra_)
        : f(f_), Hs(Hs_), Ws(Ws_), extra(extra_),
          frame_bytes((size_t)Hs_ * Ws_ + 2 * (f_.sub == VFI_YUV_420 ? (size_t)(Hs_ / 2) * (Ws_ / 2) : (size_t)Hs_ * Ws_)),
          stride(frame_bytes + extra_), buf(2 * stride + frame_bytes, (size_t)extra_), k(make_coef(f_.matrix, f_.range)) {
        for (size_t n = 0; n < 2 * stride + frame_bytes; ++n) buf.p[n] = rnd();
        for (int fr = 0; fr < 3; ++fr) {
            const unsigned char *p = buf.p + fr * stride;
            if (f.sub != VFI_YUV_420) whole_frame<false, false>(p, Hs, Ws, k, rgb[fr], lab[fr]);
            else if (f.siting == VFI_YUV_SITING_LEFT) whole_frame<true, true>(p, Hs, Ws, k, rgb[fr], lab[fr]);
            else whole_frame<true, false>(p, Hs, Ws, k, rgb[fr], lab[fr]);
        }
    }

    void crop(int h, int w, int i, int j, int flags, int off) {
        ++cases;
        const int R = f.sub == VFI_YUV_420 ? 2 : 1;
        const size_t hw = (size_t)h * w, slot = 3 * hw + off, total = 2 * slot + 3 * hw;
        const bool hflip = flags & 1, vflip = flags & 2, swap = flags & 4;
        // writers, from the index functions alone
        const BlockSpan span = block_span(i, j, h, w, R);
        const int threads = (block_count(span) + 255) / 256 * 256;
        std::vector<int> writers(hw, 0);
        bool ok = true;
        for (int g = 0; g < threads; ++g) {
            int ry, x0;
            if (!block_of(span, g, &ry, &x0)) continue;
            ok = ok && ry >= 0 && ry * R + R <= Hs && x0 >= 0 && x0 < Ws && x0 % kDecPix == 0;      // a block of the frame's grid
            int c_lo, c_hi;
            cols_inside(x0, j, w, &c_lo, &c_hi);
            for (int r = 0; r < R; ++r) {
                if (!row_inside(ry * R + r, i, h)) continue;
                const int oy = out_row(ry * R + r, i, h, vflip);
                for (int c = c_lo; c < c_hi; ++c) {
                    const int ox = out_col(x0 + c, j, w, hflip);
                    if (oy < 0 || oy >= h || ox < 0 || ox >= w) { ok = false; continue; }
                    ++writers[(size_t)oy * w + ox];
                }
            }
        }
        for (size_t n = 0; n < hw; ++n) ok = ok && writers[n] == 1;
        if (!ok) fail("writers", f, Hs, Ws, h, w, i, j, flags, extra, off);
        // the body itself, over exact-size outputs
        Exact R_(total * 4, (size_t)off * 4), L_(total * 4, (size_t)off * 4);
        float *rgb_o = reinterpret_cast<float *>(R_.p), *lab_o = reinterpret_cast<float *>(L_.p);
        for (size_t n = 0; n < total; ++n) { memcpy(rgb_o + n, &kSentinel, 4); memcpy(lab_o + n, &kSentinel, 4); }
        for (int fr = 0; fr < 3; ++fr)
            for (int g = 0; g < threads; ++g) {
                const unsigned char *p = buf.p + fr * stride;
                if (f.sub != VFI_YUV_420) thread_of<false, false>(p, Hs, Ws, k, i, j, flags, fr, g, rgb_o, (long long)slot, lab_o, (long long)slot, h, w);
                else if (f.siting == VFI_YUV_SITING_LEFT) thread_of<true, true>(p, Hs, Ws, k, i, j, flags, fr, g, rgb_o, (long long)slot, lab_o, (long long)slot, h, w);
                else thread_of<true, false>(p, Hs, Ws, k, i, j, flags, fr, g, rgb_o, (long long)slot, lab_o, (long long)slot, h, w);
            }
        bool same = true;
        const size_t shw = (size_t)Hs * Ws;
        for (int fr = 0; fr < 3; ++fr) {
            const int s = fr == 1 ? 2 : ((fr == 2) != swap ? 1 : 0);
            for (int p = 0; p < 3; ++p)
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const int sy = i + (vflip ? h - 1 - y : y), sx = j + (hflip ? w - 1 - x : x);
                        const size_t at = s * slot + p * hw + (size_t)y * w + x, from = p * shw + (size_t)sy * Ws + sx;
                        same = same && bits(rgb_o[at]) == bits(rgb[fr][from]) && bits(lab_o[at]) == bits(lab[fr][from]);
                    }
        }
        for (int s = 0; s < 2; ++s)
            for (int n = 0; n < off; ++n)
                same = same && bits(rgb_o[s * slot + 3 * hw + n]) == kSentinel && bits(lab_o[s * slot + 3 * hw + n]) == kSentinel;
        if (!same) fail("values", f, Hs, Ws, h, w, i, j, flags, extra, off);
    }

    void origins(int h, int w) {
        for (int i = 0; i + h <= Hs; ++i)
            for (int j = 0; j + w <= Ws; ++j)
                for (int flags = 0; flags < 8; ++flags)
                    for (int off = 0; off < 4; ++off) crop(h, w, i, j, flags, off);
    }
    void every_crop() {
        for (int h = 1; h <= Hs; ++h)
            for (int w = 1; w <= Ws; ++w) origins(h, w);
    }
};

}  // namespace

int main() {
    const Format f420[] = {{VFI_YUV_420, VFI_YUV_SITING_CENTRE, VFI_YUV_BT709, VFI_YUV_LIMITED}, {VFI_YUV_420, VFI_YUV_SITING_LEFT, VFI_YUV_BT601, VFI_YUV_FULL}};
    const Format f444[] = {{VFI_YUV_444, VFI_YUV_SITING_CENTRE, VFI_YUV_BT709, VFI_YUV_FULL}, {VFI_YUV_444, VFI_YUV_SITING_CENTRE, VFI_YUV_BT601, VFI_YUV_LIMITED}};
    for (int extra = 0; extra < 2; ++extra) {
        for (const Format &f : f420) {
            Source(f, 2, 2, extra).every_crop();
            Source(f, 6, 10, extra).every_crop();
            Source(f, 18, 66, extra).origins(5, 7);
            { Source s(f, 8, 130, extra); s.origins(8, 128); s.origins(6, 127); }
        }
        for (const Format &f : f444) {
            Source(f, 3, 5, extra).every_crop();
            { Source s(f, 7, 67, extra); s.origins(4, 61); s.origins(1, 4); s.origins(7, 67); }
        }
    }
    printf("yuv_triplet_host_check: %lld cases, %lld failures\n", cases, failures);
    return failures ? 1 : 0;
}
