// Per-pixel pieces of the Y'CbCr decode, shared by the whole-frame decoder (vfi_yuv.hip) and the training-side crop
// decoder (vfi_yuv_triplet.hip): the coefficients, the byte loads, the 4:2:0 chroma up-sampling, the colour matrix with its
// clamp, and the Lab of the clamped rgb.  Both kernels give a thread the same block of the frame's own grid -- four luma
// columns of one chroma row -- and call decode_block on it, so a pixel sees the same arithmetic whichever kernel decodes it.
// The text also compiles as host C++ with VFI_YUV_HOST defined, where a stand-alone program walks the crop decoder thread by
// thread under AddressSanitizer (tools/yuv_triplet_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/vfi_hip.h"

#ifdef VFI_YUV_HOST
#define VFI_YUV_FN inline
#else
#define VFI_YUV_FN __host__ __device__ __forceinline__      // (host too: the launch sizes its grid with the index functions)
#endif

namespace vfi_yuv {

struct YuvCoef {
    float kr, kb, kg;                  // luma weights, kg = 1 - kr - kb
    float r_cr, b_cb;                  // 2 (1 - kr), 2 (1 - kb)
    float y_off, y_scale, c_scale;     // 16, 219, 224 (limited) | 0, 255, 255 (full)
    float y_lo, y_hi, c_lo, c_hi;      // the range's limits
};

inline YuvCoef make_coef(int matrix, int range) {
    YuvCoef k;
    k.kr = matrix == VFI_YUV_BT709 ? 0.2126f : 0.299f;
    k.kb = matrix == VFI_YUV_BT709 ? 0.0722f : 0.114f;
    k.kg = 1.0f - k.kr - k.kb;
    k.r_cr = 2.0f * (1.0f - k.kr);
    k.b_cb = 2.0f * (1.0f - k.kb);
    const bool lim = range == VFI_YUV_LIMITED;
    k.y_off = lim ? 16.0f : 0.0f;
    k.y_scale = lim ? 219.0f : 255.0f;
    k.c_scale = lim ? 224.0f : 255.0f;
    k.y_lo = k.c_lo = lim ? 16.0f : 0.0f;
    k.y_hi = lim ? 235.0f : 255.0f;
    k.c_hi = lim ? 240.0f : 255.0f;
    return k;
}

VFI_YUV_FN int imin(int a, int b) { return a < b ? a : b; }
VFI_YUV_FN int imax(int a, int b) { return a > b ? a : b; }

// the formulas of rgb2lab_kernel (vfi_image.hip), which stays as it is; the compiler may contract them differently here
VFI_YUV_FN void lab_of(const float rgb[3], float lab[3]) {
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = rgb[k];
        c[k] = v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
    }
    float x = 0.412453f * c[0] + 0.357580f * c[1] + 0.180423f * c[2];
    float y = 0.212671f * c[0] + 0.715160f * c[1] + 0.072169f * c[2];
    float z = 0.019334f * c[0] + 0.119193f * c[1] + 0.950227f * c[2];
    x /= 0.95047f; z /= 1.08883f;
    auto f = [](float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; };
    const float fx = f(x), fy = f(y), fz = f(z);
    lab[0] = (116.0f * fy - 16.0f) / 100.0f;
    lab[1] = (500.0f * (fx - fy) + 128.0f) / 255.0f;
    lab[2] = (200.0f * (fy - fz) + 128.0f) / 255.0f;
}

VFI_YUV_FN bool aligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

constexpr int kDecPix = 4;             // luma columns per thread

// four consecutive bytes of one plane row as floats: one dword where the row is whole and the address allows
VFI_YUV_FN void load4(const unsigned char *p, int nvalid, float v[kDecPix]) {
    if (nvalid == kDecPix && aligned(p, 3)) {
        const unsigned u = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
        for (int k = 0; k < kDecPix; ++k) v[k] = (float)((u >> (8 * k)) & 255u);
    } else {
#pragma unroll
        for (int k = 0; k < kDecPix; ++k) v[k] = k < nvalid ? (float)p[k] : 0.0f;
    }
}

// One 4:2:0 chroma plane at the thread's 2 x 4 luma pixels.  Bytes times weights of 1/4 and 1/2 are exact in float32, so
// the order of the two interpolations and any contraction leave the bits alone.
template <bool LEFT>
VFI_YUV_FN void chroma420(const unsigned char *__restrict__ plane, int cw, const int row[3], const int col[4],
                          float out[2][kDecPix]) {
    float raw[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) raw[r][q] = (float)plane[(size_t)row[r] * cw + col[q]];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)          // even luma row: 1/4 above + 3/4 own; odd: 3/4 own + 1/4 below
            v[q] = r == 0 ? 0.25f * raw[0][q] + 0.75f * raw[1][q] : 0.75f * raw[1][q] + 0.25f * raw[2][q];
        if (LEFT) {                          // chroma sits on the even luma columns
            out[r][0] = v[1];
            out[r][1] = 0.5f * (v[1] + v[2]);
            out[r][2] = v[2];
            out[r][3] = 0.5f * (v[2] + v[3]);
        } else {                             // chroma sits between columns 2i and 2i + 1
            out[r][0] = 0.25f * v[0] + 0.75f * v[1];
            out[r][1] = 0.75f * v[1] + 0.25f * v[2];
            out[r][2] = 0.25f * v[1] + 0.75f * v[2];
            out[r][3] = 0.75f * v[2] + 0.25f * v[3];
        }
    }
}

VFI_YUV_FN float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// The block of the frame's grid at chroma row `ry` (luma rows R ry ... R ry + R - 1, R = 2 in 4:2:0) and luma columns
// x0 ... x0 + 3, x0 a multiple of 4 below W: the clamped rgb of its R x 4 pixels.  Columns at or beyond W (the row's tail)
// are computed from zero luma and never stored.  Chroma indices clamp at the frame's edges.
template <bool S420, bool LEFT>
VFI_YUV_FN void decode_block(const unsigned char *__restrict__ frame, int H, int W, const YuvCoef &k, int ry, int x0,
                             float px[S420 ? 2 : 1][kDecPix][3]) {
    constexpr int R = S420 ? 2 : 1;
    const int r0 = ry * R;
    const int nvalid = imin(kDecPix, W - x0);
    const size_t hw = (size_t)H * W;
    float Y[R][kDecPix], Cb[R][kDecPix], Cr[R][kDecPix];
#pragma unroll
    for (int r = 0; r < R; ++r) load4(frame + (size_t)(r0 + r) * W + x0, nvalid, Y[r]);
    if (S420) {
        const int cw = W / 2, ch = H / 2;
        const int row[3] = {imax(ry - 1, 0), ry, imin(ry + 1, ch - 1)};
        int col[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) col[q] = imin(imax(x0 / 2 - 1 + q, 0), cw - 1);
        chroma420<LEFT>(frame + hw, cw, row, col, Cb);
        chroma420<LEFT>(frame + hw + (size_t)cw * ch, cw, row, col, Cr);
    } else {
        load4(frame + hw + (size_t)r0 * W + x0, nvalid, Cb[0]);
        load4(frame + 2 * hw + (size_t)r0 * W + x0, nvalid, Cr[0]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int i = 0; i < kDecPix; ++i) {
            const float y = (Y[r][i] - k.y_off) / k.y_scale;
            const float cb = (Cb[r][i] - 128.0f) / k.c_scale, cr = (Cr[r][i] - 128.0f) / k.c_scale;
            const float red = y + k.r_cr * cr;
            const float blue = y + k.b_cb * cb;
            const float green = (y - k.kr * red - k.kb * blue) / k.kg;
            px[r][i][0] = clamp01(red); px[r][i][1] = clamp01(green); px[r][i][2] = clamp01(blue);
        }
    }
}

}  // namespace vfi_yuv
