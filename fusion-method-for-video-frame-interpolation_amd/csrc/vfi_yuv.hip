// Clip I/O: everything between the bytes of a YUV4MPEG2 frame and the tensors of the fused frame, in one launch each way.
//   decode  planar 8-bit Y'CbCr (4:2:0 or 4:4:4) -> bilinear chroma up-sampling -> range scaling -> colour matrix -> clamp
//           -> rgb (3, H, W) and the scaled Lab of rgb2lab_kernel (vfi_image.hip), written to up to two destinations
//   encode  rgb (3, H, W) -> clamp -> matrix -> chroma down-sampling -> quantisation -> the same byte layout
// Streaming passes: no LDS, no atomics, one writer per byte.  A decode thread owns four luma columns of one chroma row (two
// luma rows in 4:2:0), an encode thread eight; both move their bytes as dwords and their floats as float4 where the
// addresses allow, and one byte / one float at a time otherwise (row tails, frames or planes off their alignment).
#include "vfi_common.h"
#include <cstdint>

namespace {

using vfi::ceil_div;

struct YuvCoef {
    float kr, kb, kg;                  // luma weights, kg = 1 - kr - kb
    float r_cr, b_cb;                  // 2 (1 - kr), 2 (1 - kb)
    float y_off, y_scale, c_scale;     // 16, 219, 224 (limited) | 0, 255, 255 (full)
    float y_lo, y_hi, c_lo, c_hi;      // the range's limits
};

YuvCoef make_coef(int matrix, int range) {
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

// the formulas of rgb2lab_kernel (vfi_image.hip), which stays as it is; the compiler may contract them differently here
__device__ __forceinline__ void lab_of(const float rgb[3], float lab[3]) {
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

__device__ __forceinline__ bool aligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

// ---------------------------------------------------------------------------------------------------------------- decode

constexpr int kDecPix = 4;             // luma columns per thread

// four consecutive bytes of one plane row as floats: one dword where the row is whole and the address allows
__device__ __forceinline__ void load4(const unsigned char *p, int nvalid, float v[kDecPix]) {
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
__device__ __forceinline__ void chroma420(const unsigned char *__restrict__ plane, int cw, const int row[3], const int col[4],
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

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__device__ __forceinline__ void store_planes(float *__restrict__ dst, size_t hw, size_t at, const float px[kDecPix][3], int nvalid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float *d = dst + c * hw + at;
        if (nvalid == kDecPix && aligned(d, 15)) {
            *reinterpret_cast<float4 *>(d) = make_float4(px[0][c], px[1][c], px[2][c], px[3][c]);
        } else {
#pragma unroll
            for (int k = 0; k < kDecPix; ++k)
                if (k < nvalid) d[k] = px[k][c];
        }
    }
}

// grid: x = groups of four luma columns of one chroma row (ceil(W / 4) * H / R, 256 per workgroup), R = 2 rows in 4:2:0
template <bool S420, bool LEFT>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const unsigned char *__restrict__ frame, int H, int W, YuvCoef k,
                                                         float *__restrict__ rgb, float *__restrict__ lab_a, float *__restrict__ lab_b) {
    constexpr int R = S420 ? 2 : 1;
    const int gw = ceil_div(W, kDecPix);
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)gw * (H / R)) return;
    const int ry = (int)(g / gw), x0 = (int)(g - (long long)ry * gw) * kDecPix, r0 = ry * R;
    const int nvalid = min(kDecPix, W - x0);
    const size_t hw = (size_t)H * W;
    float Y[R][kDecPix], Cb[R][kDecPix], Cr[R][kDecPix];
#pragma unroll
    for (int r = 0; r < R; ++r) load4(frame + (size_t)(r0 + r) * W + x0, nvalid, Y[r]);
    if (S420) {
        const int cw = W / 2, ch = H / 2;
        const int row[3] = {max(ry - 1, 0), ry, min(ry + 1, ch - 1)};
        int col[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) col[q] = min(max(x0 / 2 - 1 + q, 0), cw - 1);
        chroma420<LEFT>(frame + hw, cw, row, col, Cb);
        chroma420<LEFT>(frame + hw + (size_t)cw * ch, cw, row, col, Cr);
    } else {
        load4(frame + hw + (size_t)r0 * W + x0, nvalid, Cb[0]);
        load4(frame + 2 * hw + (size_t)r0 * W + x0, nvalid, Cr[0]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float px[kDecPix][3];
#pragma unroll
        for (int i = 0; i < kDecPix; ++i) {
            const float y = (Y[r][i] - k.y_off) / k.y_scale;
            const float cb = (Cb[r][i] - 128.0f) / k.c_scale, cr = (Cr[r][i] - 128.0f) / k.c_scale;
            const float red = y + k.r_cr * cr;
            const float blue = y + k.b_cb * cb;
            const float green = (y - k.kr * red - k.kb * blue) / k.kg;
            px[i][0] = clamp01(red); px[i][1] = clamp01(green); px[i][2] = clamp01(blue);
        }
        const size_t at = (size_t)(r0 + r) * W + x0;
        if (rgb) store_planes(rgb, hw, at, px, nvalid);
        if (lab_a || lab_b) {
            float q[kDecPix][3];
#pragma unroll
            for (int i = 0; i < kDecPix; ++i) lab_of(px[i], q[i]);
            if (lab_a) store_planes(lab_a, hw, at, q, nvalid);
            if (lab_b) store_planes(lab_b, hw, at, q, nvalid);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- encode

constexpr int kEncPix = 8;             // luma columns per thread

// NaN passes through (both comparisons are false): the quantiser turns it into the range's lower limit
__device__ __forceinline__ float clamp01_nan(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// floor(v + 0.5) clamped to [lo, hi]; NaN -> lo
__device__ __forceinline__ unsigned quantise(float v, float lo, float hi) {
    const float q = floorf(v + 0.5f);
    return (unsigned)(!(q >= lo) ? lo : (q > hi ? hi : q));
}

// n <= 8 consecutive bytes, packed little-endian in (lo, hi): one dwordx2 or dwords where whole and aligned, else bytes
__device__ __forceinline__ void store_bytes(unsigned char *p, unsigned lo, unsigned hi, int n) {
    if (n == 8 && aligned(p, 7)) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(lo, hi);
    } else if (n >= 4 && aligned(p, 3)) {
        *reinterpret_cast<unsigned *>(p) = lo;
        if (n == 8) {
            *reinterpret_cast<unsigned *>(p + 4) = hi;
        } else {
            for (int k = 4; k < n; ++k) p[k] = (unsigned char)(hi >> (8 * (k - 4)));
        }
    } else {
        for (int k = 0; k < n; ++k) p[k] = (unsigned char)((k < 4 ? lo >> (8 * k) : hi >> (8 * (k - 4))));
    }
}

// grid: x = groups of eight luma columns of one chroma row (ceil(W / 8) * H / R, 256 per workgroup).  In 4:2:0 the thread
// owns the 2 x 2 luma blocks of its four chroma samples; left siting reads the column before the group once more.
template <bool S420, bool LEFT>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const float *__restrict__ rgb, int H, int W, YuvCoef k,
                                                         unsigned char *__restrict__ frame) {
    constexpr int R = S420 ? 2 : 1;
    constexpr int P = kEncPix + 1;       // slot 0: column x0 - 1 (clamped), slots 1 ... 8: the group
    const int gw = ceil_div(W, kEncPix);
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)gw * (H / R)) return;
    const int ry = (int)(g / gw), x0 = (int)(g - (long long)ry * gw) * kEncPix, r0 = ry * R;
    const int nvalid = min(kEncPix, W - x0);
    const size_t hw = (size_t)H * W;
    float cb[R][P], cr[R][P];
    unsigned ylo[R], yhi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float *row = rgb + (size_t)(r0 + r) * W;
        float in[3][P];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *s = row + c * hw + x0;
#pragma unroll
            for (int q = 0; q < kEncPix / 4; ++q) {
                if (4 * q + 4 <= nvalid && aligned(s + 4 * q, 15)) {
                    const float4 v = *reinterpret_cast<const float4 *>(s + 4 * q);
                    in[c][1 + 4 * q] = v.x; in[c][2 + 4 * q] = v.y; in[c][3 + 4 * q] = v.z; in[c][4 + 4 * q] = v.w;
                } else {
#pragma unroll
                    for (int i = 4 * q; i < 4 * q + 4; ++i) in[c][1 + i] = i < nvalid ? s[i] : 0.0f;
                }
            }
            in[c][0] = (S420 && LEFT) ? row[c * hw + max(x0 - 1, 0)] : 0.0f;
        }
        ylo[r] = yhi[r] = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const float red = clamp01_nan(in[0][i]), green = clamp01_nan(in[1][i]), blue = clamp01_nan(in[2][i]);
            const float y = k.kr * red + k.kg * green + k.kb * blue;
            cb[r][i] = (blue - y) / k.b_cb;
            cr[r][i] = (red - y) / k.r_cr;
            if (i >= 1) {
                const unsigned b = quantise(k.y_off + k.y_scale * y, k.y_lo, k.y_hi);
                if (i <= 4) ylo[r] |= b << (8 * (i - 1)); else yhi[r] |= b << (8 * (i - 5));
            }
        }
        store_bytes(frame + (size_t)(r0 + r) * W + x0, ylo[r], yhi[r], nvalid);
    }
    if (S420) {
        const int cw = W / 2, ch = H / 2, nc = nvalid / 2;       // (W is even: the group ends on a whole chroma sample)
        unsigned pcb = 0, pcr = 0;
#pragma unroll
        for (int i = 0; i < kEncPix / 2; ++i) {
            float b, r;
            if (LEFT) {
                b = (0.5f * (cb[0][2 * i] + cb[1][2 * i]) + 2.0f * (0.5f * (cb[0][2 * i + 1] + cb[1][2 * i + 1])) +
                     0.5f * (cb[0][2 * i + 2] + cb[1][2 * i + 2])) * 0.25f;
                r = (0.5f * (cr[0][2 * i] + cr[1][2 * i]) + 2.0f * (0.5f * (cr[0][2 * i + 1] + cr[1][2 * i + 1])) +
                     0.5f * (cr[0][2 * i + 2] + cr[1][2 * i + 2])) * 0.25f;
            } else {
                b = 0.5f * (0.5f * (cb[0][2 * i + 1] + cb[1][2 * i + 1]) + 0.5f * (cb[0][2 * i + 2] + cb[1][2 * i + 2]));
                r = 0.5f * (0.5f * (cr[0][2 * i + 1] + cr[1][2 * i + 1]) + 0.5f * (cr[0][2 * i + 2] + cr[1][2 * i + 2]));
            }
            pcb |= quantise(128.0f + k.c_scale * b, k.c_lo, k.c_hi) << (8 * i);
            pcr |= quantise(128.0f + k.c_scale * r, k.c_lo, k.c_hi) << (8 * i);
        }
        unsigned char *pb = frame + hw + (size_t)ry * cw + x0 / 2;
        store_bytes(pb, pcb, 0, nc);
        store_bytes(pb + (size_t)cw * ch, pcr, 0, nc);
    } else {
        unsigned blo = 0, bhi = 0, rlo = 0, rhi = 0;
#pragma unroll
        for (int i = 0; i < kEncPix; ++i) {
            const unsigned b = quantise(128.0f + k.c_scale * cb[0][i + 1], k.c_lo, k.c_hi);
            const unsigned r = quantise(128.0f + k.c_scale * cr[0][i + 1], k.c_lo, k.c_hi);
            if (i < 4) { blo |= b << (8 * i); rlo |= r << (8 * i); } else { bhi |= b << (8 * (i - 4)); rhi |= r << (8 * (i - 4)); }
        }
        unsigned char *pb = frame + hw + (size_t)r0 * W + x0;
        store_bytes(pb, blo, bhi, nvalid);
        store_bytes(pb + hw, rlo, rhi, nvalid);
    }
}

// refusals shared by both directions, in the header's order; 0 = accepted
int check_format(const char *who, const void *a, const void *b, int H, int W, const int *format) {
    VFI_REQUIRE(a && b && format, VFI_ERR_INVALID_ARG, "%s: null pointer", who);
    VFI_REQUIRE(H > 0 && W > 0, VFI_ERR_INVALID_ARG, "%s: bad size %dx%d", who, H, W);
    VFI_REQUIRE(format[0] == VFI_YUV_420 || format[0] == VFI_YUV_444, VFI_ERR_INVALID_ARG, "%s: unknown subsampling %d", who, format[0]);
    VFI_REQUIRE(format[1] == VFI_YUV_SITING_CENTRE || format[1] == VFI_YUV_SITING_LEFT, VFI_ERR_INVALID_ARG, "%s: unknown chroma siting %d", who, format[1]);
    VFI_REQUIRE(format[2] == VFI_YUV_BT709 || format[2] == VFI_YUV_BT601, VFI_ERR_INVALID_ARG, "%s: unknown matrix %d", who, format[2]);
    VFI_REQUIRE(format[3] == VFI_YUV_LIMITED || format[3] == VFI_YUV_FULL, VFI_ERR_INVALID_ARG, "%s: unknown range %d", who, format[3]);
    VFI_REQUIRE(format[0] != VFI_YUV_420 || (H % 2 == 0 && W % 2 == 0), VFI_ERR_SHAPE, "%s: 4:2:0 needs even sizes, got %dx%d", who, H, W);
    VFI_REQUIRE((long long)H * W < (1ll << 31), VFI_ERR_UNSUPPORTED, "%s: %dx%d has 2^31 pixels or more", who, H, W);
    return VFI_OK;
}

}  // namespace

extern "C" int vfi_yuv_to_rgb(const unsigned char *frame, int H, int W, const int *format, float *rgb, float *lab_a, float *lab_b,
                              vfi_stream_t stream) {
    if (int e = check_format("vfi_yuv_to_rgb", frame, format, H, W, format)) return e;
    VFI_REQUIRE(rgb || lab_a || lab_b, VFI_ERR_INVALID_ARG, "vfi_yuv_to_rgb: all three outputs are NULL");
    const bool s420 = format[0] == VFI_YUV_420, left = format[1] == VFI_YUV_SITING_LEFT;
    const YuvCoef k = make_coef(format[2], format[3]);
    const long long groups = (long long)ceil_div(W, kDecPix) * (H / (s420 ? 2 : 1));
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    hipStream_t s = vfi::as_stream(stream);
    if (!s420) hipLaunchKernelGGL((yuv_to_rgb_kernel<false, false>), grid, block, 0, s, frame, H, W, k, rgb, lab_a, lab_b);
    else if (left) hipLaunchKernelGGL((yuv_to_rgb_kernel<true, true>), grid, block, 0, s, frame, H, W, k, rgb, lab_a, lab_b);
    else hipLaunchKernelGGL((yuv_to_rgb_kernel<true, false>), grid, block, 0, s, frame, H, W, k, rgb, lab_a, lab_b);
    return vfi::check_launch("vfi_yuv_to_rgb");
}

extern "C" int vfi_rgb_to_yuv(const float *rgb, int H, int W, const int *format, unsigned char *frame, vfi_stream_t stream) {
    if (int e = check_format("vfi_rgb_to_yuv", rgb, frame, H, W, format)) return e;
    const bool s420 = format[0] == VFI_YUV_420, left = format[1] == VFI_YUV_SITING_LEFT;
    const YuvCoef k = make_coef(format[2], format[3]);
    const long long groups = (long long)ceil_div(W, kEncPix) * (H / (s420 ? 2 : 1));
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    hipStream_t s = vfi::as_stream(stream);
    if (!s420) hipLaunchKernelGGL((rgb_to_yuv_kernel<false, false>), grid, block, 0, s, rgb, H, W, k, frame);
    else if (left) hipLaunchKernelGGL((rgb_to_yuv_kernel<true, true>), grid, block, 0, s, rgb, H, W, k, frame);
    else hipLaunchKernelGGL((rgb_to_yuv_kernel<true, false>), grid, block, 0, s, rgb, H, W, k, frame);
    return vfi::check_launch("vfi_rgb_to_yuv");
}
