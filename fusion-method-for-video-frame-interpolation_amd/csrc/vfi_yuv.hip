// Clip I/O: everything between the bytes of a YUV4MPEG2 frame and the tensors of the fused frame, in one launch each way.
//   decode  planar 8-bit Y'CbCr (4:2:0 or 4:4:4) -> bilinear chroma up-sampling -> range scaling -> colour matrix -> clamp
//           -> rgb (3, H, W) and the scaled Lab of rgb2lab_kernel (vfi_image.hip), written to up to two destinations
//   encode  rgb (3, H, W) -> clamp -> matrix -> chroma down-sampling -> quantisation -> the same byte layout
// Streaming passes: no LDS, no atomics, one writer per byte.  A decode thread owns four luma columns of one chroma row (two
// luma rows in 4:2:0), an encode thread eight; both move their bytes as dwords and their floats as float4 where the
// addresses allow, and one byte / one float at a time otherwise (row tails, frames or planes off their alignment).
#include "vfi_common.h"
#include "vfi_yuv_pixel.h"
#include <cstdint>

namespace {

using vfi::ceil_div;

using namespace vfi_yuv;     // YuvCoef, make_coef, load4, chroma420, clamp01, lab_of, decode_block, aligned, kDecPix (vfi_yuv_pixel.h)

// ---------------------------------------------------------------------------------------------------------------- decode

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
    float px[R][kDecPix][3];
    decode_block<S420, LEFT>(frame, H, W, k, ry, x0, px);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t at = (size_t)(r0 + r) * W + x0;
        if (rgb) store_planes(rgb, hw, at, px[r], nvalid);
        if (lab_a || lab_b) {
            float q[kDecPix][3];
#pragma unroll
            for (int i = 0; i < kDecPix; ++i) lab_of(px[r][i], q[i]);
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
