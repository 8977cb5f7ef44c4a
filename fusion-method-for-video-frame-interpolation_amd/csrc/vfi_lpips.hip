// The LPIPS head (gfx950): per tap, the weighted squared distance of two channel-normalised feature maps, and its
// adjoint with the ReLU mask of the tapped layer; and the ImageNet normalisation of the input.  DESIGN.md section 24.
//
//   xh_c = x_c / (sqrt(sum_k x_k^2) + 1e-10), yh likewise;   d[n] = 1 / HW * sum_p sum_c w_c (xh_c - yh_c)^2
//
// Both kernels see a map (N, C, HW) as tiles of PX pixels and give a block of 256 threads one tile at a time: thread
// (p, g) = (tid % PX, tid / PX) walks the channels g, g + CG, g + 2 CG, ... (CG = 256 / PX) of pixel p at stride HW.  With
// PX = 64 a wave reads one 256-byte row per channel; at the deep taps, whose planes are small, PX shrinks and the lanes
// of a block spread over the channels instead, so that a 32 x 32 (or 1 x 1) plane still fills its blocks.  PX is chosen by
// HW alone (tile_px).  The per-pixel sums over the channels are combined across the CG groups through LDS, in the order
// g = 0, 1, ..., by every thread of the pixel, so all of them hold the same bits.  The forward sweeps the channels twice
// (the norms, then the value), the backward three times (see there); every sweep after the first re-reads what the block
// has just read, a tile of PX * C * 8 bytes.
//
// Rules of vfi_grad_common.h: no float atomics, one writer per element, and an order of summation fixed by C and HW
// alone -- every image has its own blocks and its own partials, so the bits of image n's score depend neither on N nor
// on n.  x == y gives exactly 0 (value and gradient): x_c / s - y_c / t is formed by two divisions of equal operands.
// The file is compiled without fused contraction, so the sums are the products' roundings added, as written.
#include "vfi_grad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr float kLpipsEps = 1e-10f;
constexpr int kImagesPerLaunch = VFI_REDUCE_WORKSPACE_FLOATS / kMaxPartials;     // partials of 4 images fit the workspace

// pixels of a tile: by HW alone.  64 only where that still leaves a thousand tiles for the 256 CUs: at the 64 x 64 tap of a
// 512 x 512 crop (C = 512) tiles of 64 pixels are 64 blocks of 128 channels per thread, measured 43 us against the
// 23 us of the 32 x 32 tap below it
inline int tile_px(int HW) { return HW >= 65536 ? 64 : (HW >= 128 ? 16 : (HW >= 8 ? 4 : 1)); }

// v[q] <- sum over the CG channel groups of pixel p, in group order; every thread of the pixel gets the same bits
template <int NV, int PX> __device__ __forceinline__ void pixel_sum(float *v, float *lds) {
    constexpr int CG = kThreads / PX;
    const int p = threadIdx.x % PX;
    __syncthreads();                                   // the previous tile's readers are done with lds
#pragma unroll
    for (int q = 0; q < NV; ++q) lds[q * kThreads + threadIdx.x] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        float s = lds[q * kThreads + p];
        for (int g = 1; g < CG; ++g) s += lds[q * kThreads + g * PX + p];
        v[q] = s;
    }
}

// stage 1: part[img * gridDim.x + block] = sum over the block's tiles of sum_c w_c (xh_c - yh_c)^2
template <int PX>
__global__ __launch_bounds__(kThreads) void lpips_head_partial_kernel(const float *__restrict__ x, long long x_bs,
                                                                      const float *__restrict__ y, long long y_bs,
                                                                      const float *__restrict__ w, int C, int HW, int tiles,
                                                                      float *__restrict__ part) {
    constexpr int CG = kThreads / PX;
    __shared__ float lds[2 * kThreads];
    const int p = threadIdx.x % PX, g = threadIdx.x / PX;
    const float *xn = x + (long long)blockIdx.y * x_bs, *yn = y + (long long)blockIdx.y * y_bs;
    float acc[1] = {0.0f};
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int pix = t * PX + p;
        const bool live = pix < HW;
        float v[2] = {0.0f, 0.0f};
        if (live) {
#pragma unroll 4
            for (int c = g; c < C; c += CG) {
                const float a = xn[(long long)c * HW + pix], b = yn[(long long)c * HW + pix];
                v[0] += a * a;
                v[1] += b * b;
            }
        }
        pixel_sum<2, PX>(v, lds);
        if (live) {
            const float s = sqrtf(v[0]) + kLpipsEps, t = sqrtf(v[1]) + kLpipsEps;
            float d = 0.0f;
#pragma unroll 4
            for (int c = g; c < C; c += CG) {
                const float a = xn[(long long)c * HW + pix], b = yn[(long long)c * HW + pix];
                const float e = a / s - b / t;
                d += w[c] * (e * e);
            }
            acc[0] += d;
        }
    }
    __syncthreads();
    block_sum<1>(acc, lds);
    if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// stage 2 (one block per image): out[n] = prior[n] + (sum of the image's partials) / HW
__global__ __launch_bounds__(kThreads) void lpips_head_final_kernel(const float *__restrict__ part, int blocks, int HW,
                                                                    const float *prior, float *out) {
    __shared__ float lds[kThreads];
    float v[1] = {0.0f};
    for (int b = threadIdx.x; b < blocks; b += kThreads) v[0] += part[(long long)blockIdx.x * blocks + b];
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) {
        const float d = v[0] / (float)HW;
        out[blockIdx.x] = prior ? prior[blockIdx.x] + d : d;
    }
}

// gx = (above + u[n] / HW * (e_c / s - (sum_k e_k x_k) x_c / (|x| s^2))) [x > 0 when mask],  e_c = 2 w_c (x_c / s - y_c / t),
// s = |x| + eps, t = |y| + eps; the head's part is 0 where |x| = 0.  With the unit vector v = x / |x| and d = sum_k e_k v_k
// the bracket is 1 / s * ((e_c - v_c d) + eps / s * v_c d): the part of e orthogonal to x, and eps / s of the part along it.
// It is evaluated in that form, in three sweeps (the norms; d; the gradient).  At a pixel with one dominant channel e is
// nearly parallel to x and e_c / s and the projection cancel to a fraction eps / s of either; written as their difference,
// fp32 leaves an error of some ulps of e_c / s there, which at a small |x| is larger than the largest entry of the whole
// gradient (measured on the CPU, C = 2: 2.5e-7 of the largest entry, against 5e-8 for torch's fp32 autograd).  In the
// split form v_c is exactly 1 at a pixel with a single channel, the orthogonal part exactly 0, and what is left is exact
// to rounding.  Gathering sum_k e_k x_k in the first sweep from sum w x^2 / s - sum w x y / t loses more still (1.5e-6).
template <int PX>
__global__ __launch_bounds__(kThreads) void lpips_head_backward_kernel(const float *__restrict__ x, long long x_bs,
                                                                       const float *__restrict__ y, long long y_bs,
                                                                       const float *__restrict__ w, const float *__restrict__ up,
                                                                       const float *above, long long a_bs, float *gx,
                                                                       long long g_bs, int N, int C, int HW, int tiles, int mask) {
    constexpr int CG = kThreads / PX;
    __shared__ float lds[2 * kThreads];
    const int p = threadIdx.x % PX, g = threadIdx.x / PX;
    const long long total = (long long)N * tiles;
    for (long long i = blockIdx.x; i < total; i += gridDim.x) {
        const int n = (int)(i / tiles), pix = (int)(i - (long long)n * tiles) * PX + p;
        const bool live = pix < HW;
        const float *xn = x + (long long)n * x_bs, *yn = y + (long long)n * y_bs;
        float v[2] = {0.0f, 0.0f};
        if (live) {
#pragma unroll 4
            for (int c = g; c < C; c += CG) {
                const float a = xn[(long long)c * HW + pix], b = yn[(long long)c * HW + pix];
                v[0] += a * a;
                v[1] += b * b;
            }
        }
        pixel_sum<2, PX>(v, lds);
        const float nx = sqrtf(v[0]), s = nx + kLpipsEps, t = sqrtf(v[1]) + kLpipsEps, is = 1.0f / s;
        float dot[1] = {0.0f};
        if (live && nx > 0.0f) {
#pragma unroll 4
            for (int c = g; c < C; c += CG) {
                const float a = xn[(long long)c * HW + pix], b = yn[(long long)c * HW + pix];
                dot[0] += 2.0f * w[c] * (a / s - b / t) * (a / nx);
            }
        }
        pixel_sum<1, PX>(dot, lds);
        if (live) {
            const bool some = nx > 0.0f;
            const float k = some ? up[n] / (float)HW * is : 0.0f, along = kLpipsEps * is, d = dot[0];
            const float *an = above ? above + (long long)n * a_bs : nullptr;
            float *gn = gx + (long long)n * g_bs;
#pragma unroll 4
            for (int c = g; c < C; c += CG) {
                const long long o = (long long)c * HW + pix;
                const float a = xn[o], b = yn[o];
                const float e = 2.0f * w[c] * (a / s - b / t);
                const float vd = some ? a / nx * d : 0.0f;
                float r = k * ((e - vd) + along * vd);
                if (an) r = an[o] + r;
                gn[o] = (mask && !(a > 0.0f)) ? 0.0f : r;
            }
        }
    }
}

// (x - mean_c) / std_c of the [0, 1] image, or (adjoint) g / std_c; three channels
__global__ void lpips_normalize_kernel(const float *x, long long x_bs, float *out, long long o_bs,
                                       int N, int HW, int adjoint) {
    GRID_STRIDE(i, (long long)N * 3 * HW) {
        const long long n = i / (3LL * HW), e = i - n * 3LL * HW;
        const int c = (int)(e / HW);
        const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        const float v = x[n * x_bs + e];
        out[n * o_bs + e] = (adjoint ? v : v - mean) / sd;
    }
}

#define LPIPS_BY_PX(px, CALL) \
    do {                      \
        if ((px) == 64) { CALL(64); } else if ((px) == 16) { CALL(16); } else if ((px) == 4) { CALL(4); } else { CALL(1); } \
    } while (0)

}  // namespace

extern "C" int vfi_lpips_head_forward(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *w,
                                      const float *prior, float *out, float *workspace, int N, int C, int HW,
                                      vfi_stream_t stream) {
    VFI_REQUIRE(x && y && w && out && workspace, VFI_ERR_INVALID_ARG, "vfi_lpips_head_forward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && HW > 0 && HW <= (1 << 30), VFI_ERR_INVALID_ARG, "vfi_lpips_head_forward: bad sizes");
    VFI_REQUIRE((long long)C * HW <= x_bstride && (long long)C * HW <= y_bstride, VFI_ERR_INVALID_ARG,
                "vfi_lpips_head_forward: a batch stride below C * HW");
    const int px = tile_px(HW), tiles = (HW + px - 1) / px;
    const int blocks = tiles < kMaxPartials ? tiles : kMaxPartials;      // by HW alone
    hipStream_t s = vfi::as_stream(stream);
    for (int n0 = 0; n0 < N; n0 += kImagesPerLaunch) {
        const int imgs = N - n0 < kImagesPerLaunch ? N - n0 : kImagesPerLaunch;
#define CALL(PX)                                                                                                         \
    hipLaunchKernelGGL(lpips_head_partial_kernel<PX>, dim3(blocks, imgs), dim3(kThreads), 0, s, x + (long long)n0 * x_bstride, \
                       x_bstride, y + (long long)n0 * y_bstride, y_bstride, w, C, HW, tiles, workspace)
        LPIPS_BY_PX(px, CALL);
#undef CALL
        hipLaunchKernelGGL(lpips_head_final_kernel, dim3(imgs), dim3(kThreads), 0, s, workspace, blocks, HW,
                           prior ? prior + n0 : nullptr, out + n0);
    }
    return vfi::check_launch("vfi_lpips_head_forward");
}

extern "C" int vfi_lpips_head_backward(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *w,
                                       const float *upstream, const float *above, long long above_bstride, float *grad_x,
                                       long long gx_bstride, int N, int C, int HW, int relu_mask, vfi_stream_t stream) {
    VFI_REQUIRE(x && y && w && upstream && grad_x, VFI_ERR_INVALID_ARG, "vfi_lpips_head_backward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && HW > 0 && HW <= (1 << 30), VFI_ERR_INVALID_ARG, "vfi_lpips_head_backward: bad sizes");
    const long long chw = (long long)C * HW;
    VFI_REQUIRE(chw <= x_bstride && chw <= y_bstride && chw <= gx_bstride && (!above || chw <= above_bstride),
                VFI_ERR_INVALID_ARG, "vfi_lpips_head_backward: a batch stride below C * HW");
    const int px = tile_px(HW), tiles = (HW + px - 1) / px;
    const long long total = (long long)N * tiles;
    const int blocks = (int)(total < 16384 ? total : 16384);
#define CALL(PX)                                                                                                          \
    hipLaunchKernelGGL(lpips_head_backward_kernel<PX>, dim3(blocks), dim3(kThreads), 0, vfi::as_stream(stream), x, x_bstride, y, \
                       y_bstride, w, upstream, above, above_bstride, grad_x, gx_bstride, N, C, HW, tiles, relu_mask != 0)
    LPIPS_BY_PX(px, CALL);
#undef CALL
    return vfi::check_launch("vfi_lpips_head_backward");
}

extern "C" int vfi_lpips_normalize(const float *x, long long x_bstride, float *out, long long out_bstride, int N, int HW,
                                   int adjoint, vfi_stream_t stream) {
    VFI_REQUIRE(x && out, VFI_ERR_INVALID_ARG, "vfi_lpips_normalize: null pointer");
    VFI_REQUIRE(N > 0 && HW > 0 && HW <= (1 << 30) && 3LL * HW <= x_bstride && 3LL * HW <= out_bstride, VFI_ERR_INVALID_ARG,
                "vfi_lpips_normalize: bad sizes");
    LAUNCH_1D(lpips_normalize_kernel, (long long)N * 3 * HW, stream, x, x_bstride, out, out_bstride, N, HW, adjoint != 0);
    return vfi::check_launch("vfi_lpips_normalize");
}
