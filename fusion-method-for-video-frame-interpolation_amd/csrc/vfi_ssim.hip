// SSIM as a loss (gfx950): 1 - mean SSIM per image in one pass over x and y, its adjoint in gather form, and the adjoint of
// the average pooling piq puts in front.  DESIGN.md section 26.
//
//   mu_x = G*x, mu_y = G*y, Exx = G*x^2, Eyy = G*y^2, Exy = G*xy        (G: separable Gaussian, valid region only)
//   sxx = Exx - mu_x^2, syy = Eyy - mu_y^2, sxy = Exy - mu_x mu_y
//   ssim = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * (2 sxy + c2) / (sxx + syy + c2)
//   out[n] = 1 / count * sum over C * (H - 2r) * (W - 2r) of (1 - ssim)
//
// Both kernels cut a plane into tiles of T x T (T = kTile = 32) and give a block of 256 threads one tile at a time.  The
// forward tile is T x T pixels of the SSIM map: x and y on T + 2r are staged in LDS, the five moments are summed along the
// rows into LDS (T + 2r rows of T columns), then down the columns in registers, four rows of one column per thread, and
// the map is added to the thread's sum; the moments never leave the CU.  The backward tile is T x T pixels of grad_x: x and
// y on T + 4r, the moments and the three derivative maps A, B, Cm (below) on T + 2r, zero outside the valid region, and
// their correlation with G down to T.  Consecutive lanes walk consecutive columns in every pass.
//
// Rules of vfi_grad_common.h: no float atomics, one writer per element, and an order of summation fixed by (C, H, W) alone:
// every image has its own blocks and its own partials, so the bits of image n depend neither on N nor on n.  E[xx], E[yy]
// and E[xy] go through one instruction sequence (fmaf of the tap and the product), every other contraction is off, and
// 1 - ssim is what is summed: x == y gives (2s + c2) / (s + s + c2) = 1 and (2p + c1) / (p + p + c1) = 1 with equal
// operands, so every summand and the value are exactly 0.
#include "vfi_grad_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 32;            // T
constexpr int kMaxRadius = 5;        // kernel_size 3 ... 11
constexpr int kImagesPerLaunch = VFI_REDUCE_WORKSPACE_FLOATS / kMaxPartials;     // partials of 4 images fit the workspace
static_assert(kThreads == 8 * kTile, "a block is eight row groups of T columns");

struct Taps { float w[2 * kMaxRadius + 1]; };     // made on the host in double, rounded once

// x and y on rows [r0, r0 + ROWS) x columns [c0, c0 + COLS) of a plane, 0 outside it
template <int ROWS, int COLS>
__device__ __forceinline__ void load_tile(const float *__restrict__ xp, const float *__restrict__ yp, int H, int W, int r0,
                                          int c0, float *sx, float *sy) {
    for (int i = threadIdx.x; i < ROWS * COLS; i += kThreads) {
        const int rr = i / COLS, gr = r0 + rr, gc = c0 + (i - rr * COLS);
        const bool in = gr >= 0 && gr < H && gc >= 0 && gc < W;
        const size_t o = in ? (size_t)gr * W + gc : 0;
        sx[i] = in ? xp[o] : 0.0f;
        sy[i] = in ? yp[o] : 0.0f;
    }
}

// hm[q][row][col] = sum_k g[k] M_q[row][col + k], M = (x, y, xx, yy, xy), for ROWS rows of OUT columns of a tile IN wide
template <int R, int ROWS, int IN, int OUT>
__device__ __forceinline__ void moments_along_rows(const float *sx, const float *sy, const Taps &g, float *hm) {
    for (int i = threadIdx.x; i < ROWS * OUT; i += kThreads) {
        const int row = i / OUT, base = row * IN + (i - row * OUT);
        float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const float a = sx[base + k], b = sy[base + k], w = g.w[k];
            m[0] = fmaf(w, a, m[0]);
            m[1] = fmaf(w, b, m[1]);
            m[2] = fmaf(w, a * a, m[2]);
            m[3] = fmaf(w, b * b, m[3]);
            m[4] = fmaf(w, a * b, m[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hm[q * ROWS * OUT + i] = m[q];
    }
}

// acc[o][q] = sum_k g[FLIP ? 2R - k : k] src[q][row0 + o + k][col] for RB consecutive rows o of one column; src holds NQ
// planes of IN_ROWS rows of `cols` columns.  A row is read once and feeds every output it belongs to.
template <int R, int RB, int NQ, int IN_ROWS, bool FLIP>
__device__ __forceinline__ void sum_down_column(const float *src, int cols, int col, int row0, const Taps &g, float (&acc)[RB][NQ]) {
#pragma unroll
    for (int o = 0; o < RB; ++o)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[o][q] = 0.0f;
#pragma unroll
    for (int j = 0; j < RB + 2 * R; ++j) {
        if (row0 + j < IN_ROWS) {
            float v[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) v[q] = src[(q * IN_ROWS + row0 + j) * cols + col];
#pragma unroll
            for (int o = 0; o < RB; ++o) {
                const int k = j - o;
                if (k >= 0 && k <= 2 * R) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[o][q] = fmaf(g.w[FLIP ? 2 * R - k : k], v[q], acc[o][q]);
                }
            }
        }
    }
}

// the two factors and what the derivatives share, from the five moments m = (mu_x, mu_y, Exx, Eyy, Exy)
struct Point { float l, cs, d1, d2; };
__device__ __forceinline__ Point ssim_point(const float *m, float c1, float c2) {
    const float mx = m[0], my = m[1];
    const float sxx = fmaf(-mx, mx, m[2]), syy = fmaf(-my, my, m[3]), sxy = fmaf(-mx, my, m[4]);
    Point p;
    p.d1 = mx * mx + my * my + c1;
    p.d2 = sxx + syy + c2;
    p.l = (2.0f * (mx * my) + c1) / p.d1;
    p.cs = (2.0f * sxy + c2) / p.d2;
    return p;
}

// stage 1: part[img * gridDim.x + block] = sum over the block's tiles of (1 - ssim)
template <int R>
__global__ __launch_bounds__(kThreads) void ssim_partial_kernel(const float *__restrict__ x, long long x_bs,
                                                                const float *__restrict__ y, long long y_bs, Taps g, int C, int H,
                                                                int W, int tiles_y, int tiles_x, float c1, float c2,
                                                                float *__restrict__ part) {
    constexpr int IN = kTile + 2 * R;
    __shared__ float sx[IN * IN], sy[IN * IN], hm[5 * IN * kTile];
    const int Hv = H - 2 * R, Wv = W - 2 * R, col = threadIdx.x % kTile, rg = threadIdx.x / kTile;
    const int per_plane = tiles_y * tiles_x, total = C * per_plane;
    const float *xn = x + (long long)blockIdx.y * x_bs, *yn = y + (long long)blockIdx.y * y_bs;
    float sum[1] = {0.0f};
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int c = t / per_plane, ty = (t - c * per_plane) / tiles_x, tx = t - c * per_plane - ty * tiles_x;
        const int r0 = ty * kTile, c0 = tx * kTile;
        const size_t plane = (size_t)c * H * W;
        __syncthreads();                                   // the previous tile's readers are done with sx, sy, hm
        load_tile<IN, IN>(xn + plane, yn + plane, H, W, r0, c0, sx, sy);
        __syncthreads();
        moments_along_rows<R, IN, IN, kTile>(sx, sy, g, hm);
        __syncthreads();
        float m[4][5];
        sum_down_column<R, 4, 5, IN, false>(hm, kTile, col, rg * 4, g, m);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (r0 + rg * 4 + o < Hv && c0 + col < Wv) {
                const Point p = ssim_point(m[o], c1, c2);
                sum[0] += 1.0f - p.l * p.cs;
            }
        }
    }
    __syncthreads();
    block_sum<1>(sum, hm);
    if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = sum[0];
}

// stage 2 (one block per image): out[n] = (sum of the image's partials) / count
__global__ __launch_bounds__(kThreads) void ssim_final_kernel(const float *__restrict__ part, int blocks, float count,
                                                              float *__restrict__ out) {
    __shared__ float lds[kThreads];
    float v[1] = {0.0f};
    for (int b = threadIdx.x; b < blocks; b += kThreads) v[0] += part[(long long)blockIdx.x * blocks + b];
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = v[0] / count;
}

// grad_x(q) = -up[n] / count * ((G (*) A)(q) + 2 x(q) (G (*) B)(q) + y(q) (G (*) Cm)(q)), (*) the full correlation of the maps
// A = d ssim / d mu_x (through the chain: mu_x enters sxx and sxy as well), B = d ssim / d Exx, Cm = d ssim / d Exy, each
// zero outside the valid region: a pixel q of the image lies in the windows of the valid pixels q - 2r ... q, and the one
// at p weighs it with g[q - p].  LDS: region P holds x and y on T + 4r, later A, B, Cm on T + 2r; region Q the five row sums
// (T + 4r rows of T + 2r columns), later the row sums of A, B, Cm (T + 2r rows of T columns).
template <int R>
__global__ __launch_bounds__(kThreads) void ssim_backward_kernel(const float *__restrict__ x, long long x_bs,
                                                                 const float *__restrict__ y, long long y_bs,
                                                                 const float *__restrict__ up, float *__restrict__ gx,
                                                                 long long g_bs, Taps g, int C, int H, int W, int tiles_y,
                                                                 int tiles_x, float c1, float c2, float count) {
    constexpr int IN = kTile + 4 * R, MID = kTile + 2 * R;
    constexpr int GROUPS = kThreads / MID, RB = (MID + GROUPS - 1) / GROUPS;     // R = 5: 6 groups of 7 rows of the 42
    constexpr int PN = 2 * IN * IN > 3 * MID * MID ? 2 * IN * IN : 3 * MID * MID;      // R = 5: 5408 + 10920 floats, 65312 bytes
    static_assert(3 * MID * kTile <= 5 * IN * MID && GROUPS * RB >= MID, "the row sums of A, B, Cm fit Q; the groups cover MID rows");
    __shared__ float P[PN], Q[5 * IN * MID];
    float *sx = P, *sy = P + IN * IN;
    const int Hv = H - 2 * R, Wv = W - 2 * R;
    const int per_plane = tiles_y * tiles_x;
    const long long i = blockIdx.x;                    // one tile per block: the grid is N * C * tiles
    const int n = (int)(i / ((long long)C * per_plane)), t = (int)(i - (long long)n * C * per_plane);
    const int c = t / per_plane, ty = (t - c * per_plane) / tiles_x, tx = t - c * per_plane - ty * tiles_x;
    const int q0r = ty * kTile, q0c = tx * kTile;
    const size_t plane = (size_t)c * H * W;
    const float *xp = x + (long long)n * x_bs + plane, *yp = y + (long long)n * y_bs + plane;
    load_tile<IN, IN>(xp, yp, H, W, q0r - 2 * R, q0c - 2 * R, sx, sy);
    __syncthreads();
    moments_along_rows<R, IN, IN, MID>(sx, sy, g, Q);
    __syncthreads();
    // the moments of RB rows of one column of the T + 2r square, and A, B, Cm there
    const int mcol = threadIdx.x % MID, mrg = threadIdx.x / MID;
    float abc[RB][3];
    if (mrg < GROUPS) {
        float m[RB][5];
        sum_down_column<R, RB, 5, IN, false>(Q, MID, mcol, mrg * RB, g, m);
#pragma unroll
        for (int o = 0; o < RB; ++o) {
            const int pr = q0r - 2 * R + mrg * RB + o, pc = q0c - 2 * R + mcol;
            const bool valid = pr >= 0 && pr < Hv && pc >= 0 && pc < Wv;
            const Point p = ssim_point(m[o], c1, c2);
            const float mx = m[o][0], my = m[o][1];
            const float B = -(p.l * p.cs) / p.d2, Cm = 2.0f * p.l / p.d2;
            const float A = p.cs * (2.0f / p.d1) * (my - mx * p.l) - 2.0f * mx * B - my * Cm;
            abc[o][0] = valid ? A : 0.0f;
            abc[o][1] = valid ? B : 0.0f;
            abc[o][2] = valid ? Cm : 0.0f;
        }
    }
    __syncthreads();                                   // every read of Q above is done; x and y in P were read before it
    if (mrg < GROUPS) {
#pragma unroll
        for (int o = 0; o < RB; ++o) {
            const int row = mrg * RB + o;
            if (row < MID) {
#pragma unroll
                for (int q = 0; q < 3; ++q) P[(q * MID + row) * MID + mcol] = abc[o][q];
            }
        }
    }
    __syncthreads();
    // along the rows: Q[q][row][col] = sum_t g[2r - t] P[q][row][col + t]
    for (int e = threadIdx.x; e < MID * kTile; e += kThreads) {
        const int row = e / kTile, base = row * MID + (e - row * kTile);
        float s[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
#pragma unroll
            for (int q = 0; q < 3; ++q) s[q] = fmaf(g.w[2 * R - k], P[q * MID * MID + base + k], s[q]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) Q[q * MID * kTile + e] = s[q];
    }
    __syncthreads();
    const int col = threadIdx.x % kTile, rg = threadIdx.x / kTile;
    float v[4][3];
    sum_down_column<R, 4, 3, MID, true>(Q, kTile, col, rg * 4, g, v);
    const float scale = -(up[n] / count);
    float *gp = gx + (long long)n * g_bs + plane;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int qr = q0r + rg * 4 + o, qc = q0c + col;
        if (qr < H && qc < W) {
            const size_t e = (size_t)qr * W + qc;
            gp[e] = scale * (v[o][0] + 2.0f * xp[e] * v[o][1] + yp[e] * v[o][2]);
        }
    }
}

// adjoint of F.avg_pool2d(kernel_size=f): every pixel of a window gets g / f^2, the rows and columns the floor drops get 0
__global__ void avg_pool_backward_kernel(const float *__restrict__ g, float *__restrict__ gx, int planes, int H, int W, int f) {
    const int Ho = H / f, Wo = W / f;
    const float inv = 1.0f / (float)(f * f);
    GRID_STRIDE(i, (long long)planes * H * W) {
        const int xi = (int)(i % W), yi = (int)((i / W) % H);
        const long long p = i / ((long long)W * H);
        const int xo = xi / f, yo = yi / f;
        gx[i] = (xo < Wo && yo < Ho) ? g[(p * Ho + yo) * Wo + xo] * inv : 0.0f;
    }
}

int check_ssim_args(const char *what, int N, int C, int H, int W, int kernel_size, float sigma, long long x_bs, long long y_bs) {
    VFI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= (1LL << 30) && (long long)C * H * W <= (1LL << 40),
                VFI_ERR_INVALID_ARG, "%s: bad sizes", what);
    VFI_REQUIRE(kernel_size >= 3 && kernel_size <= 2 * kMaxRadius + 1 && (kernel_size & 1), VFI_ERR_INVALID_ARG,
                "%s: kernel_size %d is not an odd number from 3 to %d", what, kernel_size, 2 * kMaxRadius + 1);
    VFI_REQUIRE(sigma > 0.0f && std::isfinite(sigma), VFI_ERR_INVALID_ARG, "%s: sigma must be positive", what);
    VFI_REQUIRE(H >= kernel_size && W >= kernel_size, VFI_ERR_SHAPE, "%s: a %dx%d plane is smaller than the %d-tap window", what,
                H, W, kernel_size);
    const long long chw = (long long)C * H * W;
    VFI_REQUIRE(chw <= x_bs && chw <= y_bs, VFI_ERR_INVALID_ARG, "%s: a batch stride below C * H * W", what);
    return VFI_OK;
}

Taps make_taps(int kernel_size, float sigma) {
    const int r = kernel_size / 2;
    double w[2 * kMaxRadius + 1], s = 0.0;
    for (int i = 0; i < kernel_size; ++i) s += w[i] = std::exp(-(double)((i - r) * (i - r)) / (2.0 * (double)sigma * (double)sigma));
    Taps t = {};
    for (int i = 0; i < kernel_size; ++i) t.w[i] = (float)(w[i] / s);
    return t;
}

#define SSIM_BY_RADIUS(r, CALL) \
    do {                        \
        if ((r) == 1) { CALL(1); } else if ((r) == 2) { CALL(2); } else if ((r) == 3) { CALL(3); } else if ((r) == 4) { CALL(4); } else { CALL(5); } \
    } while (0)

}  // namespace

extern "C" int vfi_ssim_loss_forward(const float *x, long long x_bstride, const float *y, long long y_bstride, float *out,
                                     float *workspace, int N, int C, int H, int W, int kernel_size, float sigma, float c1, float c2,
                                     vfi_stream_t stream) {
    VFI_REQUIRE(x && y && out && workspace, VFI_ERR_INVALID_ARG, "vfi_ssim_loss_forward: null pointer");
    if (int e = check_ssim_args("vfi_ssim_loss_forward", N, C, H, W, kernel_size, sigma, x_bstride, y_bstride)) return e;
    const int r = kernel_size / 2, Hv = H - 2 * r, Wv = W - 2 * r;
    const int tiles_y = (Hv + kTile - 1) / kTile, tiles_x = (Wv + kTile - 1) / kTile;
    const long long total = (long long)C * tiles_y * tiles_x;
    VFI_REQUIRE(total <= (1LL << 30), VFI_ERR_INVALID_ARG, "vfi_ssim_loss_forward: too many tiles");
    const int blocks = (int)(total < kMaxPartials ? total : kMaxPartials);      // by (C, H, W) alone
    const float count = (float)((double)C * Hv * Wv);
    const Taps g = make_taps(kernel_size, sigma);
    hipStream_t s = vfi::as_stream(stream);
    for (int n0 = 0; n0 < N; n0 += kImagesPerLaunch) {
        const int imgs = N - n0 < kImagesPerLaunch ? N - n0 : kImagesPerLaunch;
#define CALL(R)                                                                                                                 \
    hipLaunchKernelGGL(ssim_partial_kernel<R>, dim3(blocks, imgs), dim3(kThreads), 0, s, x + (long long)n0 * x_bstride, x_bstride, \
                       y + (long long)n0 * y_bstride, y_bstride, g, C, H, W, tiles_y, tiles_x, c1, c2, workspace)
        SSIM_BY_RADIUS(r, CALL);
#undef CALL
        hipLaunchKernelGGL(ssim_final_kernel, dim3(imgs), dim3(kThreads), 0, s, workspace, blocks, count, out + n0);
    }
    return vfi::check_launch("vfi_ssim_loss_forward");
}

extern "C" int vfi_ssim_loss_backward(const float *x, long long x_bstride, const float *y, long long y_bstride,
                                      const float *upstream, float *grad_x, long long gx_bstride, int N, int C, int H, int W,
                                      int kernel_size, float sigma, float c1, float c2, vfi_stream_t stream) {
    VFI_REQUIRE(x && y && upstream && grad_x, VFI_ERR_INVALID_ARG, "vfi_ssim_loss_backward: null pointer");
    if (int e = check_ssim_args("vfi_ssim_loss_backward", N, C, H, W, kernel_size, sigma, x_bstride, y_bstride)) return e;
    VFI_REQUIRE((long long)C * H * W <= gx_bstride, VFI_ERR_INVALID_ARG, "vfi_ssim_loss_backward: a batch stride below C * H * W");
    const int r = kernel_size / 2;
    const int tiles_y = (H + kTile - 1) / kTile, tiles_x = (W + kTile - 1) / kTile;
    const long long total = (long long)N * C * tiles_y * tiles_x;
    VFI_REQUIRE(total <= 0x7fffffffLL, VFI_ERR_INVALID_ARG, "vfi_ssim_loss_backward: too many tiles");
    const float count = (float)((double)C * (H - 2 * r) * (W - 2 * r));
    const Taps g = make_taps(kernel_size, sigma);
#define CALL(R)                                                                                                                  \
    hipLaunchKernelGGL(ssim_backward_kernel<R>, dim3((unsigned)total), dim3(kThreads), 0, vfi::as_stream(stream), x, x_bstride, y, \
                       y_bstride, upstream, grad_x, gx_bstride, g, C, H, W, tiles_y, tiles_x, c1, c2, count)
    SSIM_BY_RADIUS(r, CALL);
#undef CALL
    return vfi::check_launch("vfi_ssim_loss_backward");
}

extern "C" int vfi_avg_pool_backward(const float *grad, float *grad_x, int planes, int H, int W, int f, vfi_stream_t stream) {
    VFI_REQUIRE(grad && grad_x, VFI_ERR_INVALID_ARG, "vfi_avg_pool_backward: null pointer");
    VFI_REQUIRE(planes > 0 && f >= 1 && H >= f && W >= f, VFI_ERR_INVALID_ARG, "vfi_avg_pool_backward: bad sizes");
    LAUNCH_1D(avg_pool_backward_kernel, (long long)planes * H * W, stream, grad, grad_x, planes, H, W, f);
    return vfi::check_launch("vfi_avg_pool_backward");
}
