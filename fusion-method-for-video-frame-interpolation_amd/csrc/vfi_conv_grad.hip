// Backward of FusionNet's layers (gfx950): the convolution's weight gradient (fp32 MFMA, split-K over pixels with a
// fixed-order slab reduction: no float atomics, bit-reproducible), its input gradient (the forward convolution machinery on
// the transposed, flipped weights plus a padding fold) and the three HBM-bound glue adjoints (tanh + residual + clamp head,
// ReLU + max-pool encoder block, ReLU + bilinear x2 decoder resize).  Differentiates reference src/fusion_net/fusion_net.py
// :24-41 (layers) and :46-77 (forward).  The rules: vfi_grad_common.h.
#include "vfi_grad_common.h"

namespace {

using vfi::ceil_div;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- weight gradient --------------------------------------------------------------------------------------------
// GEMM dW[co][c] = sum_p dY[co][p] * B[p][c] with c = ci*KS*KS + ky*KS + kx (plain OIHW) and p = (n, y, x):
// B[p][c] = Xpad[n][ci][y+ky][x+kx].  One workgroup = 4 waves = 32 output channels x 128 columns (32 per wave, one
// v_mfma_f32_32x32x2_f32 accumulator each) over a contiguous run of TY x 32-pixel tiles.  Per tile, dY (32 x P, stored
// pixel-major with a 33-float row so the A reads of a wave hit 64 distinct banks) and the X window of the columns' input
// channels (with the KS-1 halo, reflect / zero padding resolved by the loader) are staged in LDS; the next tile's global
// loads are issued into registers before the current tile's MFMAs.  Each workgroup writes its partial 32 x 128 block to
// its own slab of the workspace; slab_reduce_kernel sums the slabs in slab order.
constexpr int kWgCols = 128, kWgTX = 32, kYStride = 33;

template <int KS> struct WgradCfg {
    static constexpr int TY = KS == 1 ? 1 : 4;                 // 1x1: 32-pixel tiles keep 128 input channels in LDS
    static constexpr int P = TY * kWgTX;                       // pixels per tile
    static constexpr int K2 = KS * KS;
    static constexpr int RH = TY + KS - 1, RW = kWgTX + KS - 1;
    static constexpr int NCI = (kWgCols - 1) / K2 + 2 < kWgCols ? (kWgCols - 1) / K2 + 2 : kWgCols;  // input channels a block spans
    static constexpr int NX = NCI * RH * RW;                   // X window floats
    static constexpr int RX = (NX + kThreads - 1) / kThreads;  // per-thread loads
    static constexpr int RY = 32 * P / kThreads;
};

template <int KS>
__global__ __launch_bounds__(kThreads) void conv_wgrad_kernel(const float *__restrict__ x, long long x_bs,
                                                              const float *__restrict__ dy, long long dy_bs,
                                                              float *__restrict__ part_w, float *__restrict__ part_b,
                                                              int Cin, int H, int W, int Cout, int pad_mode, int tiles_x,
                                                              int tiles_y, int tiles_total, int tiles_per_split) {
    using C = WgradCfg<KS>;
    constexpr int pad = (KS - 1) / 2;
    __shared__ float sX[C::NX];
    __shared__ float sY[C::P * kYStride];
    __shared__ float sB[8 * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5;
    const int Ncols = Cin * C::K2;
    const int c0 = blockIdx.x * kWgCols, co0 = blockIdx.y * 32, split = blockIdx.z;
    const int ci0 = c0 / C::K2;
    const int t_begin = split * tiles_per_split;
    const int t_end = min(t_begin + tiles_per_split, tiles_total);
    const bool do_bias = part_b != nullptr && blockIdx.x == 0;
    const long long HW = (long long)H * W;

    // this lane's B column -> offset of its (ci, ky, kx) in the X window
    const int j = c0 + wave * 32 + (lane & 31);
    int off = 0;
    if (j < Ncols) {
        const int ci_l = j / C::K2 - ci0, tap = j % C::K2;
        off = (ci_l * C::RH + tap / KS) * C::RW + tap % KS;
    }
    const float *sXb = sX + off + hi;
    const float *sYb = sY + hi * kYStride + (lane & 31);

    float rx[C::RX], ry[C::RY];
    auto load = [&](int t) {
        const int txi = t % tiles_x, tyi = (t / tiles_x) % tiles_y, n = t / (tiles_x * tiles_y);
        const int y0 = tyi * C::TY, x0 = txi * kWgTX;
        const float *xn = x + (size_t)n * x_bs;
#pragma unroll
        for (int r = 0; r < C::RX; ++r) {
            const int e = tid + r * kThreads;
            float v = 0.0f;
            if (e < C::NX) {
                const int ci = ci0 + e / (C::RH * C::RW), rem = e % (C::RH * C::RW);
                int iy = y0 + rem / C::RW - pad, ix = x0 + rem % C::RW - pad;
                bool ok = ci < Cin && iy >= -pad && iy < H + pad && ix >= -pad && ix < W + pad;
                if (pad_mode == VFI_PAD_REFLECT) {
                    iy = iy < 0 ? -iy : (iy >= H ? 2 * (H - 1) - iy : iy);
                    ix = ix < 0 ? -ix : (ix >= W ? 2 * (W - 1) - ix : ix);
                } else {
                    ok = ok && iy >= 0 && iy < H && ix >= 0 && ix < W;
                }
                if (ok) v = xn[(size_t)ci * HW + (size_t)iy * W + ix];
            }
            rx[r] = v;
        }
        const float *dn = dy + (size_t)n * dy_bs;
#pragma unroll
        for (int r = 0; r < C::RY; ++r) {
            const int e = tid + r * kThreads, k = e % C::P, co = co0 + e / C::P;
            const int yy = y0 + k / kWgTX, xx = x0 + k % kWgTX;
            ry[r] = (co < Cout && yy < H && xx < W) ? dn[(size_t)co * HW + (size_t)yy * W + xx] : 0.0f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < C::RX; ++r) {
            const int e = tid + r * kThreads;
            if (e < C::NX) sX[e] = rx[r];
        }
#pragma unroll
        for (int r = 0; r < C::RY; ++r) {
            const int e = tid + r * kThreads;
            sY[(e % C::P) * kYStride + e / C::P] = ry[r];
        }
    };

    f32x16 acc = {};
    float bacc = 0.0f;
    if (t_begin < t_end) load(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        stage();
        __syncthreads();
        if (t + 1 < t_end) load(t + 1);
#pragma unroll
        for (int s = 0; s < C::P / 2; ++s) {
            const float a = sYb[2 * s * kYStride];
            const float b = sXb[(2 * s / kWgTX) * C::RW + (2 * s) % kWgTX];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        if (do_bias) {  // 8 parts x 32 channels, each part sums its P/8 pixels in order
            const int part = tid >> 5;
#pragma unroll
            for (int k = 0; k < C::P / 8; ++k) bacc += sY[(part * (C::P / 8) + k) * kYStride + (tid & 31)];
        }
        __syncthreads();
    }
    const size_t slab = (size_t)Cout * Ncols;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (co < Cout && j < Ncols) part_w[(size_t)split * slab + (size_t)co * Ncols + j] = acc[r];
    }
    if (do_bias) {
        sB[tid] = bacc;
        __syncthreads();
        if (tid < 32 && co0 + tid < Cout) {
            float b = sB[tid];
            for (int p = 1; p < 8; ++p) b += sB[p * 32 + tid];
            part_b[(size_t)split * Cout + co0 + tid] = b;
        }
    }
}

// out[i] = sum over slabs s = 0, 1, ... of part[s][i] (fixed order: bitwise reproducible).  The loads of 8 slabs are
// issued before their adds: a layer with few outputs (the 32 -> 3 head) has one wave here, bound by load latency.
__global__ void slab_reduce_kernel(const float *__restrict__ part, int S, long long count, float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x) {
        float v = part[i];
        int s = 1;
        for (; s + 8 <= S; s += 8) {
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = part[(size_t)(s + k) * count + i];
#pragma unroll
            for (int k = 0; k < 8; ++k) v += t[k];
        }
        for (; s < S; ++s) v += part[(size_t)s * count + i];
        out[i] = v;
    }
}

struct WgradPlan {
    int tiles_x, tiles_y, tiles_total, col_blocks, co_blocks, splits, tiles_per_split;
};

// Split count from the shape alone (never from the device), so the summation order -- and the bits -- are the same on
// every device; capped by the workspace the caller gives.
WgradPlan wgrad_plan(int N, int Cin, int H, int W, int Cout, int KS, long long workspace_floats) {
    WgradPlan p;
    const int TY = KS == 1 ? 1 : 4;
    p.tiles_x = ceil_div(W, kWgTX);
    p.tiles_y = ceil_div(H, TY);
    p.tiles_total = N * p.tiles_x * p.tiles_y;
    p.col_blocks = ceil_div(Cin * KS * KS, kWgCols);
    p.co_blocks = ceil_div(Cout, 32);
    const long long per_split = (long long)Cout * (Cin * KS * KS + 1);
    long long s = ceil_div(1024, p.col_blocks * p.co_blocks);  // about four 4-wave workgroups per CU ...
    s = s < 256 ? s : 256;                                     // ... but a short reduction for the narrow layers
    s = s < p.tiles_total ? s : p.tiles_total;
    const long long fit = workspace_floats / per_split;
    s = s < fit ? s : fit;
    if (s < 1) s = 1;
    p.tiles_per_split = ceil_div(p.tiles_total, (int)s);
    p.splits = ceil_div(p.tiles_total, p.tiles_per_split);
    return p;
}

// ---- input gradient helpers -----------------------------------------------------------------------------------------
// e[n][c] (H+2p, W+2p) = dY[n][c] placed at offset (p, p), zero ring
__global__ void embed_kernel(const float *__restrict__ dy, long long dy_bs, float *__restrict__ e, int N, int C, int H,
                             int W, int p) {
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    const long long total = (long long)N * C * Hp * Wp;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int v = i % Wp, u = (i / Wp) % Hp;
        const long long nc = i / ((long long)Wp * Hp);
        const int c = nc % C, n = nc / C;
        const int y = u - p, xx = v - p;
        e[i] = (y >= 0 && y < H && xx >= 0 && xx < W) ? dy[(size_t)n * dy_bs + ((size_t)c * H + y) * W + xx] : 0.0f;
    }
}

// padded rows of the reflect-padded axis that read source index y: the interior one, the top mirror (y in [1, p]) and
// the bottom mirror (y in [n-1-p, n-2]); returns their count
__device__ __forceinline__ int reflect_sources(int y, int n, int p, int *u) {
    int k = 0;
    u[k++] = y + p;
    if (y >= 1 && y <= p) u[k++] = p - y;
    if (y <= n - 2 && y >= n - 1 - p) u[k++] = 2 * (n - 1) - y + p;
    return k;
}

// dX[n][c][y][x] = sum of the full-extent gradient d (N, C, H+2p, W+2p) over every padded position that reads (y, x)
// under reflect padding (torch's ReflectionPad2d backward), in a fixed order
__global__ void reflect_fold_kernel(const float *__restrict__ d, float *__restrict__ dx, long long dx_bs, int N, int C,
                                    int H, int W, int p) {
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    const long long total = (long long)N * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int xx = i % W, y = (i / W) % H;
        const long long nc = i / ((long long)W * H);
        const int c = nc % C, n = nc / C;
        int us[3], vs[3];
        const int ku = reflect_sources(y, H, p, us), kv = reflect_sources(xx, W, p, vs);
        const float *dp = d + (size_t)nc * Hp * Wp;
        float v = 0.0f;
        for (int a = 0; a < ku; ++a)
            for (int b = 0; b < kv; ++b) v += dp[(size_t)us[a] * Wp + vs[b]];
        dx[(size_t)n * dx_bs + ((size_t)c * H + y) * W + xx] = v;
    }
}

// ---- glue adjoints ----------------------------------------------------------------------------------------------
// y = clamp(base + tanh(x), 0, 1): m = [0 <= base + tanh x <= 1] (both ends inclusive, torch.clamp's backward),
// g_x = g (1 - tanh^2 x) m, g_base = g m
__global__ void tanh_residual_clamp_backward_kernel(const float *__restrict__ x, const float *__restrict__ base,
                                                    const float *__restrict__ g, float *__restrict__ gx,
                                                    float *__restrict__ gb, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float t = tanhf(x[i]);
        const float v = base[i] + t;
        const bool m = v >= 0.0f && v <= 1.0f;
        const float gi = g[i];
        if (gx) gx[i] = m ? gi * (1.0f - t * t) : 0.0f;
        if (gb) gb[i] = m ? gi : 0.0f;
    }
}

// Encoder block: s = relu(z) feeds MaxPool2d(2) and the decoder skip.  g_s = (g_pooled routed to the first maximal
// element of its 2x2 window in row-major order, as torch's max_pool2d) + g_skip, times [s > 0].  One thread per window.
__global__ void pool2_max_backward_kernel(const float *__restrict__ s, long long s_bs, const float *__restrict__ gp,
                                          long long gp_bs, const float *__restrict__ gk, long long gk_bs,
                                          float *__restrict__ gs, long long gs_bs, int N, int C, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * C * Ho * Wo;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int xo = i % Wo, yo = (i / Wo) % Ho, c = (i / ((long long)Wo * Ho)) % C, n = i / ((long long)Wo * Ho * C);
        const size_t o[4] = {((size_t)c * H + 2 * yo) * W + 2 * xo, ((size_t)c * H + 2 * yo) * W + 2 * xo + 1,
                             ((size_t)c * H + 2 * yo + 1) * W + 2 * xo, ((size_t)c * H + 2 * yo + 1) * W + 2 * xo + 1};
        const float *sn = s + (size_t)n * s_bs;
        float v[4];
        int arg = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = sn[o[k]];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (v[k] > v[arg] || isnan(v[k])) arg = k;
        const float g = gp[(size_t)n * gp_bs + ((size_t)c * Ho + yo) * Wo + xo];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float r = k == arg ? g : 0.0f;
            if (gk) r += gk[(size_t)n * gk_bs + o[k]];
            gs[(size_t)n * gs_bs + o[k]] = v[k] > 0.0f ? r : 0.0f;
        }
    }
}

// Tap rule of vfi_resize_bilinear(x2, align_corners=0) for up2_backward_kernel: the output positions of one axis (source
// coordinate max(o/2 - 1/4, 0)) that read source index j of n, with their weights: o = 2j-1 (1/4), 2j (3/4; 1 at j = 0),
// 2j+1 (3/4; 1 at j = n-1, where both taps clamp onto j), 2j+2 (1/4).
// The any-size adjoint (resize_adjoint_kernel, vfi_phasenet_grad.hip) gives the same bits for an exact x2 (tested), but it
// re-derives candidates and weights per output: vfi_resize_bilinear_backward routed through it took 1.81 - 1.93 x as long
// per call at FusionNet's decoder shapes (batch 16: 128 x 32^2, 64 x 64^2, 32 x 128^2) and the glue row of
// tools/fusionnet_train_rate.py 1.36 x (0.507 against 0.374 ms, MI355X).  So the fixed taps stay for x2.
__device__ __forceinline__ int up2_sources(int j, int n, int *o, float *w) {
    int k = 0;
    if (j >= 1) { o[k] = 2 * j - 1; w[k++] = 0.25f; }
    o[k] = 2 * j; w[k++] = j == 0 ? 1.0f : 0.75f;
    o[k] = 2 * j + 1; w[k++] = j == n - 1 ? 1.0f : 0.75f;
    if (j + 1 <= n - 1) { o[k] = 2 * j + 2; w[k++] = 0.25f; }
    return k;
}

}  // namespace

extern "C" long long vfi_conv2d_backward_weight_workspace_floats(int Cout, int Cin, int KS) {
    if (Cout <= 0 || Cin <= 0 || (KS != 1 && KS != 3 && KS != 5)) return -1;
    return (long long)Cout * (Cin * KS * KS + 1);
}

extern "C" int vfi_conv2d_backward_weight_splits(int N, int Cin, int H, int W, int Cout, int KS, long long workspace_floats) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (KS != 1 && KS != 3 && KS != 5)) return -1;
    return wgrad_plan(N, Cin, H, W, Cout, KS, workspace_floats).splits;
}

extern "C" int vfi_conv2d_backward_weight(const float *x, long long x_bstride, const float *dy, long long dy_bstride,
                                          float *dw, float *dbias, int N, int Cin, int H, int W, int Cout, int KS,
                                          int pad_mode, float *workspace, long long workspace_floats, vfi_stream_t stream) {
    VFI_REQUIRE(x && dy && dw && workspace, VFI_ERR_INVALID_ARG, "vfi_conv2d_backward_weight: null pointer");
    VFI_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, VFI_ERR_INVALID_ARG,
                "vfi_conv2d_backward_weight: non-positive size");
    VFI_REQUIRE(KS == 1 || KS == 3 || KS == 5, VFI_ERR_UNSUPPORTED, "vfi_conv2d_backward_weight: kernel size %d", KS);
    VFI_REQUIRE(pad_mode == VFI_PAD_ZERO || pad_mode == VFI_PAD_REFLECT, VFI_ERR_INVALID_ARG,
                "vfi_conv2d_backward_weight: pad_mode %d", pad_mode);
    VFI_REQUIRE(pad_mode == VFI_PAD_ZERO || ((KS - 1) / 2 < H && (KS - 1) / 2 < W), VFI_ERR_SHAPE,
                "vfi_conv2d_backward_weight: reflect padding %d needs a larger input than %dx%d", (KS - 1) / 2, H, W);
    VFI_REQUIRE((long long)Cin * H * W < (1ll << 31) && (long long)Cout * H * W < (1ll << 31) &&
                    (long long)N * ceil_div(H, 4) * ceil_div(W, kWgTX) * 4 < (1ll << 31),
                VFI_ERR_UNSUPPORTED, "vfi_conv2d_backward_weight: tensor too large for 32-bit offsets");
    const long long per_split = vfi_conv2d_backward_weight_workspace_floats(Cout, Cin, KS);
    VFI_REQUIRE(workspace_floats >= per_split, VFI_ERR_INVALID_ARG,
                "vfi_conv2d_backward_weight: workspace of %lld floats, needs at least %lld", workspace_floats, per_split);
    const WgradPlan p = wgrad_plan(N, Cin, H, W, Cout, KS, workspace_floats);
    const long long wcount = (long long)Cout * Cin * KS * KS;
    float *part_w = workspace, *part_b = dbias ? workspace + (size_t)p.splits * wcount : nullptr;
    hipStream_t s = vfi::as_stream(stream);
    const dim3 grid(p.col_blocks, p.co_blocks, p.splits);
#define WGRAD_ARGS x, x_bstride, dy, dy_bstride, part_w, part_b, Cin, H, W, Cout, pad_mode, p.tiles_x, p.tiles_y, \
                   p.tiles_total, p.tiles_per_split
    if (KS == 1) hipLaunchKernelGGL(conv_wgrad_kernel<1>, grid, dim3(kThreads), 0, s, WGRAD_ARGS);
    else if (KS == 3) hipLaunchKernelGGL(conv_wgrad_kernel<3>, grid, dim3(kThreads), 0, s, WGRAD_ARGS);
    else hipLaunchKernelGGL(conv_wgrad_kernel<5>, grid, dim3(kThreads), 0, s, WGRAD_ARGS);
#undef WGRAD_ARGS
    int rc = vfi::check_launch("vfi_conv2d_backward_weight");
    if (rc != VFI_OK) return rc;
    LAUNCH_1D(slab_reduce_kernel, wcount, stream, part_w, p.splits, wcount, dw);
    if (dbias) LAUNCH_1D(slab_reduce_kernel, (long long)Cout, stream, part_b, p.splits, (long long)Cout, dbias);
    return vfi::check_launch("vfi_conv2d_backward_weight (reduce)");
}

extern "C" long long vfi_conv2d_backward_data_workspace_floats(int N, int Cin, int H, int W, int Cout, int KS,
                                                               int pad_mode) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (KS != 1 && KS != 3 && KS != 5)) return -1;
    const int p = (KS - 1) / 2;
    if (pad_mode != VFI_PAD_REFLECT || p == 0) return 0;
    return (long long)N * (Cin + Cout) * (H + 2 * p) * (W + 2 * p);
}

extern "C" int vfi_conv2d_backward_data(const float *dy, long long dy_bstride, const float *packed_wt, float *dx,
                                        long long dx_bstride, int N, int Cin, int H, int W, int Cout, int KS, int pad_mode,
                                        float *workspace, long long workspace_floats, vfi_stream_t stream) {
    VFI_REQUIRE(dy && packed_wt && dx, VFI_ERR_INVALID_ARG, "vfi_conv2d_backward_data: null pointer");
    VFI_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, VFI_ERR_INVALID_ARG,
                "vfi_conv2d_backward_data: non-positive size");
    VFI_REQUIRE(KS == 1 || KS == 3 || KS == 5, VFI_ERR_UNSUPPORTED, "vfi_conv2d_backward_data: kernel size %d", KS);
    VFI_REQUIRE(pad_mode == VFI_PAD_ZERO || pad_mode == VFI_PAD_REFLECT, VFI_ERR_INVALID_ARG,
                "vfi_conv2d_backward_data: pad_mode %d", pad_mode);
    const int p = (KS - 1) / 2;
    VFI_REQUIRE(pad_mode == VFI_PAD_ZERO || (p < H && p < W), VFI_ERR_SHAPE,
                "vfi_conv2d_backward_data: reflect padding %d needs a larger input than %dx%d", p, H, W);
    if (workspace_floats <= 0) workspace = nullptr;
    // zero padding (and 1x1): dX = conv(dY, W^T flipped) with the same zero padding -- the forward kernels as they are
    if (pad_mode == VFI_PAD_ZERO || p == 0)
        return vfi_conv2d(dy, dy_bstride, packed_wt, nullptr, nullptr, 0, dx, dx_bstride, N, Cout, H, W, Cin, KS,
                          VFI_PAD_ZERO, VFI_ACT_NONE, workspace, workspace ? workspace_floats : 0, stream);
    const long long need = vfi_conv2d_backward_data_workspace_floats(N, Cin, H, W, Cout, KS, pad_mode);
    VFI_REQUIRE(workspace && workspace_floats >= need, VFI_ERR_INVALID_ARG,
                "vfi_conv2d_backward_data: workspace of %lld floats, needs at least %lld", workspace_floats, need);
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    VFI_REQUIRE((long long)(Cin > Cout ? Cin : Cout) * Hp * Wp < (1ll << 31), VFI_ERR_UNSUPPORTED,
                "vfi_conv2d_backward_data: per-sample tensor too large for 32-bit offsets");
    // reflect: the full-extent gradient of the padded input is conv(zero-embedded dY, W^T flipped) over (H+2p) x (W+2p)
    // with zero padding; each pad row / column's gradient then folds onto the interior pixel it mirrors
    float *e = workspace, *d = workspace + (size_t)N * Cout * Hp * Wp, *rest = workspace + need;
    const long long rest_floats = workspace_floats - need;
    LAUNCH_1D(embed_kernel, (long long)N * Cout * Hp * Wp, stream, dy, dy_bstride, e, N, Cout, H, W, p);
    int rc = vfi::check_launch("vfi_conv2d_backward_data (embed)");
    if (rc != VFI_OK) return rc;
    rc = vfi_conv2d(e, (long long)Cout * Hp * Wp, packed_wt, nullptr, nullptr, 0, d, (long long)Cin * Hp * Wp, N, Cout, Hp,
                    Wp, Cin, KS, VFI_PAD_ZERO, VFI_ACT_NONE, rest_floats > 0 ? rest : nullptr, rest_floats > 0 ? rest_floats : 0,
                    stream);
    if (rc != VFI_OK) return rc;
    LAUNCH_1D(reflect_fold_kernel, (long long)N * Cin * H * W, stream, d, dx, dx_bstride, N, Cin, H, W, p);
    return vfi::check_launch("vfi_conv2d_backward_data (fold)");
}

extern "C" int vfi_tanh_residual_clamp_backward(const float *x, const float *base, const float *grad_y, float *grad_x,
                                                float *grad_base, long long count, vfi_stream_t stream) {
    VFI_REQUIRE(x && base && grad_y && (grad_x || grad_base), VFI_ERR_INVALID_ARG,
                "vfi_tanh_residual_clamp_backward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_tanh_residual_clamp_backward: bad size");
    LAUNCH_1D(tanh_residual_clamp_backward_kernel, count, stream, x, base, grad_y, grad_x, grad_base, count);
    return vfi::check_launch("vfi_tanh_residual_clamp_backward");
}

extern "C" int vfi_pool2_max_backward(const float *y, long long y_bstride, const float *grad_pooled, long long gp_bstride,
                                      const float *grad_skip, long long gs_bstride, float *grad_y, long long gy_bstride,
                                      int N, int C, int H, int W, vfi_stream_t stream) {
    VFI_REQUIRE(y && grad_pooled && grad_y, VFI_ERR_INVALID_ARG, "vfi_pool2_max_backward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && H >= 2 && W >= 2, VFI_ERR_INVALID_ARG, "vfi_pool2_max_backward: bad sizes");
    VFI_REQUIRE(H % 2 == 0 && W % 2 == 0, VFI_ERR_UNSUPPORTED, "vfi_pool2_max_backward: odd size %dx%d", H, W);
    LAUNCH_1D(pool2_max_backward_kernel, (long long)N * C * (H / 2) * (W / 2), stream, y, y_bstride, grad_pooled, gp_bstride,
              grad_skip, gs_bstride, grad_y, gy_bstride, N, C, H, W);
    return vfi::check_launch("vfi_pool2_max_backward");
}

extern "C" int vfi_resize_bilinear_backward(const float *x, long long x_bstride, const float *grad_y, long long gy_bstride,
                                            float *grad_x, long long gx_bstride, int N, int C, int Hin, int Win, int Hout,
                                            int Wout, int relu_input, vfi_stream_t stream) {
    VFI_REQUIRE(grad_y && grad_x && (x || !relu_input), VFI_ERR_INVALID_ARG, "vfi_resize_bilinear_backward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && Hin > 0 && Win > 0, VFI_ERR_INVALID_ARG, "vfi_resize_bilinear_backward: bad sizes");
    VFI_REQUIRE(Hout == 2 * Hin && Wout == 2 * Win, VFI_ERR_UNSUPPORTED,
                "vfi_resize_bilinear_backward: only x2 (got %dx%d -> %dx%d)", Hin, Win, Hout, Wout);
    LAUNCH_1D((up2_backward_kernel<4, up2_sources>), (long long)N * C * Hin * Win, stream, grad_y, gy_bstride, relu_input ? x : nullptr,
              x_bstride, grad_x, gx_bstride, N, C, Hin, Win);
    return vfi::check_launch("vfi_resize_bilinear_backward");
}
