// Backward of the plain AdaCoF network (gfx950): the HBM-bound glue between the existing convolution gradients
// (vfi_conv_grad.hip) and the existing sampler gradient (vfi_adacof.hip).  Differentiates reference
// src/adacof/models/adacofnet.py:13-153 (KernelEstimation: ReLU, AvgPool2d(2), Upsample(x2, bilinear, align_corners=True),
// additive skips, softmax / sigmoid heads) and :191-217 (blend, smoothness terms), and src/adacof/utility.py:67-77
// (Charbonnier).  The rules: vfi_grad_common.h.
#include "vfi_grad_common.h"

namespace {

// ---- elementwise glue ---------------------------------------------------------------------------------------------
// Functors of map_kernel (vfi_grad_common.h).
// a + b (the U-Net's additive skip, adacofnet.py:128-146, kept apart from relu(conv) in the training forward)
struct Add {
    __device__ __forceinline__ float operator()(float a, float b, float, bool) const { return a + b; }
};
// (g + add) * [y > 0] (y: the ReLU's output; y == 0 passes nothing, as torch's threshold backward)
struct ReluMask {
    __device__ __forceinline__ float operator()(float g, float y, float add, bool has_add) const {
        const float v = has_add ? g + add : g;
        return y > 0.0f ? v : 0.0f;
    }
};

// dst (N, C, H + 2p, W + 2p) = ReplicationPad2d(p) of src (N, C, H, W) (adacofnet.py:166,193-194)
__global__ void replicate_pad_kernel(const float *__restrict__ src, long long s_bs, float *__restrict__ dst, int N, int C,
                                     int H, int W, int p) {
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    GRID_STRIDE(i, (long long)N * C * Hp * Wp) {
        const int x = i % Wp, y = (i / Wp) % Hp, c = (i / ((long long)Wp * Hp)) % C, n = i / ((long long)Wp * Hp * C);
        const int sy = min(max(y - p, 0), H - 1), sx = min(max(x - p, 0), W - 1);
        dst[i] = src[(size_t)n * s_bs + ((size_t)c * H + sy) * W + sx];
    }
}

// Encoder block (adacofnet.py:112-125): y = relu(z) feeds AvgPool2d(2) and (levels 2..5) the decoder skip.
// g_z = (0.25 * g_pooled over its 2x2 window + g_skip) * [y > 0].  One thread per VW horizontally adjacent windows;
// VW = 2 moves 16 bytes per row access.
template <int VW>
__global__ void pool2_avg_backward_kernel(const float *__restrict__ y, long long y_bs, const float *__restrict__ gp,
                                          long long gp_bs, const float *__restrict__ gk, long long gk_bs,
                                          float *__restrict__ gy, long long gy_bs, int N, int C, int H, int W) {
    const int Ho = H / 2, Wo = W / 2, Wq = Wo / VW;
    GRID_STRIDE(i, (long long)N * C * Ho * Wq) {
        const int xq = i % Wq, yo = (i / Wq) % Ho, c = (i / ((long long)Wq * Ho)) % C, n = i / ((long long)Wq * Ho * C);
        const size_t po = ((size_t)c * Ho + yo) * Wo + (size_t)xq * VW;
        float g[VW];
        if (VW == 2) {
            const float2 t = *reinterpret_cast<const float2 *>(gp + (size_t)n * gp_bs + po);
            g[0] = 0.25f * t.x; g[VW - 1] = 0.25f * t.y;
        } else {
            g[0] = 0.25f * gp[(size_t)n * gp_bs + po];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t o = ((size_t)c * H + 2 * yo + r) * W + (size_t)xq * 2 * VW;
            float yv[2 * VW], kv[2 * VW], ov[2 * VW];
            if (VW == 2) {
                *reinterpret_cast<float4 *>(yv) = *reinterpret_cast<const float4 *>(y + (size_t)n * y_bs + o);
                if (gk) *reinterpret_cast<float4 *>(kv) = *reinterpret_cast<const float4 *>(gk + (size_t)n * gk_bs + o);
            } else {
                *reinterpret_cast<float2 *>(yv) = *reinterpret_cast<const float2 *>(y + (size_t)n * y_bs + o);
                if (gk) *reinterpret_cast<float2 *>(kv) = *reinterpret_cast<const float2 *>(gk + (size_t)n * gk_bs + o);
            }
#pragma unroll
            for (int k = 0; k < 2 * VW; ++k) {
                const float v = g[k / 2] + (gk ? kv[k] : 0.0f);
                ov[k] = yv[k] > 0.0f ? v : 0.0f;
            }
            if (VW == 2) *reinterpret_cast<float4 *>(gy + (size_t)n * gy_bs + o) = *reinterpret_cast<float4 *>(ov);
            else *reinterpret_cast<float2 *>(gy + (size_t)n * gy_bs + o) = *reinterpret_cast<float2 *>(ov);
        }
    }
}

// Tap rule of Upsample(x2, bilinear, align_corners=True) (adacofnet.py:30,42,54,68,76,88) for up2_backward_kernel: the
// outputs of one axis that read source j of n, with their weights.  Output o sits at o (n-1)/(2n-1): the cell i0 and the
// fraction come from the integer quotient and remainder, so a weight carries one rounding whatever n is (the forward
// kernel's float product o * scale is off by up to 2^-23 (n-1) instead; the two agree to that).  At most 5 outputs have a
// non-zero weight (n = 1: both outputs, weight 1).
constexpr int kUpMax = 6;
__device__ __forceinline__ int up2ac_sources(int j, int n, int *o, float *w) {
    const int no = 2 * n, den = no - 1;
    if (n == 1) { o[0] = 0; o[1] = 1; w[0] = w[1] = 1.0f; return 2; }
    // outputs whose coordinate lies in (j-1, j+1)
    const int lo = max((int)(((long long)(j - 1) * den) / (n - 1)), 0);
    const int hi = min((int)(((long long)(j + 1) * den) / (n - 1)), no - 1);
    const float inv = 1.0f / (float)den;
    int k = 0;
    for (int q = lo; q <= hi; ++q) {
        const long long num = (long long)q * (n - 1);
        const int i0 = (int)(num / den), i1 = min(i0 + 1, n - 1);
        const float l = (float)(int)(num - (long long)i0 * den) * inv;
        float wt = 0.0f;
        if (i0 == j) wt += 1.0f - l;
        if (i1 == j) wt += l;
        if (wt != 0.0f && k < kUpMax) { o[k] = q; w[k++] = wt; }
    }
    return k;
}

// ---- smoothness terms and heads -----------------------------------------------------------------------------------
// Derivative of  mean_h sqrt((m[x]-m[x+1])^2 + e^2) + mean_v sqrt((m[y]-m[y+1])^2 + e^2)  (adacofnet.py:209-213) with
// respect to m[y][x] of one (H, W) plane: the <= 4 neighbour terms +- d / sqrt(d^2 + e^2), each over its direction's count.
__device__ __forceinline__ float charb_dir(float d, float eps2) { return d * rsqrtf(d * d + eps2); }
__device__ __forceinline__ float charb_stencil(const float *__restrict__ m, int y, int x, int H, int W, float inv_h,
                                               float inv_v, float eps2) {
    const float c = m[(size_t)y * W + x];
    float qh = 0.0f, qv = 0.0f;
    if (x + 1 < W) qh += charb_dir(c - m[(size_t)y * W + x + 1], eps2);
    if (x >= 1) qh -= charb_dir(m[(size_t)y * W + x - 1] - c, eps2);
    if (y + 1 < H) qv += charb_dir(c - m[(size_t)(y + 1) * W + x], eps2);
    if (y >= 1) qv -= charb_dir(m[(size_t)(y - 1) * W + x] - c, eps2);
    return qh * inv_h + qv * inv_v;
}

// m[n][0..3] = (mean_k W1 A1, mean_k W1 B1, mean_k W2 A2, mean_k W2 B2) (adacofnet.py:204-207); blockIdx.y = side
__global__ void smooth_maps_kernel(const float *__restrict__ w1, const float *__restrict__ a1, const float *__restrict__ b1,
                                   const float *__restrict__ w2, const float *__restrict__ a2, const float *__restrict__ b2,
                                   float *__restrict__ m, int N, int F2, long long HW) {
    const float *w = blockIdx.y ? w2 : w1, *a = blockIdx.y ? a2 : a1, *b = blockIdx.y ? b2 : b1;
    const float inv = 1.0f / (float)F2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)N * HW; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / HW, p = i - n * HW;
        const size_t base = (size_t)n * F2 * HW + p;
        float sa = 0.0f, sb = 0.0f;
        for (int k = 0; k < F2; ++k) {
            const float wk = w[base + (size_t)k * HW];
            sa += wk * a[base + (size_t)k * HW];
            sb += wk * b[base + (size_t)k * HW];
        }
        m[((size_t)n * 4 + 2 * blockIdx.y) * HW + p] = sa * inv;
        m[((size_t)n * 4 + 2 * blockIdx.y + 1) * HW + p] = sb * inv;
    }
}

// stage 1: per block, the Charbonnier sums of the horizontal / vertical differences of the four m maps (v[0], v[1]) and
// of Occlusion (v[2], v[3]); each pixel owns its difference to the right and downwards
__global__ __launch_bounds__(kThreads) void smooth_partial_kernel(const float *__restrict__ m, const float *__restrict__ occ,
                                                                  float *__restrict__ part, int N, int H, int W, float eps2) {
    __shared__ float lds[4 * kThreads];
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const long long HW = (long long)H * W;
    GRID_STRIDE(i, (long long)N * HW) {
        const int x = i % W, y = (i / W) % H;
        const long long n = i / HW;
        const size_t p = (size_t)y * W + x;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float *pl = q < 4 ? m + ((size_t)n * 4 + q) * HW : occ + (size_t)n * HW;
            const float c = pl[p];
            const int o = q < 4 ? 0 : 2;
            if (x + 1 < W) { const float d = c - pl[p + 1]; v[o] += sqrtf(d * d + eps2); }
            if (y + 1 < H) { const float d = c - pl[p + W]; v[o + 1] += sqrtf(d * d + eps2); }
        }
    }
    block_sum<4>(v, lds);
    if (threadIdx.x == 0)
        for (int q = 0; q < 4; ++q) part[(size_t)q * kMaxPartials + blockIdx.x] = v[q];
}

// stage 2 (one block): out[0] = g_Spatial, out[1] = g_Occlusion
__global__ __launch_bounds__(kThreads) void smooth_final_kernel(const float *__restrict__ part, int blocks, float inv_h,
                                                                float inv_v, float *__restrict__ out) {
    __shared__ float lds[4 * kThreads];
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = threadIdx.x; b < blocks; b += kThreads)
        for (int q = 0; q < 4; ++q) v[q] += part[(size_t)q * kMaxPartials + b];
    block_sum<4>(v, lds);
    if (threadIdx.x == 0) {
        out[0] = v[0] * inv_h + v[1] * inv_v;
        out[1] = v[2] * inv_h + v[3] * inv_v;
    }
}

// Blend and occlusion head (adacofnet.py:196-200,213): frame1 = occ t1 + (1 - occ) t2, cropped to (h0, w0); g is zero in
// the crop's complement.  g_t1 = g occ, g_t2 = g (1 - occ), g_occ = sum_c g_c (t1_c - t2_c) + up_occ * stencil(occ),
// g_z = g_occ occ (1 - occ) (the sigmoid).  One thread per pixel of the padded extent.
__global__ void blend_backward_kernel(const float *__restrict__ g, const float *__restrict__ t1, const float *__restrict__ t2,
                                      const float *__restrict__ occ, const float *__restrict__ up_occ,
                                      float *__restrict__ g_t1, float *__restrict__ g_t2, float *__restrict__ g_z, int N, int C,
                                      int H, int W, int h0, int w0, float inv_h, float inv_v, float eps2) {
    const long long HW = (long long)H * W;
    const float up = up_occ ? up_occ[0] : 0.0f;
    GRID_STRIDE(i, (long long)N * HW) {
        const int x = i % W, y = (i / W) % H;
        const long long n = i / HW;
        const size_t p = (size_t)y * W + x;
        const float o = occ[(size_t)n * HW + p];
        const bool in = y < h0 && x < w0;
        float go = 0.0f;
        for (int c = 0; c < C; ++c) {
            const size_t e = ((size_t)n * C + c) * HW + p;
            const float gc = in ? g[(((size_t)n * C + c) * h0 + y) * w0 + x] : 0.0f;
            g_t1[e] = gc * o;
            g_t2[e] = gc * (1.0f - o);
            go += gc * (t1[e] - t2[e]);
        }
        if (up != 0.0f) go += up * charb_stencil(occ + (size_t)n * HW, y, x, H, W, inv_h, inv_v, eps2);
        g_z[(size_t)n * HW + p] = go * o * (1.0f - o);
    }
}

// One side's three head gradients from the sampler's (gw, ga, gb) and the smoothness terms (adacofnet.py:204-212,215):
// with q_A = up_sp * stencil(m_A), q_B likewise,  gW_k = gw_k + (q_A A_k + q_B B_k) / F^2,  then the softmax backward
// g_logit_k = W_k (gW_k - sum_j W_j gW_j),  g_alpha_k = ga_k + q_A W_k / F^2,  g_beta_k = gb_k + q_B W_k / F^2.
__global__ void head_backward_kernel(const float *__restrict__ gw, const float *__restrict__ ga, const float *__restrict__ gb,
                                     const float *__restrict__ w, const float *__restrict__ a, const float *__restrict__ b,
                                     const float *__restrict__ m_a, const float *__restrict__ m_b, long long m_bs,
                                     const float *__restrict__ up_sp, float *__restrict__ g_logit, float *__restrict__ g_alpha,
                                     float *__restrict__ g_beta, int N, int F2, int H, int W, float inv_h, float inv_v,
                                     float eps2) {
    const long long HW = (long long)H * W;
    const float up = up_sp ? up_sp[0] : 0.0f;
    const float inv = 1.0f / (float)F2;
    GRID_STRIDE(i, (long long)N * HW) {
        const int x = i % W, y = (i / W) % H;
        const long long n = i / HW;
        const size_t base = (size_t)n * F2 * HW + (size_t)y * W + x;
        float qa = 0.0f, qb = 0.0f;
        if (up != 0.0f) {
            qa = up * inv * charb_stencil(m_a + (size_t)n * m_bs, y, x, H, W, inv_h, inv_v, eps2);
            qb = up * inv * charb_stencil(m_b + (size_t)n * m_bs, y, x, H, W, inv_h, inv_v, eps2);
        }
        float dot = 0.0f;
        for (int k = 0; k < F2; ++k) {
            const size_t e = base + (size_t)k * HW;
            dot += w[e] * (gw[e] + (qa * a[e] + qb * b[e]));
        }
        for (int k = 0; k < F2; ++k) {
            const size_t e = base + (size_t)k * HW;
            const float wk = w[e];
            g_logit[e] = wk * ((gw[e] + (qa * a[e] + qb * b[e])) - dot);
            g_alpha[e] = ga[e] + qa * wk;
            g_beta[e] = gb[e] + qb * wk;
        }
    }
}

}  // namespace

extern "C" int vfi_add(const float *a, long long a_bstride, const float *b, long long b_bstride, float *out,
                       long long out_bstride, int N, long long count, vfi_stream_t stream) {
    VFI_REQUIRE(a && b && out, VFI_ERR_INVALID_ARG, "vfi_add: null pointer");
    VFI_REQUIRE(N > 0 && count > 0, VFI_ERR_INVALID_ARG, "vfi_add: bad sizes");
    launch_map<Add>(a, a_bstride, b, b_bstride, nullptr, 0, out, out_bstride, N, count, stream);
    return vfi::check_launch("vfi_add");
}

extern "C" int vfi_relu_mask(const float *grad, long long g_bstride, const float *addend, long long a_bstride, const float *y,
                             long long y_bstride, float *out, long long out_bstride, int N, long long count,
                             vfi_stream_t stream) {
    VFI_REQUIRE(grad && y && out, VFI_ERR_INVALID_ARG, "vfi_relu_mask: null pointer");
    VFI_REQUIRE(N > 0 && count > 0, VFI_ERR_INVALID_ARG, "vfi_relu_mask: bad sizes");
    launch_map<ReluMask>(grad, g_bstride, y, y_bstride, addend, a_bstride, out, out_bstride, N, count, stream);
    return vfi::check_launch("vfi_relu_mask");
}

extern "C" int vfi_sigmoid_backward(const float *grad, const float *s, float *grad_z, long long count, vfi_stream_t stream) {
    VFI_REQUIRE(grad && s && grad_z, VFI_ERR_INVALID_ARG, "vfi_sigmoid_backward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_sigmoid_backward: bad size");
    // the occlusion head (adacofnet.py:98-99), dense
    launch_map<ActGrad<VFI_ACT_SIGMOID>>(grad, count, s, count, nullptr, 0, grad_z, count, 1, count, stream);
    return vfi::check_launch("vfi_sigmoid_backward");
}

extern "C" int vfi_replicate_pad(const float *x, long long x_bstride, float *out, int N, int C, int H, int W, int pad,
                                 vfi_stream_t stream) {
    VFI_REQUIRE(x && out, VFI_ERR_INVALID_ARG, "vfi_replicate_pad: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && pad >= 0, VFI_ERR_INVALID_ARG, "vfi_replicate_pad: bad sizes");
    LAUNCH_1D(replicate_pad_kernel, (long long)N * C * (H + 2 * pad) * (W + 2 * pad), stream, x, x_bstride, out, N, C, H, W,
              pad);
    return vfi::check_launch("vfi_replicate_pad");
}

extern "C" int vfi_pool2_avg_backward(const float *y, long long y_bstride, const float *grad_pooled, long long gp_bstride,
                                      const float *grad_skip, long long gs_bstride, float *grad_y, long long gy_bstride,
                                      int N, int C, int H, int W, vfi_stream_t stream) {
    VFI_REQUIRE(y && grad_pooled && grad_y, VFI_ERR_INVALID_ARG, "vfi_pool2_avg_backward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && H >= 2 && W >= 2, VFI_ERR_INVALID_ARG, "vfi_pool2_avg_backward: bad sizes");
    VFI_REQUIRE(H % 2 == 0 && W % 2 == 0, VFI_ERR_UNSUPPORTED, "vfi_pool2_avg_backward: odd size %dx%d", H, W);
    VFI_REQUIRE(y_bstride % 2 == 0 && gs_bstride % 2 == 0 && gy_bstride % 2 == 0 && ((uintptr_t)y & 7) == 0 &&
                    ((uintptr_t)grad_skip & 7) == 0 && ((uintptr_t)grad_y & 7) == 0,
                VFI_ERR_UNSUPPORTED, "vfi_pool2_avg_backward: operands must be 8-byte aligned with even batch strides");
    const bool v4 = W % 4 == 0 && y_bstride % 4 == 0 && gs_bstride % 4 == 0 && gy_bstride % 4 == 0 && gp_bstride % 2 == 0 &&
                    aligned16(y) && aligned16(grad_skip) && aligned16(grad_y) && ((uintptr_t)grad_pooled & 7) == 0;
    if (v4)
        LAUNCH_1D(pool2_avg_backward_kernel<2>, (long long)N * C * (H / 2) * (W / 4), stream, y, y_bstride, grad_pooled,
                  gp_bstride, grad_skip, gs_bstride, grad_y, gy_bstride, N, C, H, W);
    else
        LAUNCH_1D(pool2_avg_backward_kernel<1>, (long long)N * C * (H / 2) * (W / 2), stream, y, y_bstride, grad_pooled,
                  gp_bstride, grad_skip, gs_bstride, grad_y, gy_bstride, N, C, H, W);
    return vfi::check_launch("vfi_pool2_avg_backward");
}

extern "C" int vfi_upsample2x_backward(const float *grad_y, long long gy_bstride, const float *mask_src, long long ms_bstride,
                                       float *grad_x, long long gx_bstride, int N, int C, int Hin, int Win,
                                       vfi_stream_t stream) {
    VFI_REQUIRE(grad_y && grad_x, VFI_ERR_INVALID_ARG, "vfi_upsample2x_backward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && Hin > 0 && Win > 0 && Hin < (1 << 20) && Win < (1 << 20), VFI_ERR_INVALID_ARG,
                "vfi_upsample2x_backward: bad sizes");
    LAUNCH_1D((up2_backward_kernel<kUpMax, up2ac_sources>), (long long)N * C * Hin * Win, stream, grad_y, gy_bstride, mask_src, ms_bstride,
              grad_x, gx_bstride, N, C, Hin, Win);
    return vfi::check_launch("vfi_upsample2x_backward");
}

namespace {
inline void charb_counts(int N, int H, int W, float *inv_h, float *inv_v) {
    // an empty direction (W = 1 or H = 1) has no term: its stencil is empty too, the factor is never used
    *inv_h = W > 1 ? (float)(1.0 / ((double)N * H * (W - 1))) : 0.0f;
    *inv_v = H > 1 ? (float)(1.0 / ((double)N * (H - 1) * W)) : 0.0f;
}
}  // namespace

extern "C" int vfi_adacof_smooth_forward(const float *w1, const float *a1, const float *b1, const float *w2, const float *a2,
                                         const float *b2, const float *occ, float *m, float *workspace, float *out, int N,
                                         int F, int H, int W, float epsilon, vfi_stream_t stream) {
    VFI_REQUIRE(w1 && a1 && b1 && w2 && a2 && b2 && occ && m && workspace && out, VFI_ERR_INVALID_ARG,
                "vfi_adacof_smooth_forward: null pointer");
    VFI_REQUIRE(N > 0 && F > 0 && H > 1 && W > 1, VFI_ERR_INVALID_ARG, "vfi_adacof_smooth_forward: bad sizes");
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(smooth_maps_kernel, dim3(vfi::blocks_1d((long long)N * HW), 2), dim3(kThreads), 0, vfi::as_stream(stream),
                       w1, a1, b1, w2, a2, b2, m, N, F * F, HW);
    int rc = vfi::check_launch("vfi_adacof_smooth_forward (maps)");
    if (rc != VFI_OK) return rc;
    float inv_h, inv_v;
    charb_counts(N, H, W, &inv_h, &inv_v);
    const int blocks = reduce_blocks((long long)N * HW);
    hipLaunchKernelGGL(smooth_partial_kernel, dim3(blocks), dim3(kThreads), 0, vfi::as_stream(stream), m, occ, workspace, N, H,
                       W, epsilon * epsilon);
    hipLaunchKernelGGL(smooth_final_kernel, dim3(1), dim3(kThreads), 0, vfi::as_stream(stream), workspace, blocks, inv_h, inv_v,
                       out);
    return vfi::check_launch("vfi_adacof_smooth_forward");
}

extern "C" int vfi_adacof_blend_backward(const float *grad_frame, const float *t1, const float *t2, const float *occ,
                                         const float *up_occ, float *grad_t1, float *grad_t2, float *grad_z, int N, int C,
                                         int H, int W, int h0, int w0, float epsilon, vfi_stream_t stream) {
    VFI_REQUIRE(grad_frame && t1 && t2 && occ && grad_t1 && grad_t2 && grad_z, VFI_ERR_INVALID_ARG,
                "vfi_adacof_blend_backward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && h0 > 0 && w0 > 0 && h0 <= H && w0 <= W, VFI_ERR_INVALID_ARG,
                "vfi_adacof_blend_backward: bad sizes");
    float inv_h, inv_v;
    charb_counts(N, H, W, &inv_h, &inv_v);
    LAUNCH_1D(blend_backward_kernel, (long long)N * H * W, stream, grad_frame, t1, t2, occ, up_occ, grad_t1, grad_t2, grad_z,
              N, C, H, W, h0, w0, inv_h, inv_v, epsilon * epsilon);
    return vfi::check_launch("vfi_adacof_blend_backward");
}

extern "C" int vfi_adacof_head_backward(const float *gw, const float *ga, const float *gb, const float *w, const float *a,
                                        const float *b, const float *m_a, const float *m_b, long long m_bstride,
                                        const float *up_spatial, float *grad_logit, float *grad_alpha, float *grad_beta,
                                        int N, int F, int H, int W, float epsilon, vfi_stream_t stream) {
    VFI_REQUIRE(gw && ga && gb && w && a && b && grad_logit && grad_alpha && grad_beta, VFI_ERR_INVALID_ARG,
                "vfi_adacof_head_backward: null pointer");
    VFI_REQUIRE(!up_spatial || (m_a && m_b), VFI_ERR_INVALID_ARG, "vfi_adacof_head_backward: smoothness maps missing");
    VFI_REQUIRE(N > 0 && F > 0 && H > 0 && W > 0, VFI_ERR_INVALID_ARG, "vfi_adacof_head_backward: bad sizes");
    float inv_h, inv_v;
    charb_counts(N, H, W, &inv_h, &inv_v);
    LAUNCH_1D(head_backward_kernel, (long long)N * H * W, stream, gw, ga, gb, w, a, b, m_a, m_b, m_bstride, up_spatial,
              grad_logit, grad_alpha, grad_beta, N, F * F, H, W, inv_h, inv_v, epsilon * epsilon);
    return vfi::check_launch("vfi_adacof_head_backward");
}

extern "C" int vfi_charbonnier_forward(const float *a, const float *b, long long count, float epsilon, float *workspace,
                                       float *out, vfi_stream_t stream) {
    VFI_REQUIRE(a && workspace && out, VFI_ERR_INVALID_ARG, "vfi_charbonnier_forward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_charbonnier_forward: bad size");
    // utility.py:67-77
    return launch_sum_forward(CharbonnierTerm{epsilon * epsilon}, a, b, count, (float)(1.0 / (double)count), workspace, out, stream,
                              "vfi_charbonnier_forward");
}

extern "C" int vfi_charbonnier_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b,
                                        long long count, float epsilon, vfi_stream_t stream) {
    VFI_REQUIRE(a && upstream && (grad_a || grad_b), VFI_ERR_INVALID_ARG, "vfi_charbonnier_backward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_charbonnier_backward: bad size");
    LAUNCH_1D(sum_backward_kernel<CharbonnierTerm>, count, stream, CharbonnierTerm{epsilon * epsilon}, a, b, upstream, grad_a,
              grad_b, count, (float)(1.0 / (double)count));
    return vfi::check_launch("vfi_charbonnier_backward");
}

extern "C" int vfi_mse_forward(const float *a, const float *b, long long count, float *workspace, float *out,
                               vfi_stream_t stream) {
    VFI_REQUIRE(a && b && workspace && out, VFI_ERR_INVALID_ARG, "vfi_mse_forward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_mse_forward: bad size");
    // nn.MSELoss (losses/__init__.py:17, losses/vgg.py:20)
    return launch_sum_forward(SquareTerm{}, a, b, count, (float)(1.0 / (double)count), workspace, out, stream, "vfi_mse_forward");
}

extern "C" int vfi_mse_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b,
                                long long count, vfi_stream_t stream) {
    VFI_REQUIRE(a && b && upstream && (grad_a || grad_b), VFI_ERR_INVALID_ARG, "vfi_mse_backward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_mse_backward: bad size");
    LAUNCH_1D(sum_backward_kernel<SquareTerm>, count, stream, SquareTerm{}, a, b, upstream, grad_a, grad_b, count,
              (float)(1.0 / (double)count));
    return vfi::check_launch("vfi_mse_backward");
}
