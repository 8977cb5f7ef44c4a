// Backward of one PhaseNet level (gfx950): the HBM-bound adjoints between the existing convolution gradients
// (vfi_conv_grad.hip).  Differentiates reference src/phase_net/phase_net.py:138-139 (bilinear resize to an arbitrary size),
// :190-200 (ELU, tanh), :113-116 and :155-168 with reverse_normalize :80-98 (the per-level blends), and
// src/train/loss.py:10-20 (phase loss, L1).  Rules of sections 12 and 13: no float atomics, one writer per element,
// reductions in an order fixed by the shape, fp32 throughout.
#include "vfi_common.h"

#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPartials = 1024;      // blocks of a two-stage reduction (VFI_REDUCE_WORKSPACE_FLOATS >= this)

inline int blocks_for(long long n) {
    long long b = (n + kThreads - 1) / kThreads;
    return (int)(b < 1 ? 1 : (b > 8 * 2048 ? 8 * 2048 : b));  // grid-stride beyond 16k blocks
}
// reduction grids depend on the element count alone, so the summation order -- and the bits -- repeat
inline int reduce_blocks(long long n) {
    long long b = (n + kThreads - 1) / kThreads;
    return (int)(b < 1 ? 1 : (b > kMaxPartials ? kMaxPartials : b));
}
__host__ __device__ inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

#define LAUNCH_1D(kernel, total, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3(blocks_for(total)), dim3(kThreads), 0, vfi::as_stream(stream), __VA_ARGS__)

#define GRID_STRIDE(i, total) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (long long)gridDim.x * blockDim.x)

// ---- adjoint of the arbitrary-size bilinear resize (align_corners = 0) ---------------------------------------------
// Weight with which output o of an axis resized n_in -> n_out reads source s: the forward's own fp32 arithmetic
// (resize_bilinear_kernel, vfi_aux.hip), so the adjoint cannot disagree with it about an index.  At the clamped edge
// i0 == i1 and both weights land on the same source.
__device__ __forceinline__ float resize_weight(int o, int s, float scale, int n_in) {
    const float f = fmaxf(scale * (o + 0.5f) - 0.5f, 0.0f);
    const int i0 = min((int)f, n_in - 1), i1 = min(i0 + 1, n_in - 1);
    const float l = f - (float)i0;
    float w = 0.0f;
    if (i0 == s) w += 1.0f - l;
    if (i1 == s) w += l;
    return w;
}
// Outputs that can read source s: those whose exact coordinate (o + 1/2) n_in / n_out - 1/2 lies in (s - 1, s + 1), from
// integer arithmetic, with one output of slack on each side (the fp32 coordinate is off by less than n_out 2^-22 outputs;
// the host bounds the sizes by 2^20).  The first and last source also own the outputs clamped onto them.
__device__ __forceinline__ void resize_candidates(int s, int n_in, int n_out, int *lo, int *hi) {
    // (o + 1/2) n_in / n_out - 1/2 > s - 1  <=>  o > ((2 s - 1) n_out - n_in) / (2 n_in)
    const long long a = (2ll * s - 1) * n_out - n_in, b = (2ll * s + 3) * n_out - n_in, d = 2ll * n_in;
    long long l = (a >= 0 ? a / d : -((-a + d - 1) / d)) - 1;      // floor, then the slack
    long long h = (b >= 0 ? (b + d - 1) / d : -((-b) / d)) + 1;    // ceil, then the slack
    if (s == 0) l = 0;
    if (s == n_in - 1) h = n_out - 1;
    *lo = (int)(l < 0 ? 0 : l);
    *hi = (int)(h > n_out - 1 ? n_out - 1 : h);
}

// Gather form: one thread per source element sums the gradients of the outputs that read it, rows outermost, both in
// ascending order; an output that does not hit the source has weight 0 and is skipped.  A source no output reads gets 0.
__global__ void resize_adjoint_kernel(const float *__restrict__ g, long long g_bs, float *__restrict__ gx, long long gx_bs,
                                      int N, int C, int Hi, int Wi, int Ho, int Wo) {
    const float sy = (float)Hi / (float)Ho, sx = (float)Wi / (float)Wo;
    GRID_STRIDE(i, (long long)N * C * Hi * Wi) {
        const int xj = i % Wi, yj = (i / Wi) % Hi, c = (i / ((long long)Wi * Hi)) % C, n = i / ((long long)Wi * Hi * C);
        int ylo, yhi, xlo, xhi;
        resize_candidates(yj, Hi, Ho, &ylo, &yhi);
        resize_candidates(xj, Wi, Wo, &xlo, &xhi);
        const float *gp = g + (size_t)n * g_bs + (size_t)c * Ho * Wo;
        float v = 0.0f;
        for (int yo = ylo; yo <= yhi; ++yo) {
            const float wy = resize_weight(yo, yj, sy, Hi);
            if (wy == 0.0f) continue;
            float r = 0.0f;
            for (int xo = xlo; xo <= xhi; ++xo) {
                const float wx = resize_weight(xo, xj, sx, Wi);
                if (wx != 0.0f) r += wx * gp[(size_t)yo * Wo + xo];
            }
            v += wy * r;
        }
        gx[(size_t)n * gx_bs + ((size_t)c * Hi + yj) * Wi + xj] = v;
    }
}

// ---- activation backward from the activation's output --------------------------------------------------------------
// ELU (alpha = 1): y > 0 ? 1 : y + 1 (for y <= 0, y = e^z - 1 and dy/dz = e^z);  tanh: 1 - y^2
template <int ACT> __device__ __forceinline__ float act_grad(float g, float y) {
    return ACT == VFI_ACT_ELU ? (y > 0.0f ? g : g * (y + 1.0f)) : g * (1.0f - y * y);
}
template <int ACT, typename T> __device__ __forceinline__ T act_grad_v(T g, T y);
template <> __device__ __forceinline__ float act_grad_v<VFI_ACT_ELU, float>(float g, float y) { return act_grad<VFI_ACT_ELU>(g, y); }
template <> __device__ __forceinline__ float act_grad_v<VFI_ACT_TANH, float>(float g, float y) { return act_grad<VFI_ACT_TANH>(g, y); }
template <> __device__ __forceinline__ float4 act_grad_v<VFI_ACT_ELU, float4>(float4 g, float4 y) {
    return make_float4(act_grad<VFI_ACT_ELU>(g.x, y.x), act_grad<VFI_ACT_ELU>(g.y, y.y), act_grad<VFI_ACT_ELU>(g.z, y.z),
                       act_grad<VFI_ACT_ELU>(g.w, y.w));
}
template <> __device__ __forceinline__ float4 act_grad_v<VFI_ACT_TANH, float4>(float4 g, float4 y) {
    return make_float4(act_grad<VFI_ACT_TANH>(g.x, y.x), act_grad<VFI_ACT_TANH>(g.y, y.y), act_grad<VFI_ACT_TANH>(g.z, y.z),
                       act_grad<VFI_ACT_TANH>(g.w, y.w));
}

// out = g * f'(y); out may be g itself.  T = float, or float4 (count and strides in units of T)
template <int ACT, typename T>
__global__ void act_backward_kernel(const T *g, long long g_bs, const T *__restrict__ y, long long y_bs, T *out,
                                    long long o_bs, int N, long long count) {
    GRID_STRIDE(i, (long long)N * count) {
        const long long n = i / count, e = i - n * count;
        out[n * o_bs + e] = act_grad_v<ACT, T>(g[n * g_bs + e], y[n * y_bs + e]);
    }
}

// ---- adjoints of the per-level blends (vfi_phasenet_emit, vfi_phasenet_emit_low) -----------------------------------
// phase = pi pred[:, 0:4];  amp = (b amp_in[:, 4:8] + (1 - b) amp_in[:, 0:4]) max[n], b = (pred[:, 4:8] + 1) / 2:
// g_pred[:, 0:4] = pi g_phase,  g_pred[:, 4:8] = g_amp max[n] (amp_in[:, 4:8] - amp_in[:, 0:4]) / 2.  A NULL gradient is zero.
__global__ void emit_backward_kernel(const float *__restrict__ g_phase, const float *__restrict__ g_amp,
                                     const float *__restrict__ amp_in, long long amp_bs, const float *__restrict__ maxv,
                                     float *__restrict__ g_pred, long long gp_bs, int N, int HW) {
    GRID_STRIDE(i, (long long)N * 4 * HW) {
        const int p = i % HW, b = (i / HW) % 4, n = i / ((long long)HW * 4);
        const float *am = amp_in + (size_t)n * amp_bs + p;
        float *gp = g_pred + (size_t)n * gp_bs + p;
        gp[(size_t)b * HW] = g_phase ? g_phase[i] * 3.14159265358979323846f : 0.0f;
        gp[(size_t)(4 + b) * HW] = g_amp ? g_amp[i] * maxv[n] * (am[(size_t)(4 + b) * HW] - am[(size_t)b * HW]) * 0.5f : 0.0f;
    }
}
// low = (a low_in[:, 0] + (1 - a) low_in[:, 1]) max[n], a = (pred + 1) / 2:  g_pred = g_low max[n] (low_in[:, 0] - low_in[:, 1]) / 2
__global__ void emit_low_backward_kernel(const float *__restrict__ g_low, const float *__restrict__ low, long long low_bs,
                                         const float *__restrict__ maxv, float *__restrict__ g_pred, long long gp_bs, int N,
                                         int HW) {
    GRID_STRIDE(i, (long long)N * HW) {
        const int p = i % HW, n = i / HW;
        const float *l = low + (size_t)n * low_bs + p;
        g_pred[(size_t)n * gp_bs + p] = g_low[i] * maxv[n] * (l[0] - l[HW]) * 0.5f;
    }
}

// ---- phase loss and L1 (loss.py:10-20) -----------------------------------------------------------------------------
// sums v over the block in a fixed tree order; the result is valid in thread 0
__device__ __forceinline__ float block_sum(float v, float *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}
// wrap(d) = atan2(sin d, cos d): d brought to (-pi, pi] (loss.py:15)
template <bool WRAP> __device__ __forceinline__ float wrapped(float d) { return WRAP ? atan2f(sinf(d), cosf(d)) : d; }

// stage 1: per block, sum |wrap(a - b)|; 16-byte loads when the count and both bases allow
template <bool WRAP>
__global__ __launch_bounds__(kThreads) void l1_partial_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                              long long count, int vec, float *__restrict__ part) {
    __shared__ float lds[kThreads];
    float v = 0.0f;
    if (vec) {
        const float4 *a4 = reinterpret_cast<const float4 *>(a), *b4 = reinterpret_cast<const float4 *>(b);
        GRID_STRIDE(i, count / 4) {
            const float4 p = a4[i], q = b4[i];
            v += (fabsf(wrapped<WRAP>(p.x - q.x)) + fabsf(wrapped<WRAP>(p.y - q.y))) +
                 (fabsf(wrapped<WRAP>(p.z - q.z)) + fabsf(wrapped<WRAP>(p.w - q.w)));
        }
    } else {
        GRID_STRIDE(i, count) v += fabsf(wrapped<WRAP>(a[i] - b[i]));
    }
    v = block_sum(v, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}
// stage 2 (one block): out[0] = factor * sum of the partials
__global__ __launch_bounds__(kThreads) void l1_final_kernel(const float *__restrict__ part, int blocks, float factor,
                                                            float *__restrict__ out) {
    __shared__ float lds[kThreads];
    float v = 0.0f;
    for (int b = threadIdx.x; b < blocks; b += kThreads) v += part[b];
    v = block_sum(v, lds);
    if (threadIdx.x == 0) out[0] = v * factor;
}
// g_a = sign(wrap(a - b)) * upstream * factor, g_b = -g_a
template <bool WRAP>
__global__ void l1_backward_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ up,
                                   float *__restrict__ ga, float *__restrict__ gb, long long count, float factor) {
    const float s = up[0] * factor;
    GRID_STRIDE(i, count) {
        const float d = wrapped<WRAP>(a[i] - b[i]);
        const float v = d > 0.0f ? s : (d < 0.0f ? -s : 0.0f);
        if (ga) ga[i] = v;
        if (gb) gb[i] = -v;
    }
}

template <int ACT>
void launch_act_backward(bool v4, const float *g, long long g_bs, const float *y, long long y_bs, float *out, long long o_bs,
                         int N, long long count, vfi_stream_t stream) {
    const auto k4 = act_backward_kernel<ACT, float4>;
    const auto k1 = act_backward_kernel<ACT, float>;
    if (v4)
        LAUNCH_1D(k4, (long long)N * count / 4, stream, reinterpret_cast<const float4 *>(g), g_bs / 4,
                  reinterpret_cast<const float4 *>(y), y_bs / 4, reinterpret_cast<float4 *>(out), o_bs / 4, N, count / 4);
    else
        LAUNCH_1D(k1, (long long)N * count, stream, g, g_bs, y, y_bs, out, o_bs, N, count);
}

}  // namespace

extern "C" int vfi_resize_bilinear_adjoint(const float *grad_y, long long gy_bstride, float *grad_x, long long gx_bstride,
                                           int N, int C, int Hin, int Win, int Hout, int Wout, vfi_stream_t stream) {
    VFI_REQUIRE(grad_y && grad_x, VFI_ERR_INVALID_ARG, "vfi_resize_bilinear_adjoint: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, VFI_ERR_INVALID_ARG,
                "vfi_resize_bilinear_adjoint: bad sizes");
    VFI_REQUIRE(Hin < (1 << 20) && Win < (1 << 20) && Hout < (1 << 20) && Wout < (1 << 20), VFI_ERR_UNSUPPORTED,
                "vfi_resize_bilinear_adjoint: sizes beyond 2^20 (%dx%d -> %dx%d)", Hin, Win, Hout, Wout);
    LAUNCH_1D(resize_adjoint_kernel, (long long)N * C * Hin * Win, stream, grad_y, gy_bstride, grad_x, gx_bstride, N, C, Hin,
              Win, Hout, Wout);
    return vfi::check_launch("vfi_resize_bilinear_adjoint");
}

extern "C" int vfi_act_backward(const float *grad, long long g_bstride, const float *y, long long y_bstride, float *out,
                                long long out_bstride, int N, long long count, int act, vfi_stream_t stream) {
    VFI_REQUIRE(grad && y && out, VFI_ERR_INVALID_ARG, "vfi_act_backward: null pointer");
    VFI_REQUIRE(N > 0 && count > 0, VFI_ERR_INVALID_ARG, "vfi_act_backward: bad sizes");
    VFI_REQUIRE(act == VFI_ACT_ELU || act == VFI_ACT_TANH, VFI_ERR_UNSUPPORTED, "vfi_act_backward: act %d (ELU and tanh only)", act);
    const bool v4 = count % 4 == 0 && g_bstride % 4 == 0 && y_bstride % 4 == 0 && out_bstride % 4 == 0 && aligned16(grad) &&
                    aligned16(y) && aligned16(out);
    if (act == VFI_ACT_ELU) launch_act_backward<VFI_ACT_ELU>(v4, grad, g_bstride, y, y_bstride, out, out_bstride, N, count, stream);
    else launch_act_backward<VFI_ACT_TANH>(v4, grad, g_bstride, y, y_bstride, out, out_bstride, N, count, stream);
    return vfi::check_launch("vfi_act_backward");
}

extern "C" int vfi_phasenet_emit_backward(const float *grad_phase, const float *grad_amp, const float *amp_in,
                                          long long amp_bstride, const float *max_amp, float *grad_pred,
                                          long long gp_bstride, int N, int HW, vfi_stream_t stream) {
    VFI_REQUIRE((grad_phase || grad_amp) && grad_pred, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_backward: null pointer");
    VFI_REQUIRE(!grad_amp || (amp_in && max_amp), VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_backward: amplitudes missing");
    VFI_REQUIRE(N > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_backward: bad sizes");
    LAUNCH_1D(emit_backward_kernel, (long long)N * 4 * HW, stream, grad_phase, grad_amp, amp_in, amp_bstride, max_amp,
              grad_pred, gp_bstride, N, HW);
    return vfi::check_launch("vfi_phasenet_emit_backward");
}

extern "C" int vfi_phasenet_emit_low_backward(const float *grad_low, const float *low_in, long long low_bstride,
                                              const float *max_low, float *grad_pred, long long gp_bstride, int N, int HW,
                                              vfi_stream_t stream) {
    VFI_REQUIRE(grad_low && low_in && max_low && grad_pred, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_low_backward: null pointer");
    VFI_REQUIRE(N > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_low_backward: bad sizes");
    LAUNCH_1D(emit_low_backward_kernel, (long long)N * HW, stream, grad_low, low_in, low_bstride, max_low, grad_pred,
              gp_bstride, N, HW);
    return vfi::check_launch("vfi_phasenet_emit_low_backward");
}

extern "C" int vfi_l1_forward(const float *a, const float *b, long long count, int wrap, float scale, float *workspace,
                              float *out, vfi_stream_t stream) {
    VFI_REQUIRE(a && b && workspace && out, VFI_ERR_INVALID_ARG, "vfi_l1_forward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_l1_forward: bad size");
    const int vec = count % 4 == 0 && aligned16(a) && aligned16(b);
    const int blocks = reduce_blocks(vec ? count / 4 : count);
    hipStream_t s = vfi::as_stream(stream);
    if (wrap) hipLaunchKernelGGL(l1_partial_kernel<true>, dim3(blocks), dim3(kThreads), 0, s, a, b, count, vec, workspace);
    else hipLaunchKernelGGL(l1_partial_kernel<false>, dim3(blocks), dim3(kThreads), 0, s, a, b, count, vec, workspace);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(kThreads), 0, s, workspace, blocks, (float)((double)scale / (double)count),
                       out);
    return vfi::check_launch("vfi_l1_forward");
}

extern "C" int vfi_l1_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b,
                               long long count, int wrap, float scale, vfi_stream_t stream) {
    VFI_REQUIRE(a && b && upstream && (grad_a || grad_b), VFI_ERR_INVALID_ARG, "vfi_l1_backward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_l1_backward: bad size");
    const float factor = (float)((double)scale / (double)count);
    if (wrap) LAUNCH_1D(l1_backward_kernel<true>, count, stream, a, b, upstream, grad_a, grad_b, count, factor);
    else LAUNCH_1D(l1_backward_kernel<false>, count, stream, a, b, upstream, grad_a, grad_b, count, factor);
    return vfi::check_launch("vfi_l1_backward");
}
