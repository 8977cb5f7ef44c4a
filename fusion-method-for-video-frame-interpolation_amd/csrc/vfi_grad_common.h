// What the backward passes share (gfx950): launch scaffolding, the fixed-order block sum, the strided elementwise pass,
// the two-stage scalar reduction and the x2 bilinear gather.  vfi_conv_grad.hip, vfi_adacofnet_grad.hip and
// vfi_phasenet_grad.hip are built on it; vfi_aux.hip and vfi_adacof.hip take the launch helpers alone.
//
// The three rules of every training path ("The rules"):
//   1. no float atomics;
//   2. one writer per output element;
//   3. every reduction runs in an order fixed by the shape alone (never by the device, the grid the runtime picked or
//      the arrival order of blocks), so the same inputs give the same bits on every run and every device.
// Rule 3 rests on reduce_blocks, block_sum and the (x+y)+(z+w) grouping below: they exist once, here.
#pragma once
#include "vfi_common.h"

#include <cstdint>

// Anonymous: each translation unit gets kernels of its own, as with every other kernel of the library.
namespace {

constexpr int kThreads = 256;
constexpr int kMaxPartials = 1024;      // blocks of a two-stage reduction
static_assert(4 * kMaxPartials <= VFI_REDUCE_WORKSPACE_FLOATS, "reduce workspace: four sums of kMaxPartials partials");

// reduction grids depend on the element count alone, so the summation order -- and the bits -- repeat
inline int reduce_blocks(long long n) {
    long long b = (n + kThreads - 1) / kThreads;
    return (int)(b < 1 ? 1 : (b > kMaxPartials ? kMaxPartials : b));
}
__host__ __device__ inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

#define LAUNCH_1D(kernel, total, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3(vfi::blocks_1d(total)), dim3(kThreads), 0, vfi::as_stream(stream), __VA_ARGS__)

#define GRID_STRIDE(i, total) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (long long)gridDim.x * blockDim.x)

// sums v[0..NV) over the block in a fixed tree order; the result is valid in thread 0
template <int NV> __device__ __forceinline__ void block_sum(float *v, float *lds) {
#pragma unroll
    for (int q = 0; q < NV; ++q) lds[q * kThreads + threadIdx.x] = v[q];
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int q = 0; q < NV; ++q) lds[q * kThreads + threadIdx.x] += lds[q * kThreads + threadIdx.x + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = lds[q * kThreads];
}

// component i of a float (i ignored) or a float4
__device__ __forceinline__ float lane_get(float v, int) { return v; }
__device__ __forceinline__ float lane_get(const float4 &v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
__device__ __forceinline__ void lane_set(float &v, int, float x) { v = x; }
__device__ __forceinline__ void lane_set(float4 &v, int i, float x) {
    if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
}

// ---- the elementwise pass -------------------------------------------------------------------------------------------
// out[n][e] = F(a[n][e], b[n][e], c[n][e], c != NULL) per float, over N batch-strided runs of `count`.  T = float, or
// float4 with count and strides in units of T.  out may be a itself; c may be NULL (F then sees 0 and false).
template <typename F, typename T>
__global__ void map_kernel(const T *a, long long a_bs, const T *__restrict__ b, long long b_bs, const T *__restrict__ c,
                           long long c_bs, T *out, long long o_bs, int N, long long count) {
    constexpr int L = sizeof(T) / sizeof(float);
    GRID_STRIDE(i, (long long)N * count) {
        const long long n = i / count, e = i - n * count;
        const T x = a[n * a_bs + e], y = b[n * b_bs + e];
        T z, r;
        if (c) z = c[n * c_bs + e];
#pragma unroll
        for (int l = 0; l < L; ++l) lane_set(r, l, F()(lane_get(x, l), lane_get(y, l), c ? lane_get(z, l) : 0.0f, c != nullptr));
        out[n * o_bs + e] = r;
    }
}

// 16-byte accesses when the count, every stride and every base allow, else 4-byte: the same values either way
template <typename F>
void launch_map(const float *a, long long a_bs, const float *b, long long b_bs, const float *c, long long c_bs, float *out,
                long long o_bs, int N, long long count, vfi_stream_t stream) {
    if (count % 4 == 0 && a_bs % 4 == 0 && b_bs % 4 == 0 && c_bs % 4 == 0 && o_bs % 4 == 0 && aligned16(a) && aligned16(b) &&
        aligned16(c) && aligned16(out))
        LAUNCH_1D((map_kernel<F, float4>), (long long)N * count / 4, stream, reinterpret_cast<const float4 *>(a), a_bs / 4,
                  reinterpret_cast<const float4 *>(b), b_bs / 4, reinterpret_cast<const float4 *>(c), c_bs / 4,
                  reinterpret_cast<float4 *>(out), o_bs / 4, N, count / 4);
    else
        LAUNCH_1D((map_kernel<F, float>), (long long)N * count, stream, a, a_bs, b, b_bs, c, c_bs, out, o_bs, N, count);
}

// g * f'(y) from the activation's output y.  ELU (alpha = 1): y > 0 ? 1 : y + 1 (for y <= 0, y = e^z - 1 and
// dy/dz = e^z);  tanh: 1 - y^2;  sigmoid: y (1 - y)
template <int ACT> struct ActGrad {
    __device__ __forceinline__ float operator()(float g, float y, float, bool) const {
        return ACT == VFI_ACT_ELU ? (y > 0.0f ? g : g * (y + 1.0f)) : ACT == VFI_ACT_TANH ? g * (1.0f - y * y) : g * y * (1.0f - y);
    }
};

// ---- the two-stage scalar reduction ---------------------------------------------------------------------------------
// out[0] = factor * sum_i TERM(a[i] - b[i]); b == NULL is zero.  TERM gives the summand from the difference d, and
// grad(d, s) the derivative of s * TERM(d).
struct CharbonnierTerm {        // sqrt(d^2 + e^2)
    float eps2;
    __device__ __forceinline__ float operator()(float d) const { return sqrtf(d * d + eps2); }
    __device__ __forceinline__ float grad(float d, float s) const { return s * d * rsqrtf(d * d + eps2); }
};
struct SquareTerm {             // d^2 (nn.MSELoss)
    __device__ __forceinline__ float operator()(float d) const { return d * d; }
    __device__ __forceinline__ float grad(float d, float s) const { return 2.0f * s * d; }
};
// |wrap(d)|, wrap(d) = atan2(sin d, cos d): d brought to (-pi, pi] (the phase loss); |d| without WRAP
template <bool WRAP> struct AbsTerm {
    __device__ __forceinline__ float wrapped(float d) const { return WRAP ? atan2f(sinf(d), cosf(d)) : d; }
    __device__ __forceinline__ float operator()(float d) const { return fabsf(wrapped(d)); }
    __device__ __forceinline__ float grad(float d, float s) const {
        const float w = wrapped(d);
        return w > 0.0f ? s : (w < 0.0f ? -s : 0.0f);
    }
};

// stage 1: per block, the sum of the terms; the grid is reduce_blocks(vec ? count / 4 : count).  vec (count a multiple
// of 4, both bases 16-byte aligned; decided by the host): 16-byte loads, each summed as (x + y) + (z + w).  Keep the
// 16-byte body as "subtract in place, then the four terms": written as term(p.x - q.x) + ... the compiler contracts
// Charbonnier's d * d + e^2 into one fma where this form gives a packed multiply and an add, and the sum's last bits move.
template <typename TERM>
__global__ __launch_bounds__(kThreads) void sum_partial_kernel(TERM term, const float *__restrict__ a, const float *__restrict__ b,
                                                               long long count, int vec, float *__restrict__ part) {
    __shared__ float lds[kThreads];
    float v[1] = {0.0f};
    if (vec) {
        const float4 *a4 = reinterpret_cast<const float4 *>(a), *b4 = reinterpret_cast<const float4 *>(b);
        GRID_STRIDE(i, count / 4) {
            float4 d = a4[i];
            if (b) { const float4 t = b4[i]; d.x -= t.x; d.y -= t.y; d.z -= t.z; d.w -= t.w; }
            v[0] += (term(d.x) + term(d.y)) + (term(d.z) + term(d.w));
        }
    } else {
        GRID_STRIDE(i, count) v[0] += term(a[i] - (b ? b[i] : 0.0f));
    }
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}
// stage 2 (one block): out[0] = factor * sum of the partials (a template so that only its users emit it)
template <typename = void>
__global__ __launch_bounds__(kThreads) void sum_final_kernel(const float *__restrict__ part, int blocks, float factor,
                                                             float *__restrict__ out) {
    __shared__ float lds[kThreads];
    float v[1] = {0.0f};
    for (int b = threadIdx.x; b < blocks; b += kThreads) v[0] += part[b];
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) out[0] = v[0] * factor;
}
// g_a = upstream * factor * TERM'(a - b), g_b = -g_a; either may be NULL
template <typename TERM>
__global__ void sum_backward_kernel(TERM term, const float *__restrict__ a, const float *__restrict__ b,
                                    const float *__restrict__ up, float *__restrict__ ga, float *__restrict__ gb,
                                    long long count, float factor) {
    const float s = up[0] * factor;
    GRID_STRIDE(i, count) {
        const float v = term.grad(a[i] - (b ? b[i] : 0.0f), s);
        if (ga) ga[i] = v;
        if (gb) gb[i] = -v;
    }
}

template <typename TERM>
int launch_sum_forward(TERM term, const float *a, const float *b, long long count, float factor, float *workspace, float *out,
                       vfi_stream_t stream, const char *what) {
    const int vec = count % 4 == 0 && aligned16(a) && aligned16(b);
    const int blocks = reduce_blocks(vec ? count / 4 : count);
    hipStream_t s = vfi::as_stream(stream);
    hipLaunchKernelGGL(sum_partial_kernel<TERM>, dim3(blocks), dim3(kThreads), 0, s, term, a, b, count, vec, workspace);
    hipLaunchKernelGGL(sum_final_kernel<>, dim3(1), dim3(kThreads), 0, s, workspace, blocks, factor, out);
    return vfi::check_launch(what);
}

// ---- adjoint of a x2 bilinear resize, gather form -------------------------------------------------------------------
// One thread per source element sums its weighted output gradients, rows outermost, r = sum wx g, v += wy r, in the
// order the tap rule lists them.  SOURCES(j, n, o, w) fills the outputs of one axis that read source j of n and their
// weights (at most KMAX) and returns their count.  `y` (optional) is the source itself when it is a ReLU's output: the
// result is multiplied by [y > 0].
template <int KMAX, int (*SOURCES)(int, int, int *, float *)>
__global__ void up2_backward_kernel(const float *__restrict__ g, long long g_bs, const float *__restrict__ y, long long y_bs,
                                    float *__restrict__ gx, long long gx_bs, int N, int C, int Hi, int Wi) {
    const int Ho = 2 * Hi, Wo = 2 * Wi;
    GRID_STRIDE(i, (long long)N * C * Hi * Wi) {
        const int xj = i % Wi, yj = (i / Wi) % Hi, c = (i / ((long long)Wi * Hi)) % C, n = i / ((long long)Wi * Hi * C);
        const size_t src = ((size_t)c * Hi + yj) * Wi + xj;
        float v = 0.0f;
        if (!y || y[(size_t)n * y_bs + src] > 0.0f) {
            int oy[KMAX], ox[KMAX];
            float wy[KMAX], wx[KMAX];
            const int ky = SOURCES(yj, Hi, oy, wy), kx = SOURCES(xj, Wi, ox, wx);
            const float *gp = g + (size_t)n * g_bs + (size_t)c * Ho * Wo;
            for (int a = 0; a < ky; ++a) {
                float r = 0.0f;
                for (int b = 0; b < kx; ++b) r += wx[b] * gp[(size_t)oy[a] * Wo + ox[b]];
                v += wy[a] * r;
            }
        }
        gx[(size_t)n * gx_bs + src] = v;
    }
}

}  // namespace
