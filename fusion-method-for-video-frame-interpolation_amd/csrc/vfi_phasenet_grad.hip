// Backward of one PhaseNet level (gfx950): the HBM-bound adjoints between the existing convolution gradients
// (vfi_conv_grad.hip).  Differentiates reference src/phase_net/phase_net.py:138-139 (bilinear resize to an arbitrary size),
// :190-200 (ELU, tanh), :113-116 and :155-168 with reverse_normalize :80-98 (the per-level blends; a band level's whole
// head in one pass), and
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

// ---- adjoint of a band level's head in one pass (vfi_phasenet_predict: 1x1 64 -> 8, tanh, emit) ---------------------
// Per pixel gz = (emit adjoint + grad_pred_in) (1 - pred^2); grad_f[k] = sum_j W[j][k] gz[j];  grad_W[j][k] = sum gz[j] f[k],
// grad_b[j] = sum gz[j].  A block of 256 threads walks tiles of kHeadTile pixels of one sample:
//   A1  gz of the tile -> LDS, one (channel, pixel group) per thread;
//   A2  one (pixel group, run of feature channels) per thread: f -> LDS (only when the parameters need a gradient),
//       grad_f from W in LDS, stored;
//   B   thread t owns grad_W[2w][k], grad_W[2w+1][k] (k = t % 64, w = its wave) and sums gz f over the tile's pixels
//       in ascending order, into registers it keeps for all of the block's tiles.  grad_b rides along in every lane.
// Pixels past the end of the sample hold zeros in LDS.  Stage 2 (head_reduce_kernel) sums the block partials in
// block order.  The grid, the tiles of a block and both orders depend on (N, HW) alone: the bits repeat.
// VEC = 4: 16-byte accesses (HW, every stride and every base a multiple of 4 floats); VEC = 1 otherwise.
constexpr int kHeadTile = 128;
constexpr int kHeadRow = kHeadTile + 4;     // floats per LDS row of f; (row / 4) odd keeps ds_read_b128 over k conflict-free
constexpr int kHeadOut = 8 * 64 + 8;        // floats per block partial: grad_W (8, 64), grad_b (8)
static_assert(kMaxPartials * kHeadOut <= VFI_PHASENET_HEAD_WORKSPACE_FLOATS, "head workspace");

template <int VEC> struct HeadVec;
template <> struct HeadVec<1> { typedef float type; };
template <> struct HeadVec<4> { typedef float4 type; };
__device__ __forceinline__ float hv_get(float v, int) { return v; }
__device__ __forceinline__ float hv_get(const float4 &v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
__device__ __forceinline__ void hv_set(float &v, int, float x) { v = x; }
__device__ __forceinline__ void hv_set(float4 &v, int i, float x) {
    if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
}

struct HeadArgs {
    const float *f, *pred, *amp, *maxv, *w, *g_phase, *g_amp, *g_pred;
    long long f_bs, pred_bs, amp_bs, gp_bs, gf_bs;
    float *g_f, *part;
    int N, HW, tiles_per_sample;
};

template <int VEC, bool WGRAD>
__global__ __launch_bounds__(kThreads) void head_backward_kernel(HeadArgs a) {
    typedef typename HeadVec<VEC>::type vec;
    constexpr int PG = kHeadTile / VEC;         // pixel groups per tile
    constexpr int KPT = 64 / (kThreads / PG);   // feature channels per thread in A2
    __shared__ __attribute__((aligned(16))) float s_f[WGRAD ? 64 * kHeadRow : 4];
    __shared__ __attribute__((aligned(16))) float s_gz[8 * kHeadTile];
    __shared__ __attribute__((aligned(16))) float s_w[64 * 8];      // [k][j]
    const int t = threadIdx.x;
    for (int i = t; i < 512; i += kThreads) s_w[i] = a.w ? a.w[(i & 7) * 64 + (i >> 3)] : 0.0f;
    float acc0 = 0.0f, acc1 = 0.0f, accb0 = 0.0f, accb1 = 0.0f;
    const int HW = a.HW;
    const long long tiles = (long long)a.N * a.tiles_per_sample;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int n = (int)(tile / a.tiles_per_sample);
        const int px0 = (int)(tile - (long long)n * a.tiles_per_sample) * kHeadTile;
        __syncthreads();        // the previous tile's B has read s_f and s_gz (first tile: s_w is written)
        // A1
        for (int e = t; e < 8 * PG; e += kThreads) {
            const int j = e / PG, pg = e - j * PG, q = px0 + pg * VEC;
            vec gz;
            if (q < HW) {
                const vec y = *reinterpret_cast<const vec *>(a.pred + (size_t)n * a.pred_bs + (size_t)j * HW + q);
                vec g;
                if (j < 4) {
                    if (a.g_phase) {
                        const vec gp = *reinterpret_cast<const vec *>(a.g_phase + ((size_t)n * 4 + j) * HW + q);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) hv_set(g, v, hv_get(gp, v) * 3.14159265358979323846f);
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) hv_set(g, v, 0.0f);
                    }
                } else {
                    if (a.g_amp) {
                        const float *am = a.amp + (size_t)n * a.amp_bs + q;
                        const vec ga = *reinterpret_cast<const vec *>(a.g_amp + ((size_t)n * 4 + (j - 4)) * HW + q);
                        const vec a1 = *reinterpret_cast<const vec *>(am + (size_t)j * HW);
                        const vec a0 = *reinterpret_cast<const vec *>(am + (size_t)(j - 4) * HW);
                        const float mx = a.maxv[n];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) hv_set(g, v, hv_get(ga, v) * mx * (hv_get(a1, v) - hv_get(a0, v)) * 0.5f);
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) hv_set(g, v, 0.0f);
                    }
                }
                if (a.g_pred) {
                    const vec gi = *reinterpret_cast<const vec *>(a.g_pred + (size_t)n * a.gp_bs + (size_t)j * HW + q);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) hv_set(g, v, hv_get(g, v) + hv_get(gi, v));
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) hv_set(gz, v, hv_get(g, v) * (1.0f - hv_get(y, v) * hv_get(y, v)));
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) hv_set(gz, v, 0.0f);
            }
            *reinterpret_cast<vec *>(s_gz + j * kHeadTile + pg * VEC) = gz;
        }
        __syncthreads();
        // A2
        {
            const int pg = t % PG, k0 = (t / PG) * KPT, q = px0 + pg * VEC;
            const bool valid = q < HW;
            vec gz[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) gz[j] = *reinterpret_cast<const vec *>(s_gz + j * kHeadTile + pg * VEC);
#pragma unroll 4
            for (int kk = 0; kk < KPT; ++kk) {
                const int k = k0 + kk;
                if (WGRAD) {
                    vec fv;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) hv_set(fv, v, 0.0f);
                    if (valid) fv = *reinterpret_cast<const vec *>(a.f + (size_t)n * a.f_bs + (size_t)k * HW + q);
                    *reinterpret_cast<vec *>(s_f + k * kHeadRow + pg * VEC) = fv;
                }
                if (a.g_f && valid) {
                    const float4 w0 = *reinterpret_cast<const float4 *>(s_w + k * 8), w1 = *reinterpret_cast<const float4 *>(s_w + k * 8 + 4);
                    vec r;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float s = w0.x * hv_get(gz[0], v);
                        s = fmaf(w0.y, hv_get(gz[1], v), s);
                        s = fmaf(w0.z, hv_get(gz[2], v), s);
                        s = fmaf(w0.w, hv_get(gz[3], v), s);
                        s = fmaf(w1.x, hv_get(gz[4], v), s);
                        s = fmaf(w1.y, hv_get(gz[5], v), s);
                        s = fmaf(w1.z, hv_get(gz[6], v), s);
                        s = fmaf(w1.w, hv_get(gz[7], v), s);
                        hv_set(r, v, s);
                    }
                    *reinterpret_cast<vec *>(a.g_f + (size_t)n * a.gf_bs + (size_t)k * HW + q) = r;
                }
            }
        }
        if (WGRAD) {
            __syncthreads();
            // B
            const int k = t & 63, j0 = 2 * (t >> 6);
            const float4 *fr = reinterpret_cast<const float4 *>(s_f + k * kHeadRow);
            const float4 *g0 = reinterpret_cast<const float4 *>(s_gz + j0 * kHeadTile), *g1 = g0 + kHeadTile / 4;
#pragma unroll 4
            for (int p = 0; p < kHeadTile / 4; ++p) {
                const float4 fv = fr[p], u = g0[p], v = g1[p];
                acc0 = fmaf(u.x, fv.x, acc0); acc0 = fmaf(u.y, fv.y, acc0); acc0 = fmaf(u.z, fv.z, acc0); acc0 = fmaf(u.w, fv.w, acc0);
                acc1 = fmaf(v.x, fv.x, acc1); acc1 = fmaf(v.y, fv.y, acc1); acc1 = fmaf(v.z, fv.z, acc1); acc1 = fmaf(v.w, fv.w, acc1);
                accb0 += u.x; accb0 += u.y; accb0 += u.z; accb0 += u.w;
                accb1 += v.x; accb1 += v.y; accb1 += v.z; accb1 += v.w;
            }
        }
    }
    if (WGRAD) {
        float *out = a.part + (size_t)blockIdx.x * kHeadOut;
        const int k = t & 63, j0 = 2 * (t >> 6);
        out[j0 * 64 + k] = acc0;
        out[(j0 + 1) * 64 + k] = acc1;
        if (k == 0) { out[512 + j0] = accb0; out[512 + j0 + 1] = accb1; }
    }
}

// stage 2 (one block): every output sums its column of the partials in block order
__global__ __launch_bounds__(kThreads) void head_reduce_kernel(const float *__restrict__ part, int blocks, float *__restrict__ g_w,
                                                               float *__restrict__ g_b) {
    for (int o = threadIdx.x; o < kHeadOut; o += kThreads) {
        float v = 0.0f;
        for (int b = 0; b < blocks; ++b) v += part[(size_t)b * kHeadOut + o];
        if (o < 512) { if (g_w) g_w[o] = v; }
        else if (g_b) g_b[o - 512] = v;
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

extern "C" int vfi_phasenet_predict_backward(const float *feat, long long feat_bstride, const float *pred, long long pred_bstride,
                                             const float *amp_in, long long amp_bstride, const float *max_amp, const float *weight,
                                             const float *grad_phase, const float *grad_amp, const float *grad_pred_in,
                                             long long gpi_bstride, float *grad_feat, long long gf_bstride, float *grad_weight,
                                             float *grad_bias, float *workspace, int N, int HW, vfi_stream_t stream) {
    const bool wgrad = grad_weight || grad_bias;
    VFI_REQUIRE(pred && (grad_feat || wgrad), VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_backward: null pointer");
    VFI_REQUIRE(!grad_feat || weight, VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_backward: grad_feat needs the weights");
    VFI_REQUIRE(!wgrad || (feat && workspace), VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_backward: parameter gradients need feat and a workspace");
    VFI_REQUIRE(!grad_amp || (amp_in && max_amp), VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_backward: amplitudes missing");
    VFI_REQUIRE(N > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_backward: bad sizes");
    VFI_REQUIRE(64ll * HW < (1ll << 31), VFI_ERR_UNSUPPORTED, "vfi_phasenet_predict_backward: per-sample tensor too large for 32-bit pixel indices");
    HeadArgs a{};
    a.f = feat; a.pred = pred; a.amp = amp_in; a.maxv = max_amp; a.w = weight; a.g_phase = grad_phase; a.g_amp = grad_amp;
    a.g_pred = grad_pred_in; a.f_bs = feat_bstride; a.pred_bs = pred_bstride; a.amp_bs = amp_bstride; a.gp_bs = gpi_bstride;
    a.gf_bs = gf_bstride; a.g_f = grad_feat; a.part = workspace; a.N = N; a.HW = HW;
    a.tiles_per_sample = (HW + kHeadTile - 1) / kHeadTile;
    const long long tiles = (long long)N * a.tiles_per_sample;
    const int blocks = (int)(tiles < kMaxPartials ? tiles : kMaxPartials);
    const bool v4 = HW % 4 == 0 && aligned16(pred) && pred_bstride % 4 == 0 && (!wgrad || (aligned16(feat) && feat_bstride % 4 == 0)) &&
                    (!grad_feat || (aligned16(grad_feat) && gf_bstride % 4 == 0)) && (!grad_phase || aligned16(grad_phase)) &&
                    (!grad_amp || (aligned16(grad_amp) && aligned16(amp_in) && amp_bstride % 4 == 0)) &&
                    (!grad_pred_in || (aligned16(grad_pred_in) && gpi_bstride % 4 == 0));
    hipStream_t s = vfi::as_stream(stream);
    if (wgrad) {
        if (v4) hipLaunchKernelGGL((head_backward_kernel<4, true>), dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL((head_backward_kernel<1, true>), dim3(blocks), dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(head_reduce_kernel, dim3(1), dim3(kThreads), 0, s, workspace, blocks, grad_weight, grad_bias);
    } else {
        if (v4) hipLaunchKernelGGL((head_backward_kernel<4, false>), dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL((head_backward_kernel<1, false>), dim3(blocks), dim3(kThreads), 0, s, a);
    }
    return vfi::check_launch("vfi_phasenet_predict_backward");
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
