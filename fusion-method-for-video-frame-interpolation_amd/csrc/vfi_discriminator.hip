// The AdaCoF trainer's discriminator (reference src/adacof/losses/discriminator.py), the pieces the other files do not
// have:
//   * the phase split that turns a 3x3 / stride 2 / pad 1 convolution into a 3x3 / stride 1 one over 4C channels, and its
//     adjoint (the convolutions themselves, forward and both gradients, are vfi_conv2d* on the split tensor);
//   * the classifier's linear layers with a fused LeakyReLU, forward and backward;
//   * the WGAN_GP term's streaming pieces (section 28): LeakyReLU as a mask read off another tensor's sign, the interpolate
//     between the fake and the real batch, the gradient penalty and its adjoint.
// The rules of section 12 hold: no float atomics, one writer per element, every sum in an order fixed by the shape.
#include "vfi_grad_common.h"

namespace {

// ---- phase split / merge ------------------------------------------------------------------------------------------
// xs[n, (2 py + px) C + c, i, j] = x[n, c, 2 i + py, 2 j + px], zero beyond the edge; H2 = ceil(H / 2), W2 = ceil(W / 2).
// One thread per (n, c, i, group of VJ output columns): it touches 2 rows x 2 VJ columns of x and VJ columns of each of
// the four phase planes.  VJ = 4 (W a multiple of 8, strides multiples of 4, bases 16-byte aligned): two 16-byte accesses
// per row of x, one per phase plane.  VJ = 1: 4-byte accesses, any shape.  MERGE: the adjoint, xs -> x (the zero fill is
// dropped: only positions inside H x W are written).
template <int VJ, bool MERGE>
__global__ __launch_bounds__(kThreads) void phase_kernel(const float *__restrict__ src, long long s_bs, float *__restrict__ dst,
                                                         long long d_bs, int N, int C, int H, int W) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2, G = (W2 + VJ - 1) / VJ;
    const size_t plane2 = (size_t)H2 * W2;
    GRID_STRIDE(t, (long long)N * C * H2 * G) {
        const int g = (int)(t % G), i = (int)((t / G) % H2), c = (int)((t / ((long long)G * H2)) % C);
        const long long n = t / ((long long)G * H2 * C);
        // x side: (n, c, 2 i + py, 2 VJ g ...); xs side: (n, ph C + c, i, VJ g ...)
        const float *xs_c = nullptr;
        float *xs_m = nullptr;
        const float *x_c = nullptr;
        float *x_m = nullptr;
        if (MERGE) { xs_c = src + n * s_bs; x_m = dst + n * d_bs + (size_t)c * H * W; }
        else { x_c = src + n * s_bs + (size_t)c * H * W; xs_m = dst + n * d_bs; }
        const size_t so = (size_t)i * W2 + (size_t)g * VJ;      // offset inside a phase plane
        if (VJ == 4) {
            float4 ph[4];
            if (MERGE) {
#pragma unroll
                for (int p = 0; p < 4; ++p) ph[p] = *reinterpret_cast<const float4 *>(xs_c + ((size_t)p * C + c) * plane2 + so);
#pragma unroll
                for (int py = 0; py < 2; ++py) {
                    const int r = 2 * i + py;
                    if (r >= H) continue;
                    const float4 e = ph[2 * py], o = ph[2 * py + 1];
                    float4 *d = reinterpret_cast<float4 *>(x_m + (size_t)r * W + (size_t)g * 8);
                    d[0] = make_float4(e.x, o.x, e.y, o.y);
                    d[1] = make_float4(e.z, o.z, e.w, o.w);
                }
            } else {
#pragma unroll
                for (int py = 0; py < 2; ++py) {
                    const int r = 2 * i + py;
                    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
                    if (r < H) {
                        const float4 *s = reinterpret_cast<const float4 *>(x_c + (size_t)r * W + (size_t)g * 8);
                        a = s[0];
                        b = s[1];
                    }
                    ph[2 * py] = make_float4(a.x, a.z, b.x, b.z);
                    ph[2 * py + 1] = make_float4(a.y, a.w, b.y, b.w);
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) *reinterpret_cast<float4 *>(xs_m + ((size_t)p * C + c) * plane2 + so) = ph[p];
            }
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int r = 2 * i + (p >> 1), q = 2 * g + (p & 1);
                const bool in = r < H && q < W;
                const size_t xo = (size_t)r * W + q, po = ((size_t)p * C + c) * plane2 + so;
                if (MERGE) { if (in) x_m[xo] = xs_c[po]; }
                else xs_m[po] = in ? x_c[xo] : 0.0f;
            }
        }
    }
}

template <bool MERGE>
int launch_phase(const float *src, long long s_bs, float *dst, long long d_bs, int N, int C, int H, int W, vfi_stream_t stream,
                 const char *what) {
    VFI_REQUIRE(src && dst, VFI_ERR_INVALID_ARG, "%s: null pointer", what);
    VFI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, VFI_ERR_INVALID_ARG, "%s: bad sizes", what);
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    VFI_REQUIRE(4ll * C * H2 * W2 < (1ll << 31) && H < (1 << 20) && W < (1 << 20), VFI_ERR_UNSUPPORTED,
                "%s: per-sample tensor too large (C = %d, %dx%d)", what, C, H, W);
    const bool v4 = W % 8 == 0 && s_bs % 4 == 0 && d_bs % 4 == 0 && aligned16(src) && aligned16(dst);
    if (v4) LAUNCH_1D((phase_kernel<4, MERGE>), (long long)N * C * H2 * (W2 / 4), stream, src, s_bs, dst, d_bs, N, C, H, W);
    else LAUNCH_1D((phase_kernel<1, MERGE>), (long long)N * C * H2 * W2, stream, src, s_bs, dst, d_bs, N, C, H, W);
    return vfi::check_launch(what);
}

// ---- linear layers --------------------------------------------------------------------------------------------------
constexpr int kLinRows = 4;     // rows of w (outputs j) per workgroup of the forward
constexpr int kLinBatch = 4;    // samples per slice: a slice's accumulators live in registers

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.0f ? v : v * slope; }
// the upstream gradient of the pre-activation: g times the LeakyReLU's derivative, read off the output's sign (slope > 0)
__device__ __forceinline__ float masked(const float *__restrict__ g, const float *__restrict__ y, long long i, float slope) {
    const float v = g[i];
    return (y && !(y[i] > 0.0f)) ? v * slope : v;
}

// y[b, j] = leaky(sum_k x[b, k] w[j, k] + bias[j]).  Workgroup r takes rows j = 4 r .. 4 r + 3 of w and one slice of up to
// four samples: thread t walks k = t, t + 256, ... (units of T), one accumulator per (row, sample, lane of T), so every
// element of w is loaded once per slice -- 16 bytes per load when T = float4 -- while the slice of x (a few MB at most)
// is re-read by the workgroups from the caches.  The sum: each lane's chain in k order, (x + y) + (z + w) over the lanes,
// block_sum's tree over the threads -- fixed by K alone.
template <typename T>
__global__ __launch_bounds__(kThreads) void linear_forward_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                  const float *__restrict__ bias, float *__restrict__ y, int B,
                                                                  int K, int J, float slope) {
    constexpr int L = sizeof(T) / sizeof(float);
    __shared__ float lds[kLinRows * kLinBatch * kThreads];
    const int j0 = blockIdx.x * kLinRows, b0 = blockIdx.y * kLinBatch;
    const int nb = B - b0 < kLinBatch ? B - b0 : kLinBatch;
    const int KT = K / L;
    float acc[kLinRows][kLinBatch][L];
#pragma unroll
    for (int r = 0; r < kLinRows; ++r)
#pragma unroll
        for (int b = 0; b < kLinBatch; ++b)
#pragma unroll
            for (int l = 0; l < L; ++l) acc[r][b][l] = 0.0f;
    // rows and samples beyond the edge repeat the last valid one (their sums are dropped below): no branch in the loop
    const T *wr[kLinRows], *xr[kLinBatch];
#pragma unroll
    for (int r = 0; r < kLinRows; ++r) wr[r] = reinterpret_cast<const T *>(w + (size_t)(j0 + r < J ? j0 + r : J - 1) * K);
#pragma unroll
    for (int b = 0; b < kLinBatch; ++b) xr[b] = reinterpret_cast<const T *>(x + (size_t)(b0 + (b < nb ? b : nb - 1)) * K);
    for (int k = threadIdx.x; k < KT; k += kThreads) {
        T wv[kLinRows], xv[kLinBatch];
#pragma unroll
        for (int r = 0; r < kLinRows; ++r) wv[r] = wr[r][k];
#pragma unroll
        for (int b = 0; b < kLinBatch; ++b) xv[b] = xr[b][k];
#pragma unroll
        for (int r = 0; r < kLinRows; ++r)
#pragma unroll
            for (int b = 0; b < kLinBatch; ++b)
#pragma unroll
                for (int l = 0; l < L; ++l) acc[r][b][l] = fmaf(lane_get(wv[r], l), lane_get(xv[b], l), acc[r][b][l]);
    }
    float v[kLinRows * kLinBatch];
#pragma unroll
    for (int r = 0; r < kLinRows; ++r)
#pragma unroll
        for (int b = 0; b < kLinBatch; ++b)
        {
            if constexpr (L == 4) v[r * kLinBatch + b] = (acc[r][b][0] + acc[r][b][1]) + (acc[r][b][2] + acc[r][b][3]);
            else v[r * kLinBatch + b] = acc[r][b][0];
        }
    block_sum<kLinRows * kLinBatch>(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < kLinRows; ++r)
#pragma unroll
            for (int b = 0; b < kLinBatch; ++b)
                if (j0 + r < J && b < nb) y[(size_t)(b0 + b) * J + j0 + r] = leaky(v[r * kLinBatch + b] + (bias ? bias[j0 + r] : 0.0f), slope);
    }
}

// Backward.  gm[b, j] = g[b, j] * leaky'(y[b, j]).  A workgroup of 64 threads owns the columns k of its slab (one T per
// thread) and walks j = 0 .. J - 1 in order, eight rows of w per trip (their loads are issued together):
//   dw[j, k] = sum_b gm[b, j] x[b, k]   written as it is formed (x's slab sits in registers),
//   dx[b, k] = sum_j gm[b, j] w[j, k]   accumulated in registers, written at the end,
// so w is read once and dw written once; dbias[j] = sum_b gm[b, j] comes from one more workgroup, a thread per j.  B beyond
// four samples: further slices of four in order, which add to dw and dbias (the same thread reads and writes its own
// elements) and read w again.
constexpr int kLinBackThreads = 64;
constexpr int kLinBackRows = 8;
template <typename T, bool HAS_DX, bool HAS_DW>
__global__ __launch_bounds__(kLinBackThreads) void linear_backward_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                          const float *__restrict__ y, float slope,
                                                                          const float *__restrict__ g, float *__restrict__ dx,
                                                                          float *__restrict__ dw, float *__restrict__ dbias, int B,
                                                                          int K, int J, int slabs) {
    constexpr int L = sizeof(T) / sizeof(float);
    if ((int)blockIdx.x == slabs) {         // the bias workgroup (launched only when dbias is wanted)
        for (int j = threadIdx.x; j < J; j += kLinBackThreads) {
            float s = 0.0f;
            for (int b = 0; b < B; ++b) s += masked(g, y, (long long)b * J + j, slope);
            dbias[j] = s;
        }
        return;
    }
    const int KT = K / L;
    const int k = blockIdx.x * kLinBackThreads + threadIdx.x;
    if (k >= KT) return;
    for (int b0 = 0; b0 < B; b0 += kLinBatch) {
        const int nb = B - b0 < kLinBatch ? B - b0 : kLinBatch;
        T xv[kLinBatch], ax[kLinBatch];
#pragma unroll
        for (int b = 0; b < kLinBatch; ++b) {
#pragma unroll
            for (int l = 0; l < L; ++l) { lane_set(xv[b], l, 0.0f); lane_set(ax[b], l, 0.0f); }
            if (HAS_DW && b < nb) xv[b] = reinterpret_cast<const T *>(x + (size_t)(b0 + b) * K)[k];
        }
        for (int j0 = 0; j0 < J; j0 += kLinBackRows) {
            // rows beyond J repeat the last one: loaded, never used
            T wv[kLinBackRows], dv[kLinBackRows];
            float gm[kLinBackRows][kLinBatch];
#pragma unroll
            for (int u = 0; u < kLinBackRows; ++u) {
                const int j = j0 + u < J ? j0 + u : J - 1;
                if (HAS_DX) wv[u] = reinterpret_cast<const T *>(w + (size_t)j * K)[k];
                if (HAS_DW && b0) dv[u] = reinterpret_cast<const T *>(dw + (size_t)j * K)[k];
#pragma unroll
                for (int b = 0; b < kLinBatch; ++b) gm[u][b] = b < nb ? masked(g, y, (long long)(b0 + b) * J + j, slope) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kLinBackRows; ++u) {
                if (j0 + u >= J) break;
                if (HAS_DX) {
#pragma unroll
                    for (int b = 0; b < kLinBatch; ++b)
#pragma unroll
                        for (int l = 0; l < L; ++l) lane_set(ax[b], l, fmaf(gm[u][b], lane_get(wv[u], l), lane_get(ax[b], l)));
                }
                if (HAS_DW) {
                    T r;
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        float s = b0 ? lane_get(dv[u], l) : 0.0f;
#pragma unroll
                        for (int b = 0; b < kLinBatch; ++b) s = fmaf(gm[u][b], lane_get(xv[b], l), s);
                        lane_set(r, l, s);
                    }
                    reinterpret_cast<T *>(dw + (size_t)(j0 + u) * K)[k] = r;
                }
            }
        }
        if (HAS_DX)
            for (int b = 0; b < nb; ++b) reinterpret_cast<T *>(dx + (size_t)(b0 + b) * K)[k] = ax[b];
    }
}

template <typename T>
void launch_linear_backward(const float *x, const float *w, const float *y, float slope, const float *g, float *dx, float *dw,
                            float *dbias, int B, int K, int J, hipStream_t s) {
    constexpr int L = sizeof(T) / sizeof(float);
    const int slabs = (dx || dw) ? vfi::ceil_div(K / L, kLinBackThreads) : 0;
    const dim3 grid(slabs + (dbias ? 1 : 0)), block(kLinBackThreads);
#define VFI_LB(DX, DW) hipLaunchKernelGGL((linear_backward_kernel<T, DX, DW>), grid, block, 0, s, x, w, y, slope, g, dx, dw, dbias, B, K, J, slabs)
    if (dx && dw) VFI_LB(true, true);
    else if (dx) VFI_LB(true, false);
    else if (dw) VFI_LB(false, true);
    else VFI_LB(false, false);
#undef VFI_LB
}

// ---- the WGAN_GP term ----------------------------------------------------------------------------
// out = s > 0 ? a : slope a.  No __restrict__: s may be a, out may be a (each thread reads its element before it writes it).
template <typename T>
__global__ void leaky_mask_kernel(const T *a, long long a_bs, const T *s, long long s_bs, T *out, long long o_bs, int N,
                                  long long count, float slope) {
    constexpr int L = sizeof(T) / sizeof(float);
    GRID_STRIDE(i, (long long)N * count) {
        const long long n = i / count, e = i - n * count;
        const T x = a[n * a_bs + e], y = s[n * s_bs + e];
        T r;
#pragma unroll
        for (int l = 0; l < L; ++l) lane_set(r, l, lane_get(y, l) > 0.0f ? lane_get(x, l) : lane_get(x, l) * slope);
        out[n * o_bs + e] = r;
    }
}

// fake (1 - eps) + real eps in four roundings: contraction is off for this function alone, so neither product fuses with
// the sum (torch's float32 expression rounds each of `1 - eps`, the two `mul`s and the `+`)
__device__ __forceinline__ float gp_mix_one(float f, float r, float e) {
#pragma clang fp contract(off)
    const float om = 1.0f - e;
    const float p = f * om;
    const float q = r * e;
    return p + q;
}
template <typename T>
__global__ void gp_mix_kernel(const T *__restrict__ fake, long long f_bs, const T *__restrict__ real, long long r_bs,
                              const T *__restrict__ eps, long long e_bs, T *__restrict__ hat, long long h_bs, int N,
                              long long count) {
    constexpr int L = sizeof(T) / sizeof(float);
    GRID_STRIDE(i, (long long)N * count) {
        const long long n = i / count, e = i - n * count;
        const T f = fake[n * f_bs + e], r = real[n * r_bs + e], ep = eps[n * e_bs + e];
        T h;
#pragma unroll
        for (int l = 0; l < L; ++l) lane_set(h, l, gp_mix_one(lane_get(f, l), lane_get(r, l), lane_get(ep, l)));
        hat[n * h_bs + e] = h;
    }
}

// norms[b] = sqrt(sum_i g[b][i]^2): workgroup b; thread t takes i = t, t + 256, ... (units of T), alternating between two
// accumulators per lane (shorter chains, two loads in flight), then (lane sums) and block_sum's tree.
template <typename T>
__global__ __launch_bounds__(kThreads) void grad_norm_kernel(const float *__restrict__ g, long long g_bs, float *__restrict__ norms,
                                                             long long n) {
    constexpr int L = sizeof(T) / sizeof(float);
    __shared__ float lds[kThreads];
    const T *row = reinterpret_cast<const T *>(g + (long long)blockIdx.x * g_bs);
    const long long nt = n / L;
    float acc[2][L];
#pragma unroll
    for (int l = 0; l < L; ++l) acc[0][l] = acc[1][l] = 0.0f;
    for (long long k = threadIdx.x; k < nt; k += 2 * kThreads) {
        const T u = row[k];
        const bool two = k + kThreads < nt;
        T w;
        if (two) w = row[k + kThreads];
#pragma unroll
        for (int l = 0; l < L; ++l) {
            acc[0][l] = fmaf(lane_get(u, l), lane_get(u, l), acc[0][l]);
            if (two) acc[1][l] = fmaf(lane_get(w, l), lane_get(w, l), acc[1][l]);
        }
    }
    float v[1];
    if constexpr (L == 4) v[0] = ((acc[0][0] + acc[1][0]) + (acc[0][1] + acc[1][1])) + ((acc[0][2] + acc[1][2]) + (acc[0][3] + acc[1][3]));
    else v[0] = acc[0][0] + acc[1][0];
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) norms[blockIdx.x] = sqrtf(v[0]);
}

// value = factor * sum_b (norms[b] - 1)^2, one workgroup, the tree fixed by B
__global__ __launch_bounds__(kThreads) void grad_penalty_value_kernel(const float *__restrict__ norms, int B, float factor,
                                                                      float *__restrict__ value) {
    __shared__ float lds[kThreads];
    float v[1] = {0.0f};
    for (int b = threadIdx.x; b < B; b += kThreads) {
        const float d = norms[b] - 1.0f;
        v[0] += d * d;
    }
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) value[0] = v[0] * factor;
}

// out[b] = c_b g[b], c_b = upstream 2 weight (norm_b - 1) / (B norm_b) formed in double and rounded once; blockIdx.y = b
template <typename T>
__global__ void grad_penalty_backward_kernel(const T *__restrict__ g, long long g_bs, const float *__restrict__ norms,
                                             const float *__restrict__ up, T *__restrict__ out, long long o_bs, long long nt,
                                             double two_weight_over_b) {
    constexpr int L = sizeof(T) / sizeof(float);
    const int b = blockIdx.y;
    const double nb = (double)norms[b];
    const float c = nb == 0.0 ? 0.0f : (float)((double)up[0] * two_weight_over_b * (nb - 1.0) / nb);
    const T *row = g + (long long)b * g_bs;
    T *dst = out + (long long)b * o_bs;
    GRID_STRIDE(i, nt) {
        const T x = row[i];
        T r;
#pragma unroll
        for (int l = 0; l < L; ++l) lane_set(r, l, nb == 0.0 ? 0.0f : c * lane_get(x, l));
        dst[i] = r;
    }
}

}  // namespace

extern "C" int vfi_leaky_mask(const float *a, long long a_bstride, const float *s, long long s_bstride, float *out,
                              long long out_bstride, int N, long long count, float slope, vfi_stream_t stream) {
    VFI_REQUIRE(a && s && out, VFI_ERR_INVALID_ARG, "vfi_leaky_mask: null pointer");
    VFI_REQUIRE(N > 0 && count > 0, VFI_ERR_INVALID_ARG, "vfi_leaky_mask: bad sizes");
    VFI_REQUIRE(slope > 0.0f, VFI_ERR_INVALID_ARG, "vfi_leaky_mask: slope %g (must be positive; 1 = no activation)", (double)slope);
    if (count % 4 == 0 && a_bstride % 4 == 0 && s_bstride % 4 == 0 && out_bstride % 4 == 0 && aligned16(a) && aligned16(s) &&
        aligned16(out))
        LAUNCH_1D(leaky_mask_kernel<float4>, (long long)N * count / 4, stream, reinterpret_cast<const float4 *>(a), a_bstride / 4,
                  reinterpret_cast<const float4 *>(s), s_bstride / 4, reinterpret_cast<float4 *>(out), out_bstride / 4, N,
                  count / 4, slope);
    else
        LAUNCH_1D(leaky_mask_kernel<float>, (long long)N * count, stream, a, a_bstride, s, s_bstride, out, out_bstride, N, count,
                  slope);
    return vfi::check_launch("vfi_leaky_mask");
}

extern "C" int vfi_gp_mix(const float *fake, long long f_bstride, const float *real, long long r_bstride, const float *eps,
                          long long e_bstride, float *hat, long long h_bstride, int N, long long count, vfi_stream_t stream) {
    VFI_REQUIRE(fake && real && eps && hat, VFI_ERR_INVALID_ARG, "vfi_gp_mix: null pointer");
    VFI_REQUIRE(N > 0 && count > 0, VFI_ERR_INVALID_ARG, "vfi_gp_mix: bad sizes");
    if (count % 4 == 0 && f_bstride % 4 == 0 && r_bstride % 4 == 0 && e_bstride % 4 == 0 && h_bstride % 4 == 0 &&
        aligned16(fake) && aligned16(real) && aligned16(eps) && aligned16(hat))
        LAUNCH_1D(gp_mix_kernel<float4>, (long long)N * count / 4, stream, reinterpret_cast<const float4 *>(fake), f_bstride / 4,
                  reinterpret_cast<const float4 *>(real), r_bstride / 4, reinterpret_cast<const float4 *>(eps), e_bstride / 4,
                  reinterpret_cast<float4 *>(hat), h_bstride / 4, N, count / 4);
    else
        LAUNCH_1D(gp_mix_kernel<float>, (long long)N * count, stream, fake, f_bstride, real, r_bstride, eps, e_bstride, hat,
                  h_bstride, N, count);
    return vfi::check_launch("vfi_gp_mix");
}

extern "C" int vfi_grad_penalty_forward(const float *g, long long g_bstride, float *norms, float *value, int B, long long n,
                                        float weight, vfi_stream_t stream) {
    VFI_REQUIRE(g && norms && value, VFI_ERR_INVALID_ARG, "vfi_grad_penalty_forward: null pointer");
    VFI_REQUIRE(B > 0 && n > 0, VFI_ERR_INVALID_ARG, "vfi_grad_penalty_forward: bad sizes (B = %d, n = %lld)", B, n);
    hipStream_t s = vfi::as_stream(stream);
    if (n % 4 == 0 && g_bstride % 4 == 0 && aligned16(g))
        hipLaunchKernelGGL(grad_norm_kernel<float4>, dim3(B), dim3(kThreads), 0, s, g, g_bstride, norms, n);
    else
        hipLaunchKernelGGL(grad_norm_kernel<float>, dim3(B), dim3(kThreads), 0, s, g, g_bstride, norms, n);
    hipLaunchKernelGGL(grad_penalty_value_kernel, dim3(1), dim3(kThreads), 0, s, norms, B, (float)((double)weight / (double)B), value);
    return vfi::check_launch("vfi_grad_penalty_forward");
}

extern "C" int vfi_grad_penalty_backward(const float *g, long long g_bstride, const float *norms, const float *upstream, float *out,
                                         long long out_bstride, int B, long long n, float weight, vfi_stream_t stream) {
    VFI_REQUIRE(g && norms && upstream && out, VFI_ERR_INVALID_ARG, "vfi_grad_penalty_backward: null pointer");
    VFI_REQUIRE(B > 0 && n > 0, VFI_ERR_INVALID_ARG, "vfi_grad_penalty_backward: bad sizes (B = %d, n = %lld)", B, n);
    VFI_REQUIRE(B <= 65535, VFI_ERR_UNSUPPORTED, "vfi_grad_penalty_backward: B = %d beyond the grid", B);
    hipStream_t s = vfi::as_stream(stream);
    const double f = 2.0 * (double)weight / (double)B;
    if (n % 4 == 0 && g_bstride % 4 == 0 && out_bstride % 4 == 0 && aligned16(g) && aligned16(out)) {
        const dim3 grid(vfi::blocks_1d(n / 4), B);
        hipLaunchKernelGGL(grad_penalty_backward_kernel<float4>, grid, dim3(kThreads), 0, s, reinterpret_cast<const float4 *>(g),
                           g_bstride / 4, norms, upstream, reinterpret_cast<float4 *>(out), out_bstride / 4, n / 4, f);
    } else {
        const dim3 grid(vfi::blocks_1d(n), B);
        hipLaunchKernelGGL(grad_penalty_backward_kernel<float>, grid, dim3(kThreads), 0, s, g, g_bstride, norms, upstream, out,
                           out_bstride, n, f);
    }
    return vfi::check_launch("vfi_grad_penalty_backward");
}

extern "C" int vfi_phase_split(const float *x, long long x_bstride, float *xs, long long xs_bstride, int N, int C, int H, int W,
                               vfi_stream_t stream) {
    return launch_phase<false>(x, x_bstride, xs, xs_bstride, N, C, H, W, stream, "vfi_phase_split");
}

extern "C" int vfi_phase_merge(const float *gs, long long gs_bstride, float *gx, long long gx_bstride, int N, int C, int H, int W,
                               vfi_stream_t stream) {
    return launch_phase<true>(gs, gs_bstride, gx, gx_bstride, N, C, H, W, stream, "vfi_phase_merge");
}

extern "C" int vfi_linear_forward(const float *x, const float *w, const float *bias, float *y, int B, int K, int J, float slope,
                                  vfi_stream_t stream) {
    VFI_REQUIRE(x && w && y, VFI_ERR_INVALID_ARG, "vfi_linear_forward: null pointer");
    VFI_REQUIRE(B >= 1 && K >= 1 && J >= 1, VFI_ERR_INVALID_ARG, "vfi_linear_forward: bad sizes (B = %d, K = %d, J = %d)", B, K, J);
    VFI_REQUIRE(slope > 0.0f, VFI_ERR_INVALID_ARG, "vfi_linear_forward: slope %g (must be positive; 1 = no activation)", (double)slope);
    const int gx = vfi::ceil_div(J, kLinRows), gy = vfi::ceil_div(B, kLinBatch);
    VFI_REQUIRE(gy <= 65535, VFI_ERR_UNSUPPORTED, "vfi_linear_forward: B = %d beyond the grid", B);
    const dim3 grid(gx, gy);
    hipStream_t s = vfi::as_stream(stream);
    if (K % 4 == 0 && aligned16(x) && aligned16(w))
        hipLaunchKernelGGL(linear_forward_kernel<float4>, grid, dim3(kThreads), 0, s, x, w, bias, y, B, K, J, slope);
    else
        hipLaunchKernelGGL(linear_forward_kernel<float>, grid, dim3(kThreads), 0, s, x, w, bias, y, B, K, J, slope);
    return vfi::check_launch("vfi_linear_forward");
}

extern "C" int vfi_linear_backward(const float *x, const float *w, const float *y, float slope, const float *g, float *dx, float *dw,
                                   float *dbias, int B, int K, int J, vfi_stream_t stream) {
    VFI_REQUIRE(g && (dx || dw || dbias), VFI_ERR_INVALID_ARG, "vfi_linear_backward: null pointer (g, or every output)");
    VFI_REQUIRE((!dx || w) && (!dw || x), VFI_ERR_INVALID_ARG, "vfi_linear_backward: dx needs w, dw needs x");
    VFI_REQUIRE(B >= 1 && K >= 1 && J >= 1, VFI_ERR_INVALID_ARG, "vfi_linear_backward: bad sizes (B = %d, K = %d, J = %d)", B, K, J);
    VFI_REQUIRE(slope > 0.0f, VFI_ERR_INVALID_ARG, "vfi_linear_backward: slope %g (must be positive; 1 = no activation)", (double)slope);
    VFI_REQUIRE(slope == 1.0f || y, VFI_ERR_INVALID_ARG, "vfi_linear_backward: a slope other than 1 needs the output y");
    const bool v4 = K % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(dx) && aligned16(dw);
    hipStream_t s = vfi::as_stream(stream);
    const float *ym = slope == 1.0f ? nullptr : y;
    if (v4) launch_linear_backward<float4>(x, w, ym, slope, g, dx, dw, dbias, B, K, J, s);
    else launch_linear_backward<float>(x, w, ym, slope, g, dx, dw, dbias, B, K, J, s);
    return vfi::check_launch("vfi_linear_backward");
}
