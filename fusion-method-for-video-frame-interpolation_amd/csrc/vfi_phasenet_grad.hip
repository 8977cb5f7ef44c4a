// Backward of one PhaseNet level (gfx950): the HBM-bound adjoints between the existing convolution gradients
// (vfi_conv_grad.hip).  Differentiates reference src/phase_net/phase_net.py:138-139 (bilinear resize to an arbitrary size),
// :190-200 (ELU, tanh), :113-116 and :155-168 with reverse_normalize :80-98 (the per-level blends; a band level's whole
// head in one pass; :119-121 and :158-162, the second blends of the network of three input images), and
// src/train/loss.py:10-20 (phase loss, L1: AbsTerm over the shared two-stage reduction).  The rules: vfi_grad_common.h;
// fp32 throughout.
#include "vfi_grad_common.h"

namespace {

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

// ---- the same adjoints for the network of three input images (vfi_phasenet_emit_n, vfi_phasenet_emit_low_n) ----------------
// The forward blends twice (phase_net.py:158-162): amp1 = b a[4:8] + (1 - b) a[0:4], amp = fb amp1 + (1 - fb) a[8:12] with
// b = (pred[4:8] + 1) / 2, fb = (pred[8:12] + 1) / 2, so pred is an input here:
// g_pred[0:4] = pi g_phase,  g_pred[4:8] = g_amp max[n] fb (a[4:8] - a[0:4]) / 2,  g_pred[8:12] = g_amp max[n] (amp1 - a[8:12]) / 2.
// One thread per (sample, band, group of VEC pixels); HW and the strides are in floats, HW a multiple of VEC.
template <int VEC> struct GradVec;
template <> struct GradVec<1> { typedef float type; };
template <> struct GradVec<4> { typedef float4 type; };

template <int VEC>
__global__ void emit_fuse_backward_kernel(const float *__restrict__ g_phase, const float *__restrict__ g_amp,
                                          const float *__restrict__ pred, long long pred_bs, const float *__restrict__ amp_in,
                                          long long amp_bs, const float *__restrict__ maxv, float *__restrict__ g_pred,
                                          long long gp_bs, int N, int HW) {
    typedef typename GradVec<VEC>::type vec;
    const int PG = HW / VEC;
    GRID_STRIDE(i, (long long)N * 4 * PG) {
        const int p = (int)(i % PG) * VEC, b = (i / PG) % 4, n = i / ((long long)PG * 4);
        const size_t dense = ((size_t)n * 4 + b) * HW + p;
        float *gp = g_pred + (size_t)n * gp_bs + p;
        vec r0, r1, r2;
        if (g_phase) {
            const vec g = *reinterpret_cast<const vec *>(g_phase + dense);
#pragma unroll
            for (int v = 0; v < VEC; ++v) lane_set(r0, v, lane_get(g, v) * 3.14159265358979323846f);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) lane_set(r0, v, 0.0f);
        }
        if (g_amp) {
            const float *am = amp_in + (size_t)n * amp_bs + p, *pr = pred + (size_t)n * pred_bs + p;
            const vec g = *reinterpret_cast<const vec *>(g_amp + dense);
            const vec a0 = *reinterpret_cast<const vec *>(am + (size_t)b * HW), a1 = *reinterpret_cast<const vec *>(am + (size_t)(4 + b) * HW);
            const vec a2 = *reinterpret_cast<const vec *>(am + (size_t)(8 + b) * HW);
            const vec p1 = *reinterpret_cast<const vec *>(pr + (size_t)(4 + b) * HW), p2 = *reinterpret_cast<const vec *>(pr + (size_t)(8 + b) * HW);
            const float mx = maxv[n];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float beta = (lane_get(p1, v) + 1.0f) / 2.0f, fb = (lane_get(p2, v) + 1.0f) / 2.0f;
                const float amp1 = fmaf(beta, lane_get(a1, v), (1.0f - beta) * lane_get(a0, v));      // the forward's own first blend
                const float gm = lane_get(g, v) * mx;
                lane_set(r1, v, gm * fb * (lane_get(a1, v) - lane_get(a0, v)) * 0.5f);
                lane_set(r2, v, gm * (amp1 - lane_get(a2, v)) * 0.5f);
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { lane_set(r1, v, 0.0f); lane_set(r2, v, 0.0f); }
        }
        *reinterpret_cast<vec *>(gp + (size_t)b * HW) = r0;
        *reinterpret_cast<vec *>(gp + (size_t)(4 + b) * HW) = r1;
        *reinterpret_cast<vec *>(gp + (size_t)(8 + b) * HW) = r2;
    }
}
// low1 = a l0 + (1 - a) l1, low = (fa low1 + (1 - fa) l2) max[n], a = (pred[0] + 1) / 2, fa = (pred[1] + 1) / 2:
// g_pred[0] = g max[n] fa (l0 - l1) / 2,  g_pred[1] = g max[n] (low1 - l2) / 2
template <int VEC>
__global__ void emit_low_fuse_backward_kernel(const float *__restrict__ g_low, const float *__restrict__ pred, long long pred_bs,
                                              const float *__restrict__ low, long long low_bs, const float *__restrict__ maxv,
                                              float *__restrict__ g_pred, long long gp_bs, int N, int HW) {
    typedef typename GradVec<VEC>::type vec;
    const int PG = HW / VEC;
    GRID_STRIDE(i, (long long)N * PG) {
        const int p = (int)(i % PG) * VEC, n = i / PG;
        const float *l = low + (size_t)n * low_bs + p, *pr = pred + (size_t)n * pred_bs + p;
        const vec g = *reinterpret_cast<const vec *>(g_low + (size_t)n * HW + p);
        const vec l0 = *reinterpret_cast<const vec *>(l), l1 = *reinterpret_cast<const vec *>(l + HW);
        const vec l2 = *reinterpret_cast<const vec *>(l + (size_t)2 * HW);
        const vec p0 = *reinterpret_cast<const vec *>(pr), p1 = *reinterpret_cast<const vec *>(pr + HW);
        const float mx = maxv[n];
        vec r0, r1;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float alpha = (lane_get(p0, v) + 1.0f) / 2.0f, fa = (lane_get(p1, v) + 1.0f) / 2.0f;
            const float low1 = alpha * lane_get(l0, v) + (1.0f - alpha) * lane_get(l1, v);
            const float gm = lane_get(g, v) * mx;
            lane_set(r0, v, gm * fa * (lane_get(l0, v) - lane_get(l1, v)) * 0.5f);
            lane_set(r1, v, gm * (low1 - lane_get(l2, v)) * 0.5f);
        }
        float *gp = g_pred + (size_t)n * gp_bs + p;
        *reinterpret_cast<vec *>(gp) = r0;
        *reinterpret_cast<vec *>(gp + HW) = r1;
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
                        for (int v = 0; v < VEC; ++v) lane_set(g, v, lane_get(gp, v) * 3.14159265358979323846f);
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) lane_set(g, v, 0.0f);
                    }
                } else {
                    if (a.g_amp) {
                        const float *am = a.amp + (size_t)n * a.amp_bs + q;
                        const vec ga = *reinterpret_cast<const vec *>(a.g_amp + ((size_t)n * 4 + (j - 4)) * HW + q);
                        const vec a1 = *reinterpret_cast<const vec *>(am + (size_t)j * HW);
                        const vec a0 = *reinterpret_cast<const vec *>(am + (size_t)(j - 4) * HW);
                        const float mx = a.maxv[n];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) lane_set(g, v, lane_get(ga, v) * mx * (lane_get(a1, v) - lane_get(a0, v)) * 0.5f);
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) lane_set(g, v, 0.0f);
                    }
                }
                if (a.g_pred) {
                    const vec gi = *reinterpret_cast<const vec *>(a.g_pred + (size_t)n * a.gp_bs + (size_t)j * HW + q);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) lane_set(g, v, lane_get(g, v) + lane_get(gi, v));
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) lane_set(gz, v, lane_get(g, v) * (1.0f - lane_get(y, v) * lane_get(y, v)));
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) lane_set(gz, v, 0.0f);
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
                    for (int v = 0; v < VEC; ++v) lane_set(fv, v, 0.0f);
                    if (valid) fv = *reinterpret_cast<const vec *>(a.f + (size_t)n * a.f_bs + (size_t)k * HW + q);
                    *reinterpret_cast<vec *>(s_f + k * kHeadRow + pg * VEC) = fv;
                }
                if (a.g_f && valid) {
                    const float4 w0 = *reinterpret_cast<const float4 *>(s_w + k * 8), w1 = *reinterpret_cast<const float4 *>(s_w + k * 8 + 4);
                    vec r;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float s = w0.x * lane_get(gz[0], v);
                        s = fmaf(w0.y, lane_get(gz[1], v), s);
                        s = fmaf(w0.z, lane_get(gz[2], v), s);
                        s = fmaf(w0.w, lane_get(gz[3], v), s);
                        s = fmaf(w1.x, lane_get(gz[4], v), s);
                        s = fmaf(w1.y, lane_get(gz[5], v), s);
                        s = fmaf(w1.z, lane_get(gz[6], v), s);
                        s = fmaf(w1.w, lane_get(gz[7], v), s);
                        lane_set(r, v, s);
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

// ---- the head's adjoint for three input images (vfi_phasenet_predict_n: 1x1 64 -> 12, tanh, both blends) --------------------
// head_backward_kernel's sibling with twelve rows: the same block, tiles, phases and orders.  A1 forms gz of 12 rows (the
// emit adjoint is emit_fuse_backward_kernel's), A2 reads a [k][12] weight image as three float4 per k, and in B each of the four
// waves owns three rows of grad_W.  A block partial is grad_W (12, 64) then grad_b (12).
constexpr int kHeadRowsN = 12;
constexpr int kHeadOutN = kHeadRowsN * 64 + kHeadRowsN;
static_assert(kMaxPartials * kHeadOutN <= VFI_PHASENET_HEAD_N_WORKSPACE_FLOATS, "head workspace (three images)");

template <int VEC, bool WGRAD>
__global__ __launch_bounds__(kThreads) void head_backward_fuse_kernel(HeadArgs a) {
    typedef typename HeadVec<VEC>::type vec;
    constexpr int R = kHeadRowsN;
    constexpr int PG = kHeadTile / VEC;         // pixel groups per tile
    constexpr int KPT = 64 / (kThreads / PG);   // feature channels per thread in A2
    __shared__ __attribute__((aligned(16))) float s_f[WGRAD ? 64 * kHeadRow : 4];
    __shared__ __attribute__((aligned(16))) float s_gz[R * kHeadTile];
    __shared__ __attribute__((aligned(16))) float s_w[64 * R];      // [k][j]
    const int t = threadIdx.x;
    for (int i = t; i < 64 * R; i += kThreads) s_w[i] = a.w ? a.w[(i % R) * 64 + i / R] : 0.0f;
    float acc[3] = {0.0f, 0.0f, 0.0f}, accb[3] = {0.0f, 0.0f, 0.0f};
    const int HW = a.HW;
    const long long tiles = (long long)a.N * a.tiles_per_sample;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int n = (int)(tile / a.tiles_per_sample);
        const int px0 = (int)(tile - (long long)n * a.tiles_per_sample) * kHeadTile;
        __syncthreads();        // the previous tile's B has read s_f and s_gz (first tile: s_w is written)
        // A1
        for (int e = t; e < R * PG; e += kThreads) {
            const int j = e / PG, pg = e - j * PG, q = px0 + pg * VEC;
            vec gz;
            if (q < HW) {
                const float *pr = a.pred + (size_t)n * a.pred_bs + q;
                const vec y = *reinterpret_cast<const vec *>(pr + (size_t)j * HW);
                vec g;
#pragma unroll
                for (int v = 0; v < VEC; ++v) lane_set(g, v, 0.0f);
                if (j < 4) {
                    if (a.g_phase) {
                        const vec gp = *reinterpret_cast<const vec *>(a.g_phase + ((size_t)n * 4 + j) * HW + q);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) lane_set(g, v, lane_get(gp, v) * 3.14159265358979323846f);
                    }
                } else if (a.g_amp) {
                    const int b = j & 3;
                    const float *am = a.amp + (size_t)n * a.amp_bs + q;
                    const vec ga = *reinterpret_cast<const vec *>(a.g_amp + ((size_t)n * 4 + b) * HW + q);
                    const vec a0 = *reinterpret_cast<const vec *>(am + (size_t)b * HW);
                    const vec a1 = *reinterpret_cast<const vec *>(am + (size_t)(4 + b) * HW);
                    const float mx = a.maxv[n];
                    if (j < 8) {
                        const vec p2 = *reinterpret_cast<const vec *>(pr + (size_t)(8 + b) * HW);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            const float fb = (lane_get(p2, v) + 1.0f) / 2.0f;
                            lane_set(g, v, lane_get(ga, v) * mx * fb * (lane_get(a1, v) - lane_get(a0, v)) * 0.5f);
                        }
                    } else {
                        const vec p1 = *reinterpret_cast<const vec *>(pr + (size_t)(4 + b) * HW);
                        const vec a2 = *reinterpret_cast<const vec *>(am + (size_t)(8 + b) * HW);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            const float beta = (lane_get(p1, v) + 1.0f) / 2.0f;
                            const float amp1 = fmaf(beta, lane_get(a1, v), (1.0f - beta) * lane_get(a0, v));
                            lane_set(g, v, lane_get(ga, v) * mx * (amp1 - lane_get(a2, v)) * 0.5f);
                        }
                    }
                }
                if (a.g_pred) {
                    const vec gi = *reinterpret_cast<const vec *>(a.g_pred + (size_t)n * a.gp_bs + (size_t)j * HW + q);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) lane_set(g, v, lane_get(g, v) + lane_get(gi, v));
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) lane_set(gz, v, lane_get(g, v) * (1.0f - lane_get(y, v) * lane_get(y, v)));
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) lane_set(gz, v, 0.0f);
            }
            *reinterpret_cast<vec *>(s_gz + j * kHeadTile + pg * VEC) = gz;
        }
        __syncthreads();
        // A2
        {
            const int pg = t % PG, k0 = (t / PG) * KPT, q = px0 + pg * VEC;
            const bool valid = q < HW;
            vec gz[R];
#pragma unroll
            for (int j = 0; j < R; ++j) gz[j] = *reinterpret_cast<const vec *>(s_gz + j * kHeadTile + pg * VEC);
#pragma unroll 4
            for (int kk = 0; kk < KPT; ++kk) {
                const int k = k0 + kk;
                if (WGRAD) {
                    vec fv;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) lane_set(fv, v, 0.0f);
                    if (valid) fv = *reinterpret_cast<const vec *>(a.f + (size_t)n * a.f_bs + (size_t)k * HW + q);
                    *reinterpret_cast<vec *>(s_f + k * kHeadRow + pg * VEC) = fv;
                }
                if (a.g_f && valid) {
                    const float4 *wk = reinterpret_cast<const float4 *>(s_w + k * R);
                    const float4 w0 = wk[0], w1 = wk[1], w2 = wk[2];
                    vec r;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float s = w0.x * lane_get(gz[0], v);
                        s = fmaf(w0.y, lane_get(gz[1], v), s);
                        s = fmaf(w0.z, lane_get(gz[2], v), s);
                        s = fmaf(w0.w, lane_get(gz[3], v), s);
                        s = fmaf(w1.x, lane_get(gz[4], v), s);
                        s = fmaf(w1.y, lane_get(gz[5], v), s);
                        s = fmaf(w1.z, lane_get(gz[6], v), s);
                        s = fmaf(w1.w, lane_get(gz[7], v), s);
                        s = fmaf(w2.x, lane_get(gz[8], v), s);
                        s = fmaf(w2.y, lane_get(gz[9], v), s);
                        s = fmaf(w2.z, lane_get(gz[10], v), s);
                        s = fmaf(w2.w, lane_get(gz[11], v), s);
                        lane_set(r, v, s);
                    }
                    *reinterpret_cast<vec *>(a.g_f + (size_t)n * a.gf_bs + (size_t)k * HW + q) = r;
                }
            }
        }
        if (WGRAD) {
            __syncthreads();
            // B
            const int k = t & 63, j0 = 3 * (t >> 6);
            const float4 *fr = reinterpret_cast<const float4 *>(s_f + k * kHeadRow);
            const float4 *g0 = reinterpret_cast<const float4 *>(s_gz + j0 * kHeadTile);
#pragma unroll 4
            for (int p = 0; p < kHeadTile / 4; ++p) {
                const float4 fv = fr[p];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4 u = g0[r * (kHeadTile / 4) + p];
                    acc[r] = fmaf(u.x, fv.x, acc[r]); acc[r] = fmaf(u.y, fv.y, acc[r]); acc[r] = fmaf(u.z, fv.z, acc[r]); acc[r] = fmaf(u.w, fv.w, acc[r]);
                    accb[r] += u.x; accb[r] += u.y; accb[r] += u.z; accb[r] += u.w;
                }
            }
        }
    }
    if (WGRAD) {
        float *out = a.part + (size_t)blockIdx.x * kHeadOutN;
        const int k = t & 63, j0 = 3 * (t >> 6);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out[(j0 + r) * 64 + k] = acc[r];
            if (k == 0) out[R * 64 + j0 + r] = accb[r];
        }
    }
}

// stage 2 of the twelve-row head (one block), as head_reduce_kernel
__global__ __launch_bounds__(kThreads) void head_reduce_fuse_kernel(const float *__restrict__ part, int blocks, float *__restrict__ g_w,
                                                                    float *__restrict__ g_b) {
    for (int o = threadIdx.x; o < kHeadOutN; o += kThreads) {
        float v = 0.0f;
        for (int b = 0; b < blocks; ++b) v += part[(size_t)b * kHeadOutN + o];
        if (o < kHeadRowsN * 64) { if (g_w) g_w[o] = v; }
        else if (g_b) g_b[o - kHeadRowsN * 64] = v;
    }
}

// ---- batch-statistics BatchNorm (block.py:17, nn.BatchNorm2d in training mode) ----------------------------------------
// A channel's values are N runs of HW floats; as one line of N * HW elements it is cut into bn_blocks_per_channel equal
// chunks (a multiple of 4 floats, so a 16-byte access never straddles two samples), one block each.  The cut depends on
// (N, C, HW) alone and so does every order below.
struct BnCut { int bpc; long long chunk; };
inline BnCut bn_cut(int N, int C, int HW) {
    const long long total = (long long)N * HW;
    long long b = (total + 4095) / 4096;                // at least one unrolled trip of the block per chunk
    const long long cap = VFI_REDUCE_WORKSPACE_FLOATS / (3ll * C);
    b = b > cap ? cap : (b < 1 ? 1 : b);
    BnCut c;
    c.bpc = (int)b;
    c.chunk = ((total + b - 1) / b + 3) / 4 * 4;
    return c;
}

// Chan's merge of (na, ma, M2a) and (nb, mb, M2b); an empty side leaves the other as it is
__device__ __forceinline__ void chan_merge(float &na, float &ma, float &qa, float nb, float mb, float qb) {
    if (nb == 0.0f) return;
    if (na == 0.0f) { na = nb; ma = mb; qa = qb; return; }
    const float n = na + nb, d = mb - ma, r = nb / n;
    ma = fmaf(d, r, ma);
    qa = qa + qb + d * d * na * r;
    na = n;
}

struct Welford {
    float n, m, q;
    // a group of 4: its own mean and M2 in two passes, then Chan's merge; 1 / n from v_rcp_f32 (1 ulp: the weight of a
    // merge, not a term of the variance).  The first group is taken as it is, so a constant channel keeps its value exactly.
    __device__ __forceinline__ void add(const float4 &v) {
        const float gm = ((v.x + v.y) + (v.z + v.w)) * 0.25f;
        const float a = v.x - gm, b = v.y - gm, c = v.z - gm, d = v.w - gm;
        const float gq = (a * a + b * b) + (c * c + d * d);
        const float nn = n + 4.0f, dl = gm - m, r = n == 0.0f ? 1.0f : 4.0f * __builtin_amdgcn_rcpf(nn);
        m = fmaf(dl, r, m);
        q = q + gq + dl * dl * n * r;
        n = nn;
    }
    __device__ __forceinline__ void add(float v) {
        const float nn = n + 1.0f, dl = v - m, r = n == 0.0f ? 1.0f : __builtin_amdgcn_rcpf(nn);
        m = fmaf(dl, r, m);
        q = fmaf(dl * dl * n, r, q);
        n = nn;
    }
};

// Walks elements [e0, e1) of channel c's line in steps of kThreads * L * U per block trip, sample by sample: f(ptr offset)
// is called with the float offset of element (n, p) from the sample's channel base.
template <typename T, typename BODY>
__device__ __forceinline__ void bn_walk(long long e0, long long e1, int HW, BODY body) {
    constexpr int L = sizeof(T) / sizeof(float);
    while (e0 < e1) {
        const int n = (int)(e0 / HW);
        const int p0 = (int)(e0 - (long long)n * HW);
        const long long rest = e1 - e0;
        const int p1 = rest < HW - p0 ? p0 + (int)rest : HW;
#pragma unroll 4
        for (int p = p0 + (int)threadIdx.x * L; p < p1; p += kThreads * L) body(n, p);
        e0 += p1 - p0;
    }
}

// stage 1: block (b, c) writes (count, mean, M2) of its chunk of channel c
template <typename T>
__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(const float *__restrict__ y, long long y_bs, int N, int HW,
                                                                    long long chunk, float *__restrict__ part) {
    __shared__ float lds[3 * kThreads];
    const int c = blockIdx.y, b = blockIdx.x;
    const long long total = (long long)N * HW;
    const long long e0 = (long long)b * chunk, e1 = e0 + chunk < total ? e0 + chunk : total;
    Welford w{0.0f, 0.0f, 0.0f};
    const float *yc = y + (size_t)c * HW;
    bn_walk<T>(e0, e1, HW, [&](int n, int p) { w.add(*reinterpret_cast<const T *>(yc + (size_t)n * y_bs + p)); });
    const int t = threadIdx.x;
    lds[t] = w.n; lds[kThreads + t] = w.m; lds[2 * kThreads + t] = w.q;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) chan_merge(lds[t], lds[kThreads + t], lds[2 * kThreads + t], lds[t + s], lds[kThreads + t + s], lds[2 * kThreads + t + s]);
        __syncthreads();
    }
    if (t == 0) {
        float *o = part + ((size_t)c * gridDim.x + b) * 3;
        o[0] = lds[0]; o[1] = lds[kThreads]; o[2] = lds[2 * kThreads];
    }
}
// stage 2: one block per channel merges its partials in block order
__global__ void bn_stats_final_kernel(const float *__restrict__ part, int bpc, float *__restrict__ mean, float *__restrict__ var) {
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    float n = 0.0f, m = 0.0f, q = 0.0f;
    for (int b = 0; b < bpc; ++b) {
        const float *o = part + ((size_t)c * bpc + b) * 3;
        chan_merge(n, m, q, o[0], o[1], o[2]);
    }
    mean[c] = m;
    var[c] = q / n;
}

__device__ __forceinline__ float bn_elu(float v) { return __builtin_amdgcn_fmed3f(v, __expf(v) - 1.0f, 0.0f); }   // apply_act's ELU
// LeakyReLU(slope) of the discriminator's blocks (vfi_bn_leaky_*): a third instantiation of the kernels below, internal to
// this file -- not a vfi_act value, the public entries vfi_bn_act_* keep refusing everything but none and ELU
constexpr int kActLeaky = 100;

// out = act(scale (y - mean) + beta), scale = gamma / sqrt(var + eps) formed once per block.  (y - mean) first: folded into
// one shift, a channel with |mean| >> sigma would lose its digits in scale * y + shift.  out may be y itself.
template <typename T, int ACT>
__global__ __launch_bounds__(kThreads) void bn_act_forward_kernel(const float *y, long long y_bs, const float *__restrict__ mean,
                                                                  const float *__restrict__ var, const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, float eps, float *out,
                                                                  long long o_bs, int C, int HW, float slope) {
    constexpr int L = sizeof(T) / sizeof(float);
    const int plane = blockIdx.y, n = plane / C, c = plane - n * C;
    const float mu = mean[c], sc = gamma[c] * (1.0f / sqrtf(var[c] + eps)), sh = beta[c];
    const float *yp = y + (size_t)n * y_bs + (size_t)c * HW;
    float *op = out + (size_t)n * o_bs + (size_t)c * HW;
    for (int p = (blockIdx.x * kThreads + threadIdx.x) * L; p < HW; p += gridDim.x * kThreads * L) {
        const T v = *reinterpret_cast<const T *>(yp + p);
        T r;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const float z = fmaf(lane_get(v, l) - mu, sc, sh);
            lane_set(r, l, ACT == VFI_ACT_ELU ? bn_elu(z) : ACT == kActLeaky ? (z > 0.0f ? z : z * slope) : z);
        }
        *reinterpret_cast<T *>(op + p) = r;
    }
}

struct BnBackArgs {
    const float *g_t, *t, *y, *mean, *var, *gamma;
    long long gt_bs, t_bs, y_bs, gy_bs, chunk;
    float *g_y, *g_gamma, *g_beta, *part;
    float eps, slope;
    int N, C, HW, bpc;
};
// g times the activation's derivative, from the output t (LeakyReLU: its sign, slope > 0)
template <int ACT> __device__ __forceinline__ float bn_gz(float g, float t, float slope) {
    return ACT == VFI_ACT_ELU ? (t > 0.0f ? g : g * (t + 1.0f)) : ACT == kActLeaky ? (t > 0.0f ? g : g * slope) : g;
}

// pass 1, stage 1: block (b, c) writes (sum g_z, sum g_z xhat) of its chunk
template <typename T, int ACT>
__global__ __launch_bounds__(kThreads) void bn_back_partial_kernel(BnBackArgs a) {
    constexpr int L = sizeof(T) / sizeof(float);
    __shared__ float lds[2 * kThreads];
    const int c = blockIdx.y, b = blockIdx.x;
    const long long total = (long long)a.N * a.HW;
    const long long e0 = (long long)b * a.chunk, e1 = e0 + a.chunk < total ? e0 + a.chunk : total;
    const float mu = a.mean[c], inv = 1.0f / sqrtf(a.var[c] + a.eps);
    const size_t co = (size_t)c * a.HW;
    float v[2] = {0.0f, 0.0f};
    bn_walk<T>(e0, e1, a.HW, [&](int n, int p) {
        const T g = *reinterpret_cast<const T *>(a.g_t + (size_t)n * a.gt_bs + co + p);
        const T yv = *reinterpret_cast<const T *>(a.y + (size_t)n * a.y_bs + co + p);
        T tv = g;
        if (ACT != VFI_ACT_NONE) tv = *reinterpret_cast<const T *>(a.t + (size_t)n * a.t_bs + co + p);
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const float gz = bn_gz<ACT>(lane_get(g, l), lane_get(tv, l), a.slope);
            s0 += gz;
            s1 = fmaf(gz, (lane_get(yv, l) - mu) * inv, s1);
        }
        v[0] += s0;
        v[1] += s1;
    });
    block_sum<2>(v, lds);
    if (threadIdx.x == 0) {
        float *o = a.part + ((size_t)c * gridDim.x + b) * 2;
        o[0] = v[0]; o[1] = v[1];
    }
}
// pass 1, stage 2: one block per channel sums its partials in block order
__global__ void bn_back_final_kernel(const float *__restrict__ part, int bpc, float *__restrict__ g_gamma, float *__restrict__ g_beta) {
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    float s0 = 0.0f, s1 = 0.0f;
    for (int b = 0; b < bpc; ++b) { s0 += part[((size_t)c * bpc + b) * 2]; s1 += part[((size_t)c * bpc + b) * 2 + 1]; }
    g_beta[c] = s0;
    g_gamma[c] = s1;
}
// pass 2: g_y = gamma inv (g_z - g_beta / n - xhat g_gamma / n); g_y may be g_t itself (every element is read, then
// written, by one thread)
template <typename T, int ACT>
__global__ __launch_bounds__(kThreads) void bn_back_data_kernel(BnBackArgs a) {
    constexpr int L = sizeof(T) / sizeof(float);
    const int plane = blockIdx.y, n = plane / a.C, c = plane - n * a.C;
    const float cnt = (float)((long long)a.N * a.HW);
    const float mu = a.mean[c], inv = 1.0f / sqrtf(a.var[c] + a.eps), k = a.gamma[c] * inv;
    const float mb = a.g_beta[c] / cnt, mg = a.g_gamma[c] / cnt;
    const size_t co = (size_t)c * a.HW;
    const float *gp = a.g_t + (size_t)n * a.gt_bs + co, *yp = a.y + (size_t)n * a.y_bs + co;
    const float *tp = ACT != VFI_ACT_NONE ? a.t + (size_t)n * a.t_bs + co : gp;
    float *op = a.g_y + (size_t)n * a.gy_bs + co;
    for (int p = (blockIdx.x * kThreads + threadIdx.x) * L; p < a.HW; p += gridDim.x * kThreads * L) {
        const T g = *reinterpret_cast<const T *>(gp + p), yv = *reinterpret_cast<const T *>(yp + p);
        T tv = g, r;
        if (ACT != VFI_ACT_NONE) tv = *reinterpret_cast<const T *>(tp + p);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const float gz = bn_gz<ACT>(lane_get(g, l), lane_get(tv, l), a.slope);
            const float xh = (lane_get(yv, l) - mu) * inv;
            lane_set(r, l, k * ((gz - mb) - xh * mg));
        }
        *reinterpret_cast<T *>(op + p) = r;
    }
}

// grid of the two per-plane passes: x over a plane's pixels (up to 64 blocks of one 4-deep trip each), y = N * C planes
inline dim3 bn_plane_grid(int N, int C, int HW, int lanes) {
    long long bx = ((long long)HW + (long long)kThreads * lanes * 4 - 1) / ((long long)kThreads * lanes * 4);
    return dim3((unsigned)(bx > 64 ? 64 : bx), (unsigned)(N * C));
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
    if (act == VFI_ACT_ELU) launch_map<ActGrad<VFI_ACT_ELU>>(grad, g_bstride, y, y_bstride, nullptr, 0, out, out_bstride, N, count, stream);
    else launch_map<ActGrad<VFI_ACT_TANH>>(grad, g_bstride, y, y_bstride, nullptr, 0, out, out_bstride, N, count, stream);
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

extern "C" int vfi_phasenet_emit_n_backward(const float *grad_phase, const float *grad_amp, const float *pred, long long pred_bstride,
                                            const float *amp_in, long long amp_bstride, const float *max_amp, float *grad_pred,
                                            long long gp_bstride, int N, int HW, int num_img, vfi_stream_t stream) {
    VFI_REQUIRE((grad_phase || grad_amp) && grad_pred, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_n_backward: null pointer");
    VFI_REQUIRE(!grad_amp || (amp_in && max_amp), VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_n_backward: amplitudes missing");
    VFI_REQUIRE(N > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_n_backward: bad sizes");
    VFI_REQUIRE(num_img >= 2 && num_img <= 4, VFI_ERR_UNSUPPORTED, "vfi_phasenet_emit_n_backward: num_img %d (2, 3 or 4)", num_img);
    if (num_img != 3) {         // the blend of two images, whatever follows them in amp_in
        LAUNCH_1D(emit_backward_kernel, (long long)N * 4 * HW, stream, grad_phase, grad_amp, amp_in, amp_bstride, max_amp,
                  grad_pred, gp_bstride, N, HW);
        return vfi::check_launch("vfi_phasenet_emit_n_backward");
    }
    VFI_REQUIRE(!grad_amp || pred, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_n_backward: the second blend's adjoint needs pred");
    const bool v4 = HW % 4 == 0 && aligned16(grad_pred) && gp_bstride % 4 == 0 && (!grad_phase || aligned16(grad_phase)) &&
                    (!grad_amp || (aligned16(grad_amp) && aligned16(amp_in) && amp_bstride % 4 == 0 && aligned16(pred) && pred_bstride % 4 == 0));
    if (v4) LAUNCH_1D(emit_fuse_backward_kernel<4>, (long long)N * HW, stream, grad_phase, grad_amp, pred, pred_bstride, amp_in,
                      amp_bstride, max_amp, grad_pred, gp_bstride, N, HW);
    else LAUNCH_1D(emit_fuse_backward_kernel<1>, (long long)N * 4 * HW, stream, grad_phase, grad_amp, pred, pred_bstride, amp_in,
                   amp_bstride, max_amp, grad_pred, gp_bstride, N, HW);
    return vfi::check_launch("vfi_phasenet_emit_n_backward");
}

extern "C" int vfi_phasenet_emit_low_n_backward(const float *grad_low, const float *pred, long long pred_bstride, const float *low_in,
                                                long long low_bstride, const float *max_low, float *grad_pred, long long gp_bstride,
                                                int N, int HW, int num_img, vfi_stream_t stream) {
    VFI_REQUIRE(grad_low && low_in && max_low && grad_pred, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_low_n_backward: null pointer");
    VFI_REQUIRE(N > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_low_n_backward: bad sizes");
    VFI_REQUIRE(num_img >= 2 && num_img <= 4, VFI_ERR_UNSUPPORTED, "vfi_phasenet_emit_low_n_backward: num_img %d (2, 3 or 4)", num_img);
    if (num_img != 3) {
        LAUNCH_1D(emit_low_backward_kernel, (long long)N * HW, stream, grad_low, low_in, low_bstride, max_low, grad_pred,
                  gp_bstride, N, HW);
        return vfi::check_launch("vfi_phasenet_emit_low_n_backward");
    }
    VFI_REQUIRE(pred, VFI_ERR_INVALID_ARG, "vfi_phasenet_emit_low_n_backward: the second blend's adjoint needs pred");
    const bool v4 = HW % 4 == 0 && aligned16(grad_low) && aligned16(pred) && pred_bstride % 4 == 0 && aligned16(low_in) &&
                    low_bstride % 4 == 0 && aligned16(grad_pred) && gp_bstride % 4 == 0;
    if (v4) LAUNCH_1D(emit_low_fuse_backward_kernel<4>, (long long)N * HW / 4, stream, grad_low, pred, pred_bstride, low_in, low_bstride,
                      max_low, grad_pred, gp_bstride, N, HW);
    else LAUNCH_1D(emit_low_fuse_backward_kernel<1>, (long long)N * HW, stream, grad_low, pred, pred_bstride, low_in, low_bstride,
                   max_low, grad_pred, gp_bstride, N, HW);
    return vfi::check_launch("vfi_phasenet_emit_low_n_backward");
}

extern "C" int vfi_phasenet_predict_n_backward(const float *feat, long long feat_bstride, const float *pred, long long pred_bstride,
                                               const float *amp_in, long long amp_bstride, const float *max_amp, const float *weight,
                                               const float *grad_phase, const float *grad_amp, const float *grad_pred_in,
                                               long long gpi_bstride, float *grad_feat, long long gf_bstride, float *grad_weight,
                                               float *grad_bias, float *workspace, int N, int HW, int num_img, vfi_stream_t stream) {
    const bool wgrad = grad_weight || grad_bias;
    VFI_REQUIRE(pred && (grad_feat || wgrad), VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_n_backward: null pointer");
    VFI_REQUIRE(!grad_feat || weight, VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_n_backward: grad_feat needs the weights");
    VFI_REQUIRE(!wgrad || (feat && workspace), VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_n_backward: parameter gradients need feat and a workspace");
    VFI_REQUIRE(!grad_amp || (amp_in && max_amp), VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_n_backward: amplitudes missing");
    VFI_REQUIRE(N > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_phasenet_predict_n_backward: bad sizes");
    VFI_REQUIRE(num_img >= 2 && num_img <= 4, VFI_ERR_UNSUPPORTED, "vfi_phasenet_predict_n_backward: num_img %d (2, 3 or 4)", num_img);
    if (num_img != 3)           // eight predictions, the blend of the first two images: the two-image head's own launches
        return vfi_phasenet_predict_backward(feat, feat_bstride, pred, pred_bstride, amp_in, amp_bstride, max_amp, weight, grad_phase,
                                             grad_amp, grad_pred_in, gpi_bstride, grad_feat, gf_bstride, grad_weight, grad_bias,
                                             workspace, N, HW, stream);
    VFI_REQUIRE(64ll * HW < (1ll << 31), VFI_ERR_UNSUPPORTED, "vfi_phasenet_predict_n_backward: per-sample tensor too large for 32-bit pixel indices");
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
        if (v4) hipLaunchKernelGGL((head_backward_fuse_kernel<4, true>), dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL((head_backward_fuse_kernel<1, true>), dim3(blocks), dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL(head_reduce_fuse_kernel, dim3(1), dim3(kThreads), 0, s, workspace, blocks, grad_weight, grad_bias);
    } else {
        if (v4) hipLaunchKernelGGL((head_backward_fuse_kernel<4, false>), dim3(blocks), dim3(kThreads), 0, s, a);
        else hipLaunchKernelGGL((head_backward_fuse_kernel<1, false>), dim3(blocks), dim3(kThreads), 0, s, a);
    }
    return vfi::check_launch("vfi_phasenet_predict_n_backward");
}

extern "C" int vfi_l1_forward(const float *a, const float *b, long long count, int wrap, float scale, float *workspace,
                              float *out, vfi_stream_t stream) {
    VFI_REQUIRE(a && b && workspace && out, VFI_ERR_INVALID_ARG, "vfi_l1_forward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_l1_forward: bad size");
    const float factor = (float)((double)scale / (double)count);
    if (wrap) return launch_sum_forward(AbsTerm<true>{}, a, b, count, factor, workspace, out, stream, "vfi_l1_forward");
    return launch_sum_forward(AbsTerm<false>{}, a, b, count, factor, workspace, out, stream, "vfi_l1_forward");
}

extern "C" int vfi_l1_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b,
                               long long count, int wrap, float scale, vfi_stream_t stream) {
    VFI_REQUIRE(a && b && upstream && (grad_a || grad_b), VFI_ERR_INVALID_ARG, "vfi_l1_backward: null pointer");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_l1_backward: bad size");
    const float factor = (float)((double)scale / (double)count);
    if (wrap) LAUNCH_1D(sum_backward_kernel<AbsTerm<true>>, count, stream, AbsTerm<true>{}, a, b, upstream, grad_a, grad_b, count, factor);
    else LAUNCH_1D(sum_backward_kernel<AbsTerm<false>>, count, stream, AbsTerm<false>{}, a, b, upstream, grad_a, grad_b, count, factor);
    return vfi::check_launch("vfi_l1_backward");
}

extern "C" int vfi_bn_stats(const float *y, long long y_bstride, int N, int C, int HW, float *mean, float *var, float *workspace,
                            vfi_stream_t stream) {
    VFI_REQUIRE(y && mean && var && workspace, VFI_ERR_INVALID_ARG, "vfi_bn_stats: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && HW > 0, VFI_ERR_INVALID_ARG, "vfi_bn_stats: bad sizes");
    VFI_REQUIRE((long long)N * HW >= 2, VFI_ERR_SHAPE, "vfi_bn_stats: expected more than 1 value per channel (N * HW = %lld)", (long long)N * HW);
    VFI_REQUIRE(C <= 65535 && 3ll * C <= VFI_REDUCE_WORKSPACE_FLOATS && HW < (1 << 30) && (long long)N * HW < (1ll << 40) && (long long)C * HW < (1ll << 40),
                VFI_ERR_UNSUPPORTED, "vfi_bn_stats: C = %d, N * HW = %lld beyond the workspace or the grid", C, (long long)N * HW);
    const BnCut cut = bn_cut(N, C, HW);
    const bool v4 = HW % 4 == 0 && y_bstride % 4 == 0 && aligned16(y);
    hipStream_t s = vfi::as_stream(stream);
    const dim3 grid(cut.bpc, C);
    if (v4) hipLaunchKernelGGL(bn_stats_partial_kernel<float4>, grid, dim3(kThreads), 0, s, y, y_bstride, N, HW, cut.chunk, workspace);
    else hipLaunchKernelGGL(bn_stats_partial_kernel<float>, grid, dim3(kThreads), 0, s, y, y_bstride, N, HW, cut.chunk, workspace);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C), dim3(64), 0, s, workspace, cut.bpc, mean, var);
    return vfi::check_launch("vfi_bn_stats");
}

// act: VFI_ACT_NONE, VFI_ACT_ELU or kActLeaky (slope read by the last alone); `what` names the public entry in messages
static int bn_forward(const char *what, const float *y, long long y_bstride, const float *mean, const float *var, const float *gamma,
                      const float *beta, float eps, int act, float slope, float *out, long long out_bstride, int N, int C, int HW,
                      vfi_stream_t stream) {
    VFI_REQUIRE(y && mean && var && gamma && beta && out, VFI_ERR_INVALID_ARG, "%s: null pointer", what);
    VFI_REQUIRE(N > 0 && C > 0 && HW > 0 && eps >= 0.0f, VFI_ERR_INVALID_ARG, "%s: bad sizes", what);
    VFI_REQUIRE((long long)N * C <= 65535 && HW < (1 << 30), VFI_ERR_UNSUPPORTED, "%s: N * C = %lld planes, HW = %d beyond the grid", what, (long long)N * C, HW);
    const bool v4 = HW % 4 == 0 && y_bstride % 4 == 0 && out_bstride % 4 == 0 && aligned16(y) && aligned16(out);
    hipStream_t s = vfi::as_stream(stream);
    const dim3 grid = bn_plane_grid(N, C, HW, v4 ? 4 : 1);
#define VFI_BN_FWD(T, ACT) \
    hipLaunchKernelGGL((bn_act_forward_kernel<T, ACT>), grid, dim3(kThreads), 0, s, y, y_bstride, mean, var, gamma, beta, eps, out, out_bstride, C, HW, slope)
    if (act == VFI_ACT_ELU) { if (v4) VFI_BN_FWD(float4, VFI_ACT_ELU); else VFI_BN_FWD(float, VFI_ACT_ELU); }
    else if (act == kActLeaky) { if (v4) VFI_BN_FWD(float4, kActLeaky); else VFI_BN_FWD(float, kActLeaky); }
    else { if (v4) VFI_BN_FWD(float4, VFI_ACT_NONE); else VFI_BN_FWD(float, VFI_ACT_NONE); }
#undef VFI_BN_FWD
    return vfi::check_launch(what);
}

extern "C" int vfi_bn_act_forward(const float *y, long long y_bstride, const float *mean, const float *var, const float *gamma,
                                  const float *beta, float eps, int act, float *out, long long out_bstride, int N, int C, int HW,
                                  vfi_stream_t stream) {
    VFI_REQUIRE(y && mean && var && gamma && beta && out, VFI_ERR_INVALID_ARG, "vfi_bn_act_forward: null pointer");
    VFI_REQUIRE(N > 0 && C > 0 && HW > 0 && eps >= 0.0f, VFI_ERR_INVALID_ARG, "vfi_bn_act_forward: bad sizes");
    VFI_REQUIRE(act == VFI_ACT_NONE || act == VFI_ACT_ELU, VFI_ERR_UNSUPPORTED, "vfi_bn_act_forward: act %d (none and ELU only)", act);
    return bn_forward("vfi_bn_act_forward", y, y_bstride, mean, var, gamma, beta, eps, act, 1.0f, out, out_bstride, N, C, HW, stream);
}

extern "C" int vfi_bn_leaky_forward(const float *y, long long y_bstride, const float *mean, const float *var, const float *gamma,
                                    const float *beta, float eps, float slope, float *out, long long out_bstride, int N, int C,
                                    int HW, vfi_stream_t stream) {
    VFI_REQUIRE(slope > 0.0f, VFI_ERR_INVALID_ARG, "vfi_bn_leaky_forward: slope %g (must be positive)", (double)slope);
    return bn_forward("vfi_bn_leaky_forward", y, y_bstride, mean, var, gamma, beta, eps, kActLeaky, slope, out, out_bstride, N, C, HW,
                      stream);
}

static int bn_backward(const char *what, const float *g_t, long long gt_bstride, const float *t, long long t_bstride, const float *y,
                       long long y_bstride, const float *mean, const float *var, const float *gamma, float eps, int act, float slope,
                       float *g_y, long long gy_bstride, float *g_gamma, float *g_beta, float *workspace, int N, int C, int HW,
                       vfi_stream_t stream) {
    VFI_REQUIRE(g_t && y && mean && var && g_gamma && g_beta && workspace, VFI_ERR_INVALID_ARG, "%s: null pointer", what);
    VFI_REQUIRE(act == VFI_ACT_NONE || t, VFI_ERR_INVALID_ARG, "%s: the activation needs its output t", what);
    VFI_REQUIRE(!g_y || gamma, VFI_ERR_INVALID_ARG, "%s: g_y needs gamma", what);
    VFI_REQUIRE(N > 0 && C > 0 && HW > 0 && eps >= 0.0f, VFI_ERR_INVALID_ARG, "%s: bad sizes", what);
    VFI_REQUIRE(C <= 65535 && 3ll * C <= VFI_REDUCE_WORKSPACE_FLOATS && (long long)N * C <= 65535 && HW < (1 << 30) && (long long)N * HW < (1ll << 40) &&
                (long long)C * HW < (1ll << 40), VFI_ERR_UNSUPPORTED, "%s: N = %d, C = %d, HW = %d beyond the workspace or the grid", what, N, C, HW);
    const BnCut cut = bn_cut(N, C, HW);
    BnBackArgs a{};
    a.g_t = g_t; a.t = t; a.y = y; a.mean = mean; a.var = var; a.gamma = gamma; a.gt_bs = gt_bstride; a.t_bs = t_bstride;
    a.y_bs = y_bstride; a.gy_bs = gy_bstride; a.chunk = cut.chunk; a.g_y = g_y; a.g_gamma = g_gamma; a.g_beta = g_beta;
    a.part = workspace; a.eps = eps; a.slope = slope; a.N = N; a.C = C; a.HW = HW; a.bpc = cut.bpc;
    const bool elu = act == VFI_ACT_ELU, leaky = act == kActLeaky;
    const bool v4 = HW % 4 == 0 && gt_bstride % 4 == 0 && y_bstride % 4 == 0 && aligned16(g_t) && aligned16(y) &&
                    (!(elu || leaky) || (t_bstride % 4 == 0 && aligned16(t))) && (!g_y || (gy_bstride % 4 == 0 && aligned16(g_y)));
    hipStream_t s = vfi::as_stream(stream);
    const dim3 rgrid(cut.bpc, C);
    if (elu) { if (v4) hipLaunchKernelGGL((bn_back_partial_kernel<float4, VFI_ACT_ELU>), rgrid, dim3(kThreads), 0, s, a);
               else hipLaunchKernelGGL((bn_back_partial_kernel<float, VFI_ACT_ELU>), rgrid, dim3(kThreads), 0, s, a); }
    else if (leaky) { if (v4) hipLaunchKernelGGL((bn_back_partial_kernel<float4, kActLeaky>), rgrid, dim3(kThreads), 0, s, a);
                      else hipLaunchKernelGGL((bn_back_partial_kernel<float, kActLeaky>), rgrid, dim3(kThreads), 0, s, a); }
    else { if (v4) hipLaunchKernelGGL((bn_back_partial_kernel<float4, VFI_ACT_NONE>), rgrid, dim3(kThreads), 0, s, a);
           else hipLaunchKernelGGL((bn_back_partial_kernel<float, VFI_ACT_NONE>), rgrid, dim3(kThreads), 0, s, a); }
    hipLaunchKernelGGL(bn_back_final_kernel, dim3(C), dim3(64), 0, s, workspace, cut.bpc, g_gamma, g_beta);
    if (g_y) {
        const dim3 grid = bn_plane_grid(N, C, HW, v4 ? 4 : 1);
        if (elu) { if (v4) hipLaunchKernelGGL((bn_back_data_kernel<float4, VFI_ACT_ELU>), grid, dim3(kThreads), 0, s, a);
                   else hipLaunchKernelGGL((bn_back_data_kernel<float, VFI_ACT_ELU>), grid, dim3(kThreads), 0, s, a); }
        else if (leaky) { if (v4) hipLaunchKernelGGL((bn_back_data_kernel<float4, kActLeaky>), grid, dim3(kThreads), 0, s, a);
                          else hipLaunchKernelGGL((bn_back_data_kernel<float, kActLeaky>), grid, dim3(kThreads), 0, s, a); }
        else { if (v4) hipLaunchKernelGGL((bn_back_data_kernel<float4, VFI_ACT_NONE>), grid, dim3(kThreads), 0, s, a);
               else hipLaunchKernelGGL((bn_back_data_kernel<float, VFI_ACT_NONE>), grid, dim3(kThreads), 0, s, a); }
    }
    return vfi::check_launch(what);
}

extern "C" int vfi_bn_act_backward(const float *g_t, long long gt_bstride, const float *t, long long t_bstride, const float *y,
                                   long long y_bstride, const float *mean, const float *var, const float *gamma, float eps, int act,
                                   float *g_y, long long gy_bstride, float *g_gamma, float *g_beta, float *workspace, int N, int C,
                                   int HW, vfi_stream_t stream) {
    VFI_REQUIRE(g_t && y && mean && var && g_gamma && g_beta && workspace, VFI_ERR_INVALID_ARG, "vfi_bn_act_backward: null pointer");
    VFI_REQUIRE(act == VFI_ACT_NONE || act == VFI_ACT_ELU, VFI_ERR_UNSUPPORTED, "vfi_bn_act_backward: act %d (none and ELU only)", act);
    return bn_backward("vfi_bn_act_backward", g_t, gt_bstride, t, t_bstride, y, y_bstride, mean, var, gamma, eps, act, 1.0f, g_y,
                       gy_bstride, g_gamma, g_beta, workspace, N, C, HW, stream);
}

extern "C" int vfi_bn_leaky_backward(const float *g_t, long long gt_bstride, const float *t, long long t_bstride, const float *y,
                                     long long y_bstride, const float *mean, const float *var, const float *gamma, float eps,
                                     float slope, float *g_y, long long gy_bstride, float *g_gamma, float *g_beta, float *workspace,
                                     int N, int C, int HW, vfi_stream_t stream) {
    VFI_REQUIRE(slope > 0.0f, VFI_ERR_INVALID_ARG, "vfi_bn_leaky_backward: slope %g (must be positive)", (double)slope);
    return bn_backward("vfi_bn_leaky_backward", g_t, gt_bstride, t, t_bstride, y, y_bstride, mean, var, gamma, eps, kActLeaky, slope,
                       g_y, gy_bstride, g_gamma, g_beta, workspace, N, C, HW, stream);
}
