// PhaseNet's band level, from the block's 64 feature planes to the next level's block input, in one pass over HBM
// (phase_net.py:138-168 + reverse_normalize :80-90): the 64 -> 8 prediction map with tanh, the level's outputs (phase,
// amplitude) and the bilinear resize (align_corners=False) of [feature 64 | prediction 8] into the next level's buffer.
// It replaces vfi_phasenet_predict followed by vfi_resize_bilinear, which read the 64 feature planes twice and pass the
// un-resized prediction planes through memory.  Same FMA chain over the channels and same emit arithmetic: the level's outputs
// are theirs to the bit.  Same bilinear expression too, but the compiler contracts it into other multiply-adds here than in
// resize_bilinear_tile_kernel (whose choice differs from element to element), so resized values may differ in the last bit.
#include <cstdlib>

#include "vfi_conv_common.h"
#include "vfi_phasenet_tail.h"

namespace {

using vfi::conv::apply_act;
namespace tl = vfi::tail;

constexpr int kTailCh = 4;                                                       // channel planes per LDS stage
constexpr int kTailQuads = tl::TX / 4, kTailThreads = kTailQuads * tl::TY;       // a thread per four target columns of a row
constexpr int kTailPx = (tl::MAX_ROWS * tl::MAX_COLS + kTailThreads - 1) / kTailThreads;   // window pixels per thread (5)
constexpr int kTailStride = tl::MAX_COLS + 2, kTailPlane = tl::MAX_ROWS * kTailStride;
constexpr int kTailStages = 64 / kTailCh;

// A workgroup owns one TY x TX tile of the target (vfi_phasenet_tail.h) and walks the 64 channels, kTailCh at a time, through
// two LDS buffers: while the planes of stage s are resized out of one buffer, the loads of stage s + 1 are in flight; they are
// then added into the 8 accumulators of each window pixel the thread holds and stored into the other buffer.  One barrier per
// stage.  The 8 prediction maps then take the same route as two more stages, and the pixels the tile owns emit the level's
// outputs.  VEC: target rows are 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(kTailThreads) void phasenet_level_tail_kernel(const float *__restrict__ feat, long long feat_bs, const float *__restrict__ wp,
                                                                  const float *__restrict__ bias, const float *__restrict__ amp_in, long long amp_bs,
                                                                  const float *__restrict__ maxv, float *__restrict__ dst, long long dst_bs,
                                                                  float *__restrict__ phase_out, float *__restrict__ amp_out, int Hi, int Wi,
                                                                  int Ho, int Wo) {
    __shared__ float lds[2][kTailCh][kTailPlane];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int X0 = blockIdx.x * tl::TX, Y0 = blockIdx.y * tl::TY;
    const int HW = Hi * Wi;
    const tl::Span sy = tl::tile_span(Y0, tl::TY, Hi, Ho), sx = tl::tile_span(X0, tl::TX, Wi, Wo);
    const int ylo = sy.lo, xlo = sx.lo;
    const int nrows = min(sy.hi - ylo + 1, tl::MAX_ROWS), ncols = min(sx.hi - xlo + 1, tl::MAX_COLS);   // (the host checks the scale)
    const float scale_y = (float)Hi / (float)Ho, scale_x = (float)Wi / (float)Wo;

    // the window pixels of this thread: consecutive threads take consecutive pixels of a window row
    unsigned goff[kTailPx], loff[kTailPx];       // (offsets from uniform bases: 32 bits each)
    unsigned own = 0;
#pragma unroll
    for (int j = 0; j < kTailPx; ++j) {
        const int p = tid + kTailThreads * j, r = p / ncols, q = p - r * ncols;
        const bool valid = r < nrows;
        goff[j] = valid ? (unsigned)((ylo + r) * Wi + xlo + q) : 0u;
        loff[j] = valid ? (unsigned)(r * kTailStride + q) : (unsigned)kTailStride - 1u;      // (a pad column: written by all, read by none)
        if (valid && ylo + r >= sy.own_lo && ylo + r < sy.own_hi && xlo + q >= sx.own_lo && xlo + q < sx.own_hi) own |= 1u << j;
    }

    // the target pixels of this thread: four consecutive columns of one row
    const int xo0 = X0 + 4 * (tid % kTailQuads);
    int x0[4], x1[4];
    float lx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fx = tl::src_coord(scale_x, xo0 + k);
        const int xs = min((int)fx, Wi - 1);
        lx[k] = fx - (float)xs;
        x0[k] = min(xs - xlo, ncols - 1);                    // (the min only binds past the last column, where nothing is stored)
        x1[k] = min(min(xs + 1, Wi - 1) - xlo, ncols - 1);
    }
    const int yo = Y0 + tid / kTailQuads;
    const float fy = tl::src_coord(scale_y, min(yo, Ho - 1));
    const int ys = min((int)fy, Hi - 1);
    const float ly = fy - (float)ys;
    const int t0 = (ys - ylo) * kTailStride, t1 = (min(ys + 1, Hi - 1) - ylo) * kTailStride;
    float *const yn = dst + (size_t)n * dst_bs;

    // resize the kTailCh planes of one LDS buffer into the target planes pl0 ...
    auto put = [&](const float (*buf)[kTailPlane], int pl0) {
        if (xo0 >= Wo || yo >= Ho) return;
#pragma unroll
        for (int i = 0; i < kTailCh; ++i) {
            {
                const float *r0 = buf[i] + t0, *r1 = buf[i] + t1;
                float out[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    out[k] = (1.0f - ly) * ((1.0f - lx[k]) * r0[x0[k]] + lx[k] * r0[x1[k]]) +
                             ly * ((1.0f - lx[k]) * r1[x0[k]] + lx[k] * r1[x1[k]]);
                float *o = yn + ((size_t)(pl0 + i) * Ho + yo) * Wo + xo0;
                if (VEC) {
                    *reinterpret_cast<float4 *>(o) = make_float4(out[0], out[1], out[2], out[3]);
                } else if (xo0 + 3 < Wo) {
                    // rows of a width that is no multiple of four: still one 16-byte store, which needs 4-byte alignment only
                    // (resize_bilinear_tile_kernel's form)
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    const f32x4 v = {out[0], out[1], out[2], out[3]};
                    asm volatile("global_store_dwordx4 %0, %1, off" : : "v"(o), "v"(v) : "memory");
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (xo0 + k < Wo) o[k] = out[k];
                }
            }
        }
    };

    const float *const xp = feat + (size_t)n * feat_bs;
    float acc[kTailPx][8];
#pragma unroll
    for (int j = 0; j < kTailPx; ++j)
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[j][o] = 0.0f;
    float v[kTailCh][kTailPx];

    auto load = [&](int c) {
#pragma unroll
        for (int i = 0; i < kTailCh; ++i)
#pragma unroll
            for (int j = 0; j < kTailPx; ++j) v[i][j] = (xp + (size_t)(c + i) * HW)[goff[j]];
    };
    // ... phasenet_predict_kernel's chain: acc = fmaf(w[c][o], x[c], acc) for c ascending
    auto take = [&](int c, float (*buf)[kTailPlane]) {
#pragma unroll
        for (int i = 0; i < kTailCh; ++i) {
            const float *w = wp + (size_t)(c + i) * 32;
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const float wo = w[o];
#pragma unroll
                for (int j = 0; j < kTailPx; ++j) acc[j][o] = fmaf(wo, v[i][j], acc[j][o]);
            }
#pragma unroll
            for (int j = 0; j < kTailPx; ++j)
                buf[i][loff[j]] = v[i][j];
        }
    };

    load(0);
    take(0, lds[0]);
    __syncthreads();
    for (int s = 0; s < kTailStages + 2; ++s) {
        float (*const next)[kTailPlane] = lds[(s + 1) & 1];
        // (issuing these loads a stage earlier, across the barrier, measured slower: 795 against 630 us at the 1080p level)
        if (s + 1 < kTailStages) load((s + 1) * kTailCh);
        put(lds[s & 1], s * kTailCh);
        if (s + 1 < kTailStages) {
            take((s + 1) * kTailCh, next);
        } else if (s + 1 == kTailStages) {
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const float b = bias ? bias[o] : 0.0f;
#pragma unroll
                for (int j = 0; j < kTailPx; ++j) acc[j][o] = apply_act(acc[j][o] + b, 3);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < kTailPx; ++j)
                    next[i][loff[j]] = acc[j][i];
        } else if (s + 1 == kTailStages + 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < kTailPx; ++j)
                    next[i][loff[j]] = acc[j][4 + i];
        }
        __syncthreads();
    }

    // the level's outputs at the source pixels this tile owns: phasenet_predict_kernel's arithmetic
    const float *ap = amp_in + (size_t)n * amp_bs;
    float *pho = phase_out + (size_t)n * 4 * HW, *amo = amp_out + (size_t)n * 4 * HW;
    const float mx = maxv[n];
#pragma unroll
    for (int j = 0; j < kTailPx; ++j) {
        if (!(own >> j & 1u)) continue;
        const unsigned pix = goff[j];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float a0 = (ap + (size_t)b * HW)[pix], a1 = (ap + (size_t)(4 + b) * HW)[pix];
            const float beta = (acc[j][4 + b] + 1.0f) / 2.0f;
            const float a = fmaf(beta, a1, (1.0f - beta) * a0);
            (pho + (size_t)b * HW)[pix] = acc[j][b] * 3.14159265358979323846f;
            (amo + (size_t)b * HW)[pix] = a * mx;
        }
    }
}

static_assert(kTailCh == 4 && kTailStages * kTailCh == 64, "the 8 prediction maps travel as two stages of four planes");
static_assert(tl::TX % 4 == 0 && kTailThreads % 64 == 0 && kTailThreads <= 1024 && kTailPx <= 32, "every window pixel has a thread; `own` is one word");

// Argument checks shared by the entry point and its query.
int tail_check_args(const char *who, const float *feat, const float *packed_w, const float *amp_in, const float *max_amp, const float *x_next,
                    const float *phase_out, const float *amp_out, int N, int H, int W, int Hout, int Wout) {
    VFI_REQUIRE(feat && packed_w && amp_in && max_amp && x_next && phase_out && amp_out, VFI_ERR_INVALID_ARG, "%s: null pointer", who);
    VFI_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && Hout > 0 && Wout > 0, VFI_ERR_INVALID_ARG, "%s: bad sizes", who);
    const long long HW = (long long)H * W, HWo = (long long)Hout * Wout;
    VFI_REQUIRE(64 * HW < (1ll << 31), VFI_ERR_UNSUPPORTED, "%s: per-sample tensor too large for 32-bit offsets", who);
    VFI_REQUIRE(8 * HW <= 64 * HWo, VFI_ERR_UNSUPPORTED, "%s: target %dx%d too small for source %dx%d", who, Hout, Wout, H, W);
    return VFI_OK;
}

// Which launches a call takes (VFI_TAIL_PATH_*): the one place the rule lives.  The one-pass kernel runs exactly where
// vfi_phasenet_predict streams (its fmaf chain; smaller or odd-sized levels run the matrix-core 1x1 there, other bits), so that
// results never depend on which entry point the caller chose, and only when the target is no smaller than the source along
// either axis (the window of a tile then fits the LDS planes).  Its stores are 16-byte vectors where every target row is
// 16-byte aligned.
int tail_path(const float *feat, long long feat_bstride, const float *amp_in, long long amp_bstride, const float *x_next,
              long long next_bstride, const float *phase_out, const float *amp_out, int H, int W, int Hout, int Wout) {
    static const bool stream1x1 = !(getenv("VFI_CONV_STREAM1X1") && atoi(getenv("VFI_CONV_STREAM1X1")) == 0);
    const long long HW = (long long)H * W;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(amp_in) | reinterpret_cast<uintptr_t>(phase_out) |
                           reinterpret_cast<uintptr_t>(amp_out) | (uintptr_t)(feat_bstride * 4) | (uintptr_t)(amp_bstride * 4) | (uintptr_t)(HW * 4);
    if (!(stream1x1 && HW >= 4096 && (bits & 7u) == 0 && H <= Hout && W <= Wout)) return VFI_TAIL_PATH_TWO_LAUNCHES;
    const bool vec = Wout % 4 == 0 && (reinterpret_cast<uintptr_t>(x_next) & 15u) == 0 && next_bstride % 4 == 0;
    return vec ? VFI_TAIL_PATH_ONE_PASS_VEC : VFI_TAIL_PATH_ONE_PASS;
}

}  // namespace

extern "C" int vfi_phasenet_level_tail_path(const float *feat, long long feat_bstride, const float *packed_w, const float *bias,
                                            const float *amp_in, long long amp_bstride, const float *max_amp, const float *x_next,
                                            long long next_bstride, const float *phase_out, const float *amp_out, int N, int H, int W,
                                            int Hout, int Wout) {
    (void)bias;
    if (const int rc = tail_check_args("vfi_phasenet_level_tail_path", feat, packed_w, amp_in, max_amp, x_next, phase_out, amp_out, N, H, W, Hout, Wout))
        return rc;
    return tail_path(feat, feat_bstride, amp_in, amp_bstride, x_next, next_bstride, phase_out, amp_out, H, W, Hout, Wout);
}

extern "C" int vfi_phasenet_level_tail(const float *feat, long long feat_bstride, const float *packed_w, const float *bias,
                                       const float *amp_in, long long amp_bstride, const float *max_amp, float *x_next,
                                       long long next_bstride, float *phase_out, float *amp_out, int N, int H, int W, int Hout, int Wout,
                                       vfi_stream_t stream) {
    if (const int rc = tail_check_args("vfi_phasenet_level_tail", feat, packed_w, amp_in, max_amp, x_next, phase_out, amp_out, N, H, W, Hout, Wout))
        return rc;
    const long long HWo = (long long)Hout * Wout;
    const int path = tail_path(feat, feat_bstride, amp_in, amp_bstride, x_next, next_bstride, phase_out, amp_out, H, W, Hout, Wout);
    if (path == VFI_TAIL_PATH_TWO_LAUNCHES) {
        // the launches this entry point replaces; the un-resized prediction planes pass through the head of the target's
        // feature planes, which the last launch overwrites
        int rc = vfi_phasenet_predict(feat, feat_bstride, packed_w, bias, amp_in, amp_bstride, max_amp, x_next, next_bstride, phase_out, amp_out, N,
                                      64, H, W, stream);
        if (!rc) rc = vfi_resize_bilinear(x_next, next_bstride, nullptr, 0, x_next + 64 * HWo, next_bstride, N, 8, H, W, Hout, Wout, 0, 0, stream);
        return rc ? rc : vfi_resize_bilinear(feat, feat_bstride, nullptr, 0, x_next, next_bstride, N, 64, H, W, Hout, Wout, 0, 0, stream);
    }
    const bool vec = path == VFI_TAIL_PATH_ONE_PASS_VEC;
    const dim3 grid(vfi::ceil_div(Wout, tl::TX), vfi::ceil_div(Hout, tl::TY), N);
    VFI_REQUIRE(grid.y <= 65535, VFI_ERR_UNSUPPORTED, "vfi_phasenet_level_tail: target of %d rows", Hout);
    hipStream_t s = vfi::as_stream(stream);
    if (vec)
        hipLaunchKernelGGL(phasenet_level_tail_kernel<true>, grid, dim3(kTailThreads), 0, s, feat, feat_bstride, packed_w, bias, amp_in, amp_bstride, max_amp,
                           x_next, next_bstride, phase_out, amp_out, H, W, Hout, Wout);
    else
        hipLaunchKernelGGL(phasenet_level_tail_kernel<false>, grid, dim3(kTailThreads), 0, s, feat, feat_bstride, packed_w, bias, amp_in, amp_bstride, max_amp,
                           x_next, next_bstride, phase_out, amp_out, H, W, Hout, Wout);
    return vfi::check_launch("vfi_phasenet_level_tail");
}
