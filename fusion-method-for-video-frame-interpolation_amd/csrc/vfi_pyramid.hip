// Complex steerable pyramid (frequency domain, scale_factor-generalised) for gfx950: the kernels and the calls that run on
// a plan.  The plan (spec, mask tables, transform tables, every level's resolved passes) is vfi_pyr_plan.hip; the calls
// here read it through `const` pointers and write its workspace only.
//
// Roofline: HBM (target).  No FFT library is linked: the large levels run on the wave-private register FFT engine of
// vfi_wfft.h (kernels in vfi_pyrw_kernels.h), every length that engine has no configuration for on the generic LDS
// engine of vfi_fft.h (mixed-radix Stockham + Bluestein).  Each pyramid level is two fused kernels per direction, so that
// no intermediate of the reference's op-by-op chain (mask products, crops, shifts, deepcopy, band spectra, band
// coefficients, 2*L*N*4 atan2/abs launches) is materialised except ONE half-transformed array T:
//   analysis  : the low-pass chain of the build is a product of real masks, so every level reads the R2C half spectrum S
//               of the image directly: level k, band b = IFFT2( i * window_k(S) * Q_k[b] ) with the table
//               Q_k[b] = lo0 * prod_{j<k} lomask_j * himask_k * anglemask_b folded at plan time (double precision): the
//               levels do not depend on each other and a level mask simply skips levels;
//               column kernel : (column tile, image, band): window of S (Hermitian half expanded and ifftshift done by
//                               index arithmetic) * Q, inverse column FFT -> T;
//               row kernel    : rows of T -> inverse row FFT -> (phase, amplitude) written straight into the caller's
//                               layout (per-image planes or PhaseNet's concat buffers), optional phase scale;
//   synthesis : row kernel (A cos p, A sin p -> forward row FFT -> T), column kernel (forward column FFT, sum of
//               rotated, masked band spectra + embedded low-pass of the coarser level); levels without bands only embed
//               (pyr_combine_kernel).
//   backward  : vfi_pyr_synthesize_backward, the synthesis' adjoint = the analysis passes with the tables A_k (P_a with the
//               synthesis' two-sided angle masks), the synthesis' 1/(H W), and a gradient epilogue on (phase, amplitude);
//               vfi_pyr_analyze_backward, the analysis' adjoint = the synthesis passes with the tables B_k (the analysis'
//               one-sided angle masks * himask * H W / (h w)) and a gradient prologue on (d phase, d amplitude).
#include "vfi_pyr_plan.h"

#include <cstdlib>
#include <type_traits>
#include <vector>

namespace {

using vfi::blocks_1d;
using vfi::ceil_div;
using namespace vfi::pyr;

// ---- device kernels ------------------------------------------------------------------------------------
using vfi::pyrw::PlaneMap;      // where image d's band-0 plane goes (vfi_pyramid_wave.h)

__device__ __forceinline__ int signed_freq(int u, int h) { return u <= h - h / 2 - 1 ? u : u - h; }

// high-pass half spectrum: hi_half = half * hi0 / (H W) (C2R input: `hi0dft = dft * hi0mask`, real(ifft2) of it)
__global__ __launch_bounds__(256) void pyr_high_kernel(const float2 *__restrict__ half, float2 *__restrict__ hi_half,
                                                       const float *__restrict__ hi0, int N, int H, int W, float inv_hw) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y, wh = W / 2 + 1;
    if (v >= wh) return;
    const float g = hi0[(size_t)u * W + v] * inv_hw;
    for (int n = 0; n < N; ++n) {
        const float2 z = half[((size_t)n * H + u) * wh + v];
        hi_half[((size_t)n * H + u) * wh + v] = make_float2(z.x * g, z.y * g);
    }
}

// low residual spectrum: the (hl x wl) window of the expanded half spectrum * low_gain (unshifted order)
__global__ __launch_bounds__(256) void pyr_low_kernel(const float2 *__restrict__ half, float2 *__restrict__ low,
                                                      const float *__restrict__ gain, int N, int H, int W, int hl, int wl) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= hl * wl) return;
    const int u = e / wl, v = e - u * wl, wh = W / 2 + 1;
    const int fy = signed_freq(u, hl), fx = signed_freq(v, wl);
    const int U = fx < 0 ? (fy > 0 ? H - fy : -fy) : (fy < 0 ? fy + H : fy), V = fx < 0 ? -fx : fx;
    const float g = gain[e];
    for (int n = 0; n < N; ++n) {
        float2 z = half[((size_t)n * H + U) * wh + V];
        if (fx < 0) z.y = -z.y;
        low[(size_t)n * hl * wl + e] = make_float2(z.x * g, z.y * g);
    }
}

// cur = sum_b (-i) * FFT(band_b) * P_s[b]  +  embed(res * lomask)     (reconstruct: orientdft + resdft)
template <int NB>
__global__ __launch_bounds__(256) void pyr_combine_kernel(const float2 *__restrict__ band, const float2 *__restrict__ res,
                                                          float2 *__restrict__ cur, const float *__restrict__ P_s,
                                                          const float *__restrict__ lomask, int N, int h, int w,
                                                          int h2, int w2, int have_bands) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int u = blockIdx.y;
    if (v >= w) return;
    const size_t hw = (size_t)h * w, o = (size_t)u * w + v;
    float ps[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) ps[b] = have_bands ? P_s[(size_t)b * hw + o] : 0.0f;
    const int fy = signed_freq(u, h), fx = signed_freq(v, w);
    const bool inside = fy >= -(h2 / 2) && fy <= h2 - h2 / 2 - 1 && fx >= -(w2 / 2) && fx <= w2 - w2 / 2 - 1;
    const int u2 = fy < 0 ? fy + h2 : fy, v2 = fx < 0 ? fx + w2 : fx;
    const float lom = inside ? lomask[(size_t)u2 * w2 + v2] : 0.0f;
    for (int n = 0; n < N; ++n) {
        float2 acc = make_float2(0.0f, 0.0f);
        if (have_bands) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {  // * (-i) : (re, im) -> (im, -re)
                const float2 z = band[((size_t)n * NB + b) * hw + o];
                acc.x += z.y * ps[b];
                acc.y -= z.x * ps[b];
            }
        }
        if (inside) {
            const float2 r = res[((size_t)n * h2 + u2) * w2 + v2];
            acc.x += r.x * lom;
            acc.y += r.y * lom;
        }
        cur[(size_t)n * hw + o] = acc;
    }
}

// real image -> complex (imag 0) ; complex -> real * scale
__global__ void real_to_complex_kernel(const float *__restrict__ x, float2 *__restrict__ z, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        z[i] = make_float2(x ? x[i] : 0.0f, 0.0f);
}
__global__ void complex_real_kernel(const float2 *__restrict__ z, float *__restrict__ x, long long total, float scale) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        x[i] = z[i].x * scale;
}
// out = cur * lo0 + expand(hi_half) * hi0     (reconstruct: `tempdft * lo0mask + hidft * hi0mask`)
__global__ __launch_bounds__(256) void pyr_final_kernel(float2 *__restrict__ cur, const float2 *__restrict__ hi_half,
                                                        const float *__restrict__ lo0, const float *__restrict__ hi0,
                                                        int N, int h, int w) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int u = blockIdx.y;
    if (v >= w) return;
    const size_t hw = (size_t)h * w, o = (size_t)u * w + v;
    const float l0 = lo0[o], h0 = hi0[o];
    const int wh = w / 2 + 1;
    for (int n = 0; n < N; ++n) {
        float2 z = cur[(size_t)n * hw + o];
        z.x *= l0; z.y *= l0;
        if (hi_half) {
            float2 c;
            if (v < wh) c = hi_half[((size_t)n * h + u) * wh + v];
            else { c = hi_half[((size_t)n * h + (u ? h - u : 0)) * wh + (w - v)]; c.y = -c.y; }
            z.x += c.x * h0; z.y += c.y * h0;
        }
        cur[(size_t)n * hw + o] = z;
    }
}

// a = a * ga + b * gb on half spectra (gains already include 1/(H*W))
__global__ void pyr_gain_pair_kernel(float2 *__restrict__ a, const float2 *__restrict__ b, const float *__restrict__ ga,
                                     const float *__restrict__ gb, int N, long long per_image) {
    const long long total = (long long)N * per_image;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long j = i % per_image;
        const float x = ga[j], y = gb[j];
        const float2 za = a[i], zb = b[i];
        a[i] = make_float2(za.x * x + zb.x * y, za.y * x + zb.y * y);
    }
}

// half spectrum *= gain (already includes 1/(H*W) for the un-normalised C2R)
__global__ void pyr_gain_kernel(float2 *__restrict__ half, const float *__restrict__ gain, int N, long long per_image) {
    const long long total = (long long)N * per_image;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float g = gain[i % per_image];
        float2 z = half[i];
        z.x *= g; z.y *= g;
        half[i] = z;
    }
}

// =====================================================================================================================
// Fused level kernels on the LDS FFT engine (vfi_fft.h): the band spectra and the band coefficients never exist in HBM.
//   analysis  level k :  cols kernel : (tile of columns, image): running low-pass spectrum -> for each band
//                                      i * z * P_a[b] -> inverse column FFT -> T[n][b]   (+ the next level's low-pass;
//                                      level 0 also expands the R2C half spectrum and emits the high-pass half spectrum)
//                        rows kernel : rows of T -> inverse row FFT -> 1/(hw) -> atan2 / hypot -> the caller's planes
//   synthesis level k :  rows kernel : (phase, amplitude) rows -> A cos p, A sin p -> forward row FFT -> T
//                        cols kernel : (tile, image): sum_b (-i) * FFTcol(T[n][b]) * P_s[b] + embedded coarser level
// One intermediate (T: 8 bytes per coefficient written and read once) instead of the five full passes of the op-by-op
// form (band spectrum, 2 x 2 FFT passes, polar).
// =====================================================================================================================
using vfi::fft::Plan1D;
using vfi::fft::kThreads;
using vfi::fft::mul24;

struct LevelColsArgs {
    Plan1D ph;                    // column transform (length h)
    const float2 *src;            // R2C half spectrum of the images, N x H x (W/2+1)
    float2 *T;                    // N x NB x h x w
    const float *P;               // Q_k: [NB][h][w]
    int h, w, H, W, tile;
    int bands_per_pass;           // 1, 2 or 4: how many bands go through ONE transform call as extra lines (small levels)
};

// XCD-aware tile order: workgroup b runs on XCD b % 8 (own L2).  A column tile is only tile*8 bytes wide, so the tiles
// that share 128-byte lines are dealt to the SAME XCD back to back.
__device__ __forceinline__ int tile_of_block(int b, int ntiles) {
    const int per = (ntiles + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}

// Generic-engine form of the analysis column pass (lengths the wave engine has no configuration for; the same
// arithmetic as vfi_pyrw_kernels.h: ana_cols_kernel).
// BLU: the transform length goes through Bluestein (chirp factors in the fill / drain).  A compile-time constant: with a
// run-time flag every fill / drain carries conditional chirp loads, and the compiler then waits for ALL outstanding
// memory operations (vmcnt(0): loads and stores share the counter) in front of every element -- also on the smooth
// levels, the large ones, that never load a chirp factor.
template <int NB, bool BLU>
__device__ __forceinline__ void level_cols_body(const LevelColsArgs &a, const int block_x, const int n) {
    using namespace vfi::fft;
    extern __shared__ float2 buf[];
    const int h = a.h, w = a.w, H = a.H, m = a.ph.m, tid = threadIdx.x, C = a.tile;
    const int ntiles = (w + C - 1) / C;
    const int tile = tile_of_block(block_x, ntiles);
    if (tile >= ntiles) return;
    const int pitch = ((padded_length(m) + 31) & ~31) + (C < 32 ? 32 / C : 1);
    const int v0 = tile * C, lines = w - v0 < C ? w - v0 : C;
    const int shift = __ffs(C) - 1, wh = a.W / 2 + 1;
    constexpr bool blu = BLU;
    const size_t hw = (size_t)h * w;
    const float2 *srcn = a.src + (size_t)n * H * wh;                      // (32-bit offsets inside a plane)
    auto load_z = [&](int u, int v) -> float2 {          // the level's window of the expanded half spectrum at (u, v)
        const int fy = signed_freq(u, h), fx = signed_freq(v, w);
        if (fx >= 0) return srcn[mul24(fy < 0 ? fy + H : fy, wh) + fx];
        float2 z = srcn[mul24(fy > 0 ? H - fy : -fy, wh) - fx];
        z.y = -z.y;
        return z;
    };
    float2 *twl = buf + (size_t)a.bands_per_pass * C * pitch;
    load_twiddles(twl, a.ph);
    // this thread's column of the tile (for_tile): validity, a safe column to read, offset of (row u0, that column)
    const int ccm = tid & (C - 1);
    const bool ccok = ccm < lines;
    const int vt = v0 + (ccok ? ccm : 0), tb = mul24(tid >> shift, w) + vt;
    const int BP = a.bands_per_pass;          // bands per transform call: band bb of a pass occupies lines [bb*C, bb*C + C)
#pragma unroll 1
    for (int b0 = 0; b0 < NB; b0 += BP) {
      for (int bb = 0; bb < BP; ++bb) {
        // fill: conj(i * z * Q[b]) (* chirp): the inverse transform runs as a forward one on conjugated data.  The tile
        // of z is re-read per band (L2) rather than kept in 70 registers across the stage calls.
        const int b = b0 + bb;
        float2 *bufb = buf + mul24(bb * C, pitch);
        const float *Pb = a.P + (size_t)b * hw;
        for_tile(h, shift, pitch,
                 [&](int u, int, int) {
                     Slot s;
                     s.z = load_z(u, vt);
                     s.s = Pb[mul24(u, w) + vt];
                     if (blu) s.c = a.ph.chirp[u];
                     return s;
                 },
                 [&](int, int, int, int idx, const Slot &s) {
                     if (ccok)      // * i : (re, im) -> (-im, re)
                         bufb[idx] = load_value<true>(make_float2(-(s.z.y * s.s), s.z.x * s.s), s.c, blu);
                 });
        if (blu) {
            const int totz = (m - h) * C;
            for (int e = tid; e < totz; e += kThreads) {
                const int u = h + (e >> shift), cc = e & (C - 1);
                if (cc < lines) bufb[cc * pitch + phys(u)] = make_float2(0.0f, 0.0f);
            }
        }
      }
        lds_barrier();
        // (a partial tile leaves unused lines between the bands of a pass: they are transformed too and never stored)
        fft_lines(buf, BP > 1 ? BP * C : lines, pitch, a.ph, twl);
      for (int bb = 0; bb < BP; ++bb) {
        const float2 *bufb = buf + mul24(bb * C, pitch);
        const __amdgpu_buffer_rsrc_t Tr = plane_rsrc(a.T + ((size_t)n * NB + b0 + bb) * hw, hw * sizeof(float2));
        const unsigned tlane = ccok ? (unsigned)tb * 8u : 0xffffffffu;
        for_tile(h, shift, pitch,
                 [&](int u, int, int) {
                     Slot s;
                     if (blu) s.c = a.ph.chirp[u];
                     return s;
                 },
                 [&](int, int, int, int idx, const Slot &s) { return store_value<true>(bufb[idx], s.c, blu); },
                 [&](int, int uq, int, const float2 &o) { plane_store(Tr, tlane, mul24(uq, w) * 8, o); });
      }
        lds_barrier();
    }
}

struct RowsPolarArgs {
    Plan1D pw;                    // row transform (length w)
    float2 *T;                    // planes x h x w
    float *phase, *amp;           // caller's planes (PlaneMap)
    PlaneMap pm;
    long long rows;               // planes * h
    int h, lines;
    float inv_hw, phase_scale;
    unsigned *amp_max;            // analysis only, optional: [groups] bit patterns of the largest amplitude per image group
    int groups;
};
// synthesis adjoint rows (vfi_pyr_synthesize_backward): phase / amp receive d phase / d amplitude, inv_hw = 1 / (H W)
// analysis adjoint rows (vfi_pyr_analyze_backward): phase / amp hold d phase / d amplitude, phase_scale = s, inv_hw = 1 / s
struct RowsPolarGradArgs : RowsPolarArgs {
    const float *fphase, *famp;   // the forward's (phase, amplitude), same layout (PlaneMap)
};
template <bool GRAD> using RowsArgsOf = std::conditional_t<GRAD, RowsPolarGradArgs, RowsPolarArgs>;

template <int NB, bool BLU>
__global__ __launch_bounds__(kThreads, kThreads / 128) void pyr_level_cols_kernel(const LevelColsArgs a) {
    level_cols_body<NB, BLU>(a, blockIdx.x, blockIdx.y);
}
// Several SMALL levels in one launch: below ~135 x 240 a level is a handful of workgroups and a launch costs 16-30 us
// whatever it holds, and the levels of an analysis do not depend on each other.  blockIdx.x runs over the levels' tiles
// (first[i] = first block of entry i), every entry has its own region of T.
constexpr int kMaxMulti = 12;
struct MultiColsArgs {
    LevelColsArgs lev[kMaxMulti];
    int first[kMaxMulti + 1];
    int count;
};
template <int NB, bool BLU>
__global__ __launch_bounds__(kThreads, kThreads / 128) void pyr_multi_level_cols_kernel(const MultiColsArgs ma) {
    int i = 0;
    while (i + 1 < ma.count && (int)blockIdx.x >= ma.first[i + 1]) ++i;      // (uniform)
    level_cols_body<NB, BLU>(ma.lev[i], (int)blockIdx.x - ma.first[i], blockIdx.y);
}

// per-line output base (in elements of h*w planes): plane map applied once per row, not per element
__device__ __forceinline__ void line_bases(size_t *base, int lines, long long row0, int h, int w, const PlaneMap &pm, int NB) {
    for (int l = threadIdx.x; l < lines; l += kThreads) {
        const long long g = row0 + l;
        const int plane = (int)(g / h), y = (int)(g - (long long)plane * h), n = plane / NB, b = plane - n * NB;
        base[l] = (size_t)(pm.idx[n] + b * pm.band_stride) * h * w + (size_t)y * w;
    }
}

__device__ __forceinline__ void zero_row_padding(float2 *buf, int lines, int pitch, int w, int m) {
    using namespace vfi::fft;
    const int pad = m - w, totz = lines * pad;
    const float inv_pad = 1.0f / (float)pad;
    for (int e = threadIdx.x; e < totz; e += kThreads) {
        const int l = fast_div(e, inv_pad), j = w + e - l * pad;
        buf[l * pitch + phys(j)] = make_float2(0.0f, 0.0f);
    }
}

// The walk of the LDS-engine row kernels over `lines` rows of w elements: load(l, j) -> Slot, then use(l, j, LDS index, slot).
// Long rows take the structured walk (no per-element division), short ones the flat one.
template <typename LoadF, typename UseF>
__device__ __forceinline__ void walk_rows(int lines, int w, int pitch, LoadF load, UseF use) {
    using namespace vfi::fft;
    const float inv_w = 1.0f / (float)w;
    if (w >= kThreads)
        for_rows(lines, w, pitch, [&](int l, int j, int) { return load(l, j); },
                 [&](int l, int j, int, int idx, const Slot &s) { use(l, j, idx, s); });
    else
        for_slots(lines * w, [&](int e) { const int l = fast_div(e, inv_w); return load(l, e - mul24(l, w)); },
                  [&](int e, const Slot &s) {
                      const int l = fast_div(e, inv_w), j = e - mul24(l, w);
                      use(l, j, mul24(l, pitch) + phys(j), s);
                  });
}

// rows of T -> inverse row FFT -> (phase, amplitude) or the complex coefficient (coeff_to_values, src/train/pyramid.py:63-69).
// GRAD: the epilogue of the synthesis adjoint instead -- the coefficient gradient G and the forward's (p, A) at the same
// offset give d phase = A (Im G cos p - Re G sin p), d amplitude = Re G cos p + Im G sin p.
template <int NB, bool BLU, bool GRAD = false>
__device__ __forceinline__ void rows_polar_body(const RowsArgsOf<GRAD> &a, const int block_x) {
    using namespace vfi::fft;
    extern __shared__ float2 buf[];
    const int w = a.pw.n, m = a.pw.m, pitch = padded_length(m);
    const long long row0 = (long long)block_x * a.lines;
    const int lines = (int)(a.rows - row0 < a.lines ? a.rows - row0 : a.lines);
    float2 *twl = buf + (size_t)a.lines * pitch;
    size_t *base = reinterpret_cast<size_t *>(twl + a.pw.tw_len);
    load_twiddles(twl, a.pw);
    line_bases(base, lines, row0, a.h, w, a.pm, NB);
    constexpr bool blu = BLU;
    const float2 *Trow = a.T + row0 * w;
    auto fill_load = [&](int l, int j) {
        Slot s;
        s.z = Trow[mul24(l, w) + j];
        if (blu) s.c = a.pw.chirp[j];
        return s;
    };
    auto fill_use = [&](int idx, const Slot &s) { buf[idx] = load_value<true>(s.z, s.c, blu); };
    auto drain_load = [&](int j) {
        Slot s;
        if (blu) s.c = a.pw.chirp[j];
        return s;
    };
    // per-group maximum of the amplitudes this thread writes (groups <= 4: one running value per group)
    float gmax[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool want_max = a.amp_max != nullptr;
    auto drain_use = [&](int l, int j, int idx, const Slot &s) {
        const float2 z = store_value<true>(buf[idx], s.c, blu);
        const float re = z.x * a.inv_hw, im = z.y * a.inv_hw;
        const size_t o = base[l] + j;
        if constexpr (GRAD) {
            float sn, cs;
            sincosf(a.fphase[o], &sn, &cs);      // (as pyr_rows_from_polar_kernel evaluates them for the forward)
            const float am = a.famp[o];
            a.phase[o] = am * (im * cs - re * sn);
            a.amp[o] = re * cs + im * sn;
        } else if (a.pm.complex_coeff) {
            reinterpret_cast<float2 *>(a.phase)[o] = make_float2(re, im);
        } else {
            const float am = sqrtf(re * re + im * im);
            a.phase[o] = atan2f(im, re) * a.phase_scale;
            a.amp[o] = am;
            if (want_max) {
                const int g = (int)(((row0 + l) / a.h) / NB) % a.groups;      // (uniform per line)
#pragma unroll
                for (int t = 0; t < 4; ++t) gmax[t] = t == g ? fmaxf(gmax[t], am) : gmax[t];
            }
        }
    };
    walk_rows(lines, w, pitch, fill_load, [&](int, int, int idx, const Slot &s) { fill_use(idx, s); });
    if (blu) zero_row_padding(buf, lines, pitch, w, m);
    lds_barrier();
    fft_lines(buf, lines, pitch, a.pw, twl);
    walk_rows(lines, w, pitch, [&](int, int j) { return drain_load(j); }, drain_use);
    if (want_max) {        // 64-lane butterfly, then one atomic per wave and group (amplitudes are >= 0: their bit patterns order like the values)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float m = gmax[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if ((threadIdx.x & 63) == 0 && t < a.groups && m > 0.0f) atomicMax(a.amp_max + t, __float_as_uint(m));
        }
    }
}

template <int NB, bool BLU, bool GRAD = false>
__global__ __launch_bounds__(kThreads, kThreads / 128) void pyr_rows_polar_kernel(const RowsArgsOf<GRAD> a) {
    rows_polar_body<NB, BLU, GRAD>(a, blockIdx.x);
}
template <class RA>
struct MultiRowsT {
    RA lev[kMaxMulti];
    int first[kMaxMulti + 1];
    int count;
};
using MultiRowsArgs = MultiRowsT<RowsPolarArgs>;
static_assert(sizeof(MultiRowsT<RowsPolarGradArgs>) <= 4096, "kernel arguments are limited to 4 KiB");
template <int NB, bool BLU, bool GRAD = false>
__global__ __launch_bounds__(kThreads, kThreads / 128) void pyr_multi_rows_polar_kernel(const MultiRowsT<RowsArgsOf<GRAD>> ma) {
    int i = 0;
    while (i + 1 < ma.count && (int)blockIdx.x >= ma.first[i + 1]) ++i;      // (uniform)
    rows_polar_body<NB, BLU, GRAD>(ma.lev[i], (int)blockIdx.x - ma.first[i]);
}

__global__ void pyr_amp_max_finish_kernel(const unsigned *__restrict__ bits, float *__restrict__ out, int count, float eps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = __uint_as_float(bits[i]) + eps;
}

// (phase, amplitude) rows -> complex -> forward row FFT -> T (values_to_coeff, src/train/pyramid.py:99-107, + the row half of
// reconstruct's fft2)
// GRAD: the prologue of the analysis adjoint instead -- the gradients (d phase, d amplitude) and the forward's (p, A) at the
// same offset give the coefficient gradient G = (d A + i s d p / A) e^{i p / s} (s = phase scale); the d p term is dropped
// where A == 0, where the phase has no gradient (atan2 at the origin).
template <int NB, bool BLU, bool GRAD = false>
__global__ __launch_bounds__(kThreads, kThreads / 128) void pyr_rows_from_polar_kernel(const RowsArgsOf<GRAD> a) {
    using namespace vfi::fft;
    extern __shared__ float2 buf[];
    const int w = a.pw.n, m = a.pw.m, pitch = padded_length(m);
    const long long row0 = (long long)blockIdx.x * a.lines;
    const int lines = (int)(a.rows - row0 < a.lines ? a.rows - row0 : a.lines);
    float2 *twl = buf + (size_t)a.lines * pitch;
    size_t *base = reinterpret_cast<size_t *>(twl + a.pw.tw_len);
    load_twiddles(twl, a.pw);
    line_bases(base, lines, row0, a.h, w, a.pm, NB);
    lds_barrier();
    constexpr bool blu = BLU;
    auto fill_load = [&](int l, int j) {
        const size_t o = base[l] + j;
        Slot s;
        if constexpr (GRAD) {      // (the slot's chirp field carries the forward's values: the chirp factor is read at the use)
            s.z = make_float2(a.phase[o], a.amp[o]);
            s.c = make_float2(a.fphase[o], a.famp[o]);
            return s;
        }
        if (a.pm.complex_coeff) s.z = reinterpret_cast<const float2 *>(a.phase)[o];
        else s.z = make_float2(a.phase[o], a.amp[o]);
        if (blu) s.c = a.pw.chirp[j];
        return s;
    };
    auto fill_use = [&](int j, int idx, const Slot &s) {
        if constexpr (GRAD) {
            float sn, cs;
            sincosf(s.c.x * a.inv_hw, &sn, &cs);
            const float t = s.c.y > 0.0f ? a.phase_scale * s.z.x / s.c.y : 0.0f;
            buf[idx] = load_value<false>(make_float2(s.z.y * cs - t * sn, s.z.y * sn + t * cs),
                                         blu ? a.pw.chirp[j] : make_float2(0.0f, 0.0f), blu);
            return;
        }
        float2 x = s.z;
        if (!a.pm.complex_coeff) {
            float sn, cs;
            sincosf(s.z.x, &sn, &cs);
            x = make_float2(cs * s.z.y, sn * s.z.y);
        }
        buf[idx] = load_value<false>(x, s.c, blu);
    };
    float2 *Trow = a.T + row0 * w;
    auto drain_load = [&](int j) {
        Slot s;
        if (blu) s.c = a.pw.chirp[j];
        return s;
    };
    auto drain_use = [&](int l, int j, int idx, const Slot &s) { Trow[mul24(l, w) + j] = store_value<false>(buf[idx], s.c, blu); };
    walk_rows(lines, w, pitch, fill_load, [&](int, int j, int idx, const Slot &s) { fill_use(j, idx, s); });
    if (blu) zero_row_padding(buf, lines, pitch, w, m);
    lds_barrier();
    fft_lines(buf, lines, pitch, a.pw, twl);
    walk_rows(lines, w, pitch, [&](int, int j) { return drain_load(j); }, drain_use);
}

struct CombineColsArgs {
    Plan1D ph;
    const float2 *T;              // N x NB x h x w (row-transformed bands)
    const float2 *res;            // N x h2 x w2 (coarser level's spectrum; may be null)
    float2 *cur;                  // N x h x w
    const float *P, *lomask;
    int h, w, h2, w2, tile;
    int bands_per_pass;
};

// cur = sum_b (-i) * FFTcol(T_b) * P_s[b]  +  embed(res * lomask)     (reconstruct: orientdft + resdft)
template <int NB, bool BLU>
__global__ __launch_bounds__(kThreads, kThreads / 128) void pyr_combine_cols_kernel(const CombineColsArgs a) {
    using namespace vfi::fft;
    extern __shared__ float2 buf[];
    const int h = a.h, w = a.w, m = a.ph.m, tid = threadIdx.x, C = a.tile, n = blockIdx.y;
    const int ntiles = (w + C - 1) / C;
    const int tile = tile_of_block(blockIdx.x, ntiles);
    if (tile >= ntiles) return;
    const int pitch = ((padded_length(m) + 31) & ~31) + (C < 32 ? 32 / C : 1);
    const int v0 = tile * C, lines = w - v0 < C ? w - v0 : C;
    const int shift = __ffs(C) - 1;
    constexpr bool blu = BLU;
    const size_t hw = (size_t)h * w;
    float2 *cur = a.cur + (size_t)n * hw;
    const int BP = a.bands_per_pass;
    float2 *twl = buf + (size_t)BP * C * pitch;
    load_twiddles(twl, a.ph);
    const int ccm = tid & (C - 1);
    const bool ccok = ccm < lines;
    const int vt = v0 + (ccok ? ccm : 0), tb = mul24(tid >> shift, w) + vt;      // (for_tile: this thread's column)
#pragma unroll 1
    for (int b0 = 0; b0 < NB; b0 += BP) {
      for (int bb = 0; bb < BP; ++bb) {
        const float2 *Tb = a.T + ((size_t)n * NB + b0 + bb) * hw;
        float2 *bufb = buf + mul24(bb * C, pitch);
        for_tile(h, shift, pitch,
                 [&](int u, int uq, int) {
                     Slot s;
                     s.z = Tb[tb + mul24(uq, w)];
                     if (blu) s.c = a.ph.chirp[u];
                     return s;
                 },
                 [&](int, int, int, int idx, const Slot &s) {
                     if (ccok) bufb[idx] = load_value<false>(s.z, s.c, blu);
                 });
        if (blu) {
            const int totz = (m - h) * C;
            for (int e = tid; e < totz; e += kThreads) {
                const int u = h + (e >> shift), cc = e & (C - 1);
                if (cc < lines) bufb[cc * pitch + phys(u)] = make_float2(0.0f, 0.0f);
            }
        }
      }
        lds_barrier();
        fft_lines(buf, BP > 1 ? BP * C : lines, pitch, a.ph, twl);
      for (int bb = 0; bb < BP; ++bb) {
        const int b = b0 + bb;
        const float2 *bufb = buf + mul24(bb * C, pitch);
        const float *Pb = a.P + (size_t)b * hw;
        // drain: band 0 starts the sum from the embedded coarser level, bands 1.. add to what this thread wrote for the
        // previous band (its own elements: still in L2)
        for_tile(h, shift, pitch,
                 [&](int u, int uq, int) {
                      const int v = vt, o = tb + mul24(uq, w);
                      Slot s;
                      if (blu) s.c = a.ph.chirp[u];
                      s.s = Pb[o];
                      if (b == 0) {
                          s.z = make_float2(0.0f, 0.0f);
                          if (a.res) {
                              const int h2 = a.h2, w2 = a.w2, fy = signed_freq(u, h), fx = signed_freq(v, w);
                              if (fy >= -(h2 / 2) && fy <= h2 - h2 / 2 - 1 && fx >= -(w2 / 2) && fx <= w2 - w2 / 2 - 1) {
                                  const int u2 = fy < 0 ? fy + h2 : fy, v2 = fx < 0 ? fx + w2 : fx;
                                  const float2 r = a.res[((size_t)n * h2 + u2) * w2 + v2];
                                  const float lom = a.lomask[(size_t)u2 * w2 + v2];
                                  s.z = make_float2(r.x * lom, r.y * lom);
                              }
                          }
                      } else {
                          s.z = cur[o];
                      }
                      return s;
                 },
                 [&](int, int uq, int, int idx, const Slot &s) {
                      if (ccok) {
                          const float2 z = store_value<false>(bufb[idx], s.c, blu);
                          // * (-i) : (re, im) -> (im, -re)
                          cur[tb + mul24(uq, w)] = make_float2(s.z.x + z.y * s.s, s.z.y - z.x * s.s);
                      }
                 });
      }
        lds_barrier();
    }
}

// Launches the smooth or the Bluestein instance of a generic-engine kernel.  > 64 KiB of dynamic LDS needs the attribute,
// per KERNEL (not per signature) and device; it is set once (idempotent: racing threads store the same thing).
template <auto bluestein, auto smooth, class Args>
int launch_engine(bool blu, dim3 grid, size_t lds, hipStream_t s, const Args &a) {
    static bool done[2][vfi::kMaxDevices] = {};
    const auto kernel = blu ? bluestein : smooth;
    bool &d = done[blu][vfi::current_device()];
    if (!d) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(vfi::fft::kLdsElemsMax * sizeof(float2) + 8192));
        if (e != hipSuccess) return vfi::fail(VFI_ERR_LAUNCH, "pyramid: set LDS size: %s", hipGetErrorString(e));
        d = true;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(vfi::fft::kThreads), lds, s, a);
    return VFI_OK;
}

// debugging aid (VFI_PYR_CHECK=1): wait for the stream and count the NaNs of a device array
void debug_scan(const void *dev, size_t floats, hipStream_t s, const char *what, int level) {
    static const bool on = getenv("VFI_PYR_CHECK") != nullptr;
    if (!on) return;
    (void)hipStreamSynchronize(s);
    std::vector<float> host(floats);
    (void)hipMemcpy(host.data(), dev, floats * sizeof(float), hipMemcpyDeviceToHost);
    size_t bad = 0, first = 0;
    for (size_t i = 0; i < floats; ++i)
        if (host[i] != host[i]) { if (!bad) first = i; ++bad; }
    if (bad) fprintf(stderr, "[vfi_pyr check] %s level %d: %zu NaNs of %zu floats, first at %zu\n", what, level, bad, floats, first);
}

// ---- 2-D transforms = a row pass and a column pass, each on the wave engine where the plan resolved a configuration
// for the length, otherwise on the generic LDS engine (vfi_fft.h / vfi_fft.hip) ------------------------------------------
int pass_rows(const Size2D &z, const void *src, void *dst, long long rows, int src_pitch, int dst_pitch, vfi::fft::RowLoad load,
              vfi::fft::RowStore store, bool inverse, hipStream_t s, float scale = 1.0f) {
    using namespace vfi::fft;
    const vfi::pyrw::Tables &tb = z.wave[kWaveRows];
    if (tb.M && rows < (1LL << 31)) {
        vfi::pyrw::GenRowsArgs a{tb, src, dst, (int)rows, src_pitch, dst_pitch, scale};
        return vfi::pyrw::launch_gen_rows(a, (int)load, (int)store, inverse, s);      // (RowLoad / RowStore == GenRowKind values)
    }
    RowArgs r{z.pw, src, dst, rows, src_pitch, dst_pitch, rows_per_group(z.pw, rows), scale};
    return launch_rows(r, load, store, inverse, s);
}
int pass_cols(const Size2D &z, float2 *data, int planes, int cols, int ld, bool inverse, hipStream_t s) {
    using namespace vfi::fft;
    const vfi::pyrw::Tables &tb = z.wave[kWaveAnaCols];      // (the plain column pass runs with the analysis column geometry)
    if (tb.M) {
        vfi::pyrw::GenColsArgs a{tb, data, planes, cols, ld, 1.0f};
        return vfi::pyrw::launch_gen_cols(a, inverse, s);
    }
    ColArgs c{z.ph, data, planes, cols, ld, cols_per_group(z.ph, cols), 1.0f};
    return launch_cols(c, inverse, s);
}

// in-place complex 2-D transform of `planes` dense z.h x z.w arrays (un-normalised, times `scale`)
int fft2d_c2c(const Size2D &z, float2 *data, int planes, bool inverse, hipStream_t s, float scale = 1.0f) {
    const int rc = pass_cols(z, data, planes, z.w, z.w, inverse, s);
    if (rc) return rc;
    return pass_rows(z, data, data, (long long)planes * z.h, z.w, z.w, vfi::fft::kLoadComplex, vfi::fft::kStoreComplex, inverse, s, scale);
}
// real H x W images -> half spectra N x H x (W/2+1)
int fft2d_r2c(const vfi_pyr_plan *p, const float *img, float2 *half, int N, hipStream_t s) {
    const int wh = p->W / 2 + 1;
    const int rc = pass_rows(p->frame, img, half, (long long)N * p->H, p->W, wh, vfi::fft::kLoadReal, vfi::fft::kStoreHalf, false, s);
    if (rc) return rc;
    return pass_cols(p->frame, half, N, wh, wh, false, s);
}
// half spectra (destroyed) -> real images, un-normalised inverse
int fft2d_c2r(const vfi_pyr_plan *p, float2 *half, float *out, int N, hipStream_t s) {
    const int wh = p->W / 2 + 1;
    const int rc = pass_cols(p->frame, half, N, wh, wh, true, s);
    if (rc) return rc;
    return pass_rows(p->frame, half, out, (long long)N * p->H, wh, p->W, vfi::fft::kLoadHalf, vfi::fft::kStoreReal, true, s);
}

// One slice of a call: images [first, first + n) of the call's `total`.  A call of more than the plan's max_images images
// runs as consecutive slices on the plan's one workspace; every slice's map addresses the caller's tensors of the WHOLE
// call (a band-major tensor's bands lie `total` planes apart, and a caller's plane_index has `total` entries per level).
struct Slice {
    int first, n, total;
};

PlaneMap make_map(const int *plane_index, int level, const Slice &sl, int nb, int flags) {
    PlaneMap pm;
    const bool band_major = flags & VFI_PYR_BAND_MAJOR;
    for (int d = 0; d < kMaxImages; ++d) {
        const int g = sl.first + d;
        pm.idx[d] = d < sl.n ? (plane_index ? plane_index[(size_t)level * sl.total + g] : (band_major ? g : g * nb)) : 0;
    }
    pm.band_stride = band_major ? sl.total : 1;
    pm.complex_coeff = (flags & VFI_PYR_COMPLEX_COEFF) ? 1 : 0;
    return pm;
}

// ---- the passes of one level: each takes the engine from the level's record and builds its arguments in one place ------
// generic-engine geometry: column workgroups (tile_of_block deals them in whole groups of 8) and their LDS; rows per
// workgroup of a level's row pass, its workgroups and LDS (the line bases follow the lines)
inline int cols_blocks(const Level &L) { return 8 * ceil_div(ceil_div(L.w, L.tile), 8); }
inline size_t cols_lds(const Level &L) {
    return ((size_t)L.bands * L.tile * vfi::fft::col_pitch(L.ph, L.tile) + L.ph.tw_len) * sizeof(float2);
}
inline int level_row_lines(const Plan1D &pw, long long rows) {
    const int lines = vfi::fft::rows_per_group(pw, rows);
    return lines > 256 ? 256 : lines;
}
inline int rows_blocks(const RowsPolarArgs &ra) { return (int)((ra.rows + ra.lines - 1) / ra.lines); }
inline size_t rows_lds(const RowsPolarArgs &ra) { return vfi::fft::row_lds_bytes(ra.pw, ra.lines, (size_t)ra.lines * sizeof(size_t)); }
// the wave engine's form of a level's row pass (T with the pitch the plan resolved for that direction)
vfi::pyrw::RowsArgs wave_rows_args(const Level &L, int tpitch, int planes, const RowsPolarArgs &g) {
    return vfi::pyrw::RowsArgs{L.wave[kWaveRows], g.T, tpitch, g.phase, g.amp, g.pm, planes, L.h, L.w,
                               g.inv_hw, g.phase_scale, g.amp_max, g.groups};
}

// What vfi_pyr_analyze, vfi_pyr_analyze_max and vfi_pyr_synthesize_backward ask of the analysis passes.
// adjoint: vfi_pyr_synthesize_backward runs them on the synthesis' adjoint: the level tables A_k in place of P_a, the
// 1 / (H W) of the synthesis' final inverse in place of each level's 1 / (h w) (also on the low residual), and with
// (phase, amplitude) the gradient epilogue of the row pass, which reads the forward's values
struct AnalyzeCall {
    float *high;
    float *const *phase, *const *amp;
    const int *plane_index;
    float *low;
    float phase_scale;
    unsigned long long level_mask;
    int flags;
    float *amp_max = nullptr;      // vfi_pyr_analyze_max
    int groups = 1;
    float eps = 0.0f;
    bool adjoint = false;
    const float *const *fphase = nullptr, *const *famp = nullptr;   // forward inputs per level (unused with VFI_PYR_COMPLEX_COEFF)
    Slice slice = {0, 0, 0};       // set by pyr_analyze_impl's walk; high / low already point at the slice's first image
    bool grad() const { return adjoint && !(flags & VFI_PYR_COMPLEX_COEFF); }      // gradient epilogue on (phase, amplitude)
};

LevelColsArgs ana_cols_args(const vfi_pyr_plan *p, int k, const AnalyzeCall &c, float2 *T) {
    const Level &L = p->lev[k];
    return LevelColsArgs{L.ph, p->half0, T, c.adjoint ? L.A : L.P_a, L.h, L.w, p->H, p->W, L.tile, L.bands};
}
RowsPolarGradArgs ana_rows_args(const vfi_pyr_plan *p, int k, int N, const AnalyzeCall &c, float2 *T) {
    const Level &L = p->lev[k];
    const long long rows = (long long)N * p->nbands * L.h;
    return RowsPolarGradArgs{{L.pw, T, c.phase[k], c.amp ? c.amp[k] : nullptr, make_map(c.plane_index, k, c.slice, p->nbands, c.flags), rows, L.h,
                              level_row_lines(L.pw, rows),
                              c.adjoint ? 1.0f / ((float)p->H * (float)p->W) : 1.0f / ((float)L.h * (float)L.w), c.phase_scale,
                              c.amp_max ? p->amp_bits + (size_t)k * c.groups : nullptr, c.groups},
                             c.grad() ? c.fphase[k] : nullptr, c.grad() ? c.famp[k] : nullptr};
}

// ---- the small levels (<= 40 k coefficients per band: from 135 x 240 down at 1080p) as FOUR launches on the generic LDS
// engine instead of two per level: column passes of the smooth / Bluestein heights, row passes of the smooth / Bluestein
// widths; every level has its own region of T.  VFI_PYR_MULTI=0: one launch pair per level (A/B aid)
unsigned long long multi_levels(const vfi_pyr_plan *p, int N, unsigned long long level_mask) {
    static const bool multi_on = !(getenv("VFI_PYR_MULTI") && atoi(getenv("VFI_PYR_MULTI")) == 0);
    // (coarsest first, while their T regions fit into the workspace together: it is sized for ONE level, the finest)
    const size_t cap = (size_t)p->max_images * p->nbands * p->H * p->tpitch_max;
    unsigned long long multi_mask = 0;
    size_t need = 0;
    int cnt = 0;
    for (int k = p->nlev - 1; k >= 0 && cnt < kMaxMulti; --k) {
        if (!((level_mask >> k) & 1ull)) continue;
        const size_t t = (size_t)N * p->nbands * p->lev[k].h * p->lev[k].w;
        if ((long long)p->lev[k].h * p->lev[k].w > 40000 || need + t > cap) break;
        multi_mask |= 1ull << k; need += t; ++cnt;
    }
    return multi_on && cnt >= 2 ? multi_mask : 0;
}
// the small levels' row passes in one launch; g holds the adjoint's form of every entry (sliced to the analysis form for !GRAD)
template <bool GRAD>
int launch_multi_rows(const MultiRowsT<RowsPolarGradArgs> &g, bool blu, size_t lds, hipStream_t s) {
    MultiRowsT<RowsArgsOf<GRAD>> m;
    m.count = g.count;
    for (int i = 0; i <= g.count; ++i) m.first[i] = g.first[i];
    for (int i = 0; i < g.count; ++i) m.lev[i] = g.lev[i];
    return launch_engine<pyr_multi_rows_polar_kernel<4, true, GRAD>, pyr_multi_rows_polar_kernel<4, false, GRAD>>(blu, dim3(m.first[m.count]), lds, s, m);
}
int analyze_multi(const vfi_pyr_plan *p, unsigned long long multi_mask, int N, const AnalyzeCall &c, hipStream_t s) {
    MultiColsArgs mc[2];      // [bluestein]
    MultiRowsT<RowsPolarGradArgs> mr[2];
    size_t clds[2] = {0, 0}, rlds[2] = {0, 0};
    for (int b = 0; b < 2; ++b) { mc[b].count = 0; mc[b].first[0] = 0; mr[b].count = 0; mr[b].first[0] = 0; }
    float2 *T = p->bands;
    for (int k = 0; k < p->nlev; ++k) {
        if (!((multi_mask >> k) & 1ull)) continue;
        const Level &L = p->lev[k];
        MultiColsArgs &cm = mc[L.ph.bluestein ? 1 : 0];
        cm.lev[cm.count] = ana_cols_args(p, k, c, T);
        cm.first[cm.count + 1] = cm.first[cm.count] + cols_blocks(L);
        ++cm.count;
        clds[L.ph.bluestein ? 1 : 0] = std::max(clds[L.ph.bluestein ? 1 : 0], cols_lds(L));
        MultiRowsT<RowsPolarGradArgs> &rm = mr[L.pw.bluestein ? 1 : 0];
        const RowsPolarGradArgs &ra = rm.lev[rm.count] = ana_rows_args(p, k, N, c, T);
        rm.first[rm.count + 1] = rm.first[rm.count] + rows_blocks(ra);
        ++rm.count;
        rlds[L.pw.bluestein ? 1 : 0] = std::max(rlds[L.pw.bluestein ? 1 : 0], rows_lds(ra));
        T += (size_t)N * p->nbands * L.h * L.w;
    }
    int rc = VFI_OK;
    for (int b = 0; b < 2 && !rc; ++b)
        if (mc[b].count)
            rc = launch_engine<pyr_multi_level_cols_kernel<4, true>, pyr_multi_level_cols_kernel<4, false>>(b == 1, dim3(mc[b].first[mc[b].count], N),
                                                                                                            clds[b], s, mc[b]);
    for (int b = 0; b < 2 && !rc; ++b)
        if (mr[b].count) rc = c.grad() ? launch_multi_rows<true>(mr[b], b == 1, rlds[b], s) : launch_multi_rows<false>(mr[b], b == 1, rlds[b], s);
    return rc;
}

int ana_cols(const vfi_pyr_plan *p, int k, int N, const AnalyzeCall &c, hipStream_t s) {
    const Level &L = p->lev[k];
    const LevelColsArgs g = ana_cols_args(p, k, c, p->bands);
    const vfi::pyrw::Tables &tb = L.wave[kWaveAnaCols];
    if (!tb.M)
        return launch_engine<pyr_level_cols_kernel<4, true>, pyr_level_cols_kernel<4, false>>(L.ph.bluestein, dim3(cols_blocks(L), N),
                                                                                              cols_lds(L), s, g);
    vfi::pyrw::AnaColsArgs ca{tb, g.src, p->W / 2 + 1, p->H, g.P, g.T, L.tpitch_ana, N, L.h, L.w};
    const int rc = vfi::pyrw::launch_ana_cols(ca, s);
    if (!rc) debug_scan(p->bands, (size_t)N * p->nbands * L.h * L.tpitch_ana * 2, s, "T after the wave column pass", k);
    return rc;
}

// generic-engine row pass of one level (analysis, or the synthesis adjoint with GRAD)
template <bool GRAD>
int launch_level_rows(const RowsArgsOf<GRAD> &ra, hipStream_t s) {
    return launch_engine<pyr_rows_polar_kernel<4, true, GRAD>, pyr_rows_polar_kernel<4, false, GRAD>>(ra.pw.bluestein, dim3(rows_blocks(ra)),
                                                                                                      rows_lds(ra), s, ra);
}
int ana_rows(const vfi_pyr_plan *p, int k, int N, const AnalyzeCall &c, hipStream_t s) {
    const Level &L = p->lev[k];
    const RowsPolarGradArgs g = ana_rows_args(p, k, N, c, p->bands);
    if (!L.wave[kWaveRows].M) return c.grad() ? launch_level_rows<true>(g, s) : launch_level_rows<false>(g, s);
    const vfi::pyrw::RowsArgs ra = wave_rows_args(L, L.tpitch_ana, N * p->nbands, g);
    return c.grad() ? vfi::pyrw::launch_rows_polar_grad(vfi::pyrw::RowsGradArgs{ra, g.fphase, g.famp}, s) : vfi::pyrw::launch_rows_polar(ra, s);
}

// the analysis passes of one slice (c.slice; N = c.slice.n images from img on)
int analyze_slice(const vfi_pyr_plan *p, const float *img, const AnalyzeCall &c, hipStream_t s) {
    const int N = c.slice.n, H = p->H, W = p->W;
    const float inv_full = 1.0f / ((float)H * (float)W);
    int rc;
    if (c.amp_max && hipMemsetAsync(p->amp_bits, 0, sizeof(unsigned) * p->nlev * c.groups, s) != hipSuccess)
        return vfi::fail(VFI_ERR_LAUNCH, "vfi_pyr_analyze_max: memset");
    if ((rc = fft2d_r2c(p, img, p->half0, N, s))) return rc;
    debug_scan(p->half0, (size_t)N * H * (W / 2 + 1) * 2, s, "half spectrum", -1);
    const unsigned long long multi_mask = multi_levels(p, N, c.level_mask);
    if (multi_mask && (rc = analyze_multi(p, multi_mask, N, c, s))) return rc;
    for (int k = 0; k < p->nlev; ++k) {      // (the levels read the half spectrum directly: nothing to pass along)
        if (!((c.level_mask >> k) & 1ull) || ((multi_mask >> k) & 1ull)) continue;
        if ((rc = ana_cols(p, k, N, c, s)) || (rc = ana_rows(p, k, N, c, s))) return rc;
    }
    if (c.low) {  // low residual: real(ifft2(window(dft) * low_gain))
        float2 *buf = p->lod[0];
        const int tot1 = p->low.h * p->low.w;
        hipLaunchKernelGGL(pyr_low_kernel, dim3(ceil_div(tot1, 256)), dim3(256), 0, s, p->half0, buf, p->low_gain, N, H, W, p->low.h, p->low.w);
        if ((rc = fft2d_c2c(p->low, buf, N, true, s))) return rc;
        const long long tot = (long long)N * tot1;
        hipLaunchKernelGGL(complex_real_kernel, dim3(blocks_1d(tot)), dim3(256), 0, s, buf, c.low, tot,
                           c.adjoint ? inv_full : 1.0f / ((float)p->low.h * (float)p->low.w));
    }
    if (c.high) {  // high residual: C2R of half * hi0 / (H W)
        hipLaunchKernelGGL(pyr_high_kernel, dim3(ceil_div(W / 2 + 1, 256), H), dim3(256), 0, s, p->half0, p->half_hi, p->hi0, N, H, W, inv_full);
        if ((rc = fft2d_c2r(p, p->half_hi, c.high, N, s))) return rc;
    }
    if (c.amp_max) {
        const int count = p->nlev * c.groups;
        hipLaunchKernelGGL(pyr_amp_max_finish_kernel, dim3(ceil_div(count, 64)), dim3(64), 0, s, p->amp_bits, c.amp_max, count, c.eps);
    }
    return VFI_OK;
}

// Any N >= 1: consecutive slices of at most max_images images, the last one shorter, each through analyze_slice on the
// plan's workspace and the caller's stream (stream order keeps a slice off the workspace until the one before is done).
// The amplitude maxima of vfi_pyr_analyze_max are reduced inside one launch, so that form stays within one slice.
int pyr_analyze_impl(const vfi_pyr_plan *p, const float *img, int N, const AnalyzeCall &c, vfi_stream_t stream) {
    VFI_REQUIRE(p && img, VFI_ERR_INVALID_ARG, "vfi_pyr_analyze: null pointer");
    VFI_REQUIRE(!c.amp_max || (c.groups >= 1 && c.groups <= 4 && !(c.flags & VFI_PYR_COMPLEX_COEFF)), VFI_ERR_INVALID_ARG,
                "vfi_pyr_analyze_max: groups must be 1..4 and the outputs (phase, amplitude)");
    VFI_REQUIRE(N >= 1 && (!c.amp_max || N <= p->max_images), VFI_ERR_INVALID_ARG, "vfi_pyr_analyze: N=%d (plan max %d)", N, p->max_images);
    VFI_REQUIRE((c.phase && (c.amp || (c.flags & VFI_PYR_COMPLEX_COEFF))) || c.level_mask == 0, VFI_ERR_INVALID_ARG,
                "vfi_pyr_analyze: null phase/amp tables");
    for (int k = 0; k < p->nlev; ++k) {
        if (!((c.level_mask >> k) & 1ull)) continue;
        VFI_REQUIRE(c.phase[k] && ((c.flags & VFI_PYR_COMPLEX_COEFF) || c.amp[k]), VFI_ERR_INVALID_ARG,
                    "vfi_pyr_analyze: null output for level %d", k);
        VFI_REQUIRE(!c.grad() || (c.fphase[k] && c.famp[k]), VFI_ERR_INVALID_ARG, "vfi_pyr_synthesize_backward: null input for level %d", k);
    }
    hipStream_t s = vfi::as_stream(stream);
    const size_t full = (size_t)p->H * p->W, lowpx = (size_t)p->low.h * p->low.w;
    for (int first = 0; first < N; first += p->max_images) {
        AnalyzeCall sc = c;
        sc.slice = Slice{first, std::min(p->max_images, N - first), N};
        if (c.high) sc.high = c.high + first * full;
        if (c.low) sc.low = c.low + first * lowpx;
        if (const int rc = analyze_slice(p, img + first * full, sc, s)) return rc;
    }
    return vfi::check_launch("vfi_pyr_analyze");
}

// ---- synthesis passes of one level -------------------------------------------------------------------------------------
// a level without bands only embeds the coarser spectrum res (h2 x w2) into cur
void syn_embed(const vfi_pyr_plan *p, int k, int N, const float2 *res, int h2, int w2, float2 *cur, hipStream_t s) {
    const Level &L = p->lev[k];
    hipLaunchKernelGGL((pyr_combine_kernel<4>), dim3(ceil_div(L.w, 256), L.h), dim3(256), 0, s, p->bands, res, cur, L.P_s, L.lomask, N, L.h, L.w,
                       h2, w2, 0);
}
// What vfi_pyr_synthesize and vfi_pyr_analyze_backward ask of the synthesis passes.
// adjoint: vfi_pyr_analyze_backward runs them on the analysis' adjoint: the level tables B_k in place of P_s (they hold the
// H W / (h w) that turns the final 1 / (H W) into each level's 1 / (h w); the low residual gets its own on the way in), and
// with (phase, amplitude) the gradient prologue of the row pass, which reads the forward's values
struct SynthCall {
    const float *high;
    const float *const *phase, *const *amp;       // adjoint: d phase / d amplitude (or G with VFI_PYR_COMPLEX_COEFF)
    const int *plane_index;
    const float *low;
    unsigned long long level_mask;
    int flags;
    bool adjoint = false;
    const float *const *fphase = nullptr, *const *famp = nullptr;   // the forward's outputs per level (unused with VFI_PYR_COMPLEX_COEFF)
    float phase_scale = 1.0f;
    Slice slice = {0, 0, 0};       // set by pyr_synthesize_impl's walk; high / low already point at the slice's first image
    bool grad() const { return adjoint && !(flags & VFI_PYR_COMPLEX_COEFF); }      // gradient prologue on (d phase, d amplitude)
};

int syn_rows(const vfi_pyr_plan *p, int k, int N, const SynthCall &c, hipStream_t s) {
    const Level &L = p->lev[k];
    const long long rows = (long long)N * p->nbands * L.h;
    const bool grad = c.grad();
    const RowsPolarGradArgs g{{L.pw, p->bands, const_cast<float *>(c.phase[k]), const_cast<float *>(c.amp ? c.amp[k] : nullptr),
                               make_map(c.plane_index, k, c.slice, p->nbands, c.flags), rows, L.h, level_row_lines(L.pw, rows),
                               grad ? 1.0f / c.phase_scale : 1.0f, grad ? c.phase_scale : 1.0f, nullptr, 1},
                              grad ? c.fphase[k] : nullptr, grad ? c.famp[k] : nullptr};
    if (L.wave[kWaveRows].M) {
        const vfi::pyrw::RowsArgs ra = wave_rows_args(L, L.tpitch_syn, N * p->nbands, g);
        return grad ? vfi::pyrw::launch_rows_from_polar_grad(vfi::pyrw::RowsGradArgs{ra, g.fphase, g.famp}, s) : vfi::pyrw::launch_rows_from_polar(ra, s);
    }
    if (grad)
        return launch_engine<pyr_rows_from_polar_kernel<4, true, true>, pyr_rows_from_polar_kernel<4, false, true>>(L.pw.bluestein, dim3(rows_blocks(g)),
                                                                                                                rows_lds(g), s, g);
    return launch_engine<pyr_rows_from_polar_kernel<4, true>, pyr_rows_from_polar_kernel<4, false>>(L.pw.bluestein, dim3(rows_blocks(g)),
                                                                                                    rows_lds(g), s, static_cast<const RowsPolarArgs &>(g));
}
// cur = this level's bands + the embedded coarser spectrum res (h2 x w2)
int syn_cols(const vfi_pyr_plan *p, int k, int N, const float *P, const float2 *res, int h2, int w2, float2 *cur, hipStream_t s) {
    const Level &L = p->lev[k];
    const vfi::pyrw::Tables &tb = L.wave[kWaveSynCols];
    if (tb.M) {
        vfi::pyrw::SynColsArgs ca{tb, p->bands, L.tpitch_syn, P, res, L.lomask, cur, N, L.h, L.w, h2, w2};
        return vfi::pyrw::launch_syn_cols(ca, s);
    }
    const CombineColsArgs ca{L.ph, p->bands, res, cur, P, L.lomask, L.h, L.w, h2, w2, L.tile, L.bands};
    return launch_engine<pyr_combine_cols_kernel<4, true>, pyr_combine_cols_kernel<4, false>>(L.ph.bluestein, dim3(cols_blocks(L), N),
                                                                                              cols_lds(L), s, ca);
}

// the synthesis passes of one slice (c.slice; N = c.slice.n images written from img on)
int synthesize_slice(const vfi_pyr_plan *p, const SynthCall &c, float *img, const char *who, hipStream_t s) {
    const int N = c.slice.n, H = p->H, W = p->W;
    int rc;
    // coarsest: res = FFT(low) (zeros when low is NULL); the adjoint's low residual carries 1 / (hL wL) where the final has 1 / (H W)
    float2 *res = p->lod[p->nlev & 1];
    {
        const long long tot = (long long)N * p->low.h * p->low.w;
        hipLaunchKernelGGL(real_to_complex_kernel, dim3(blocks_1d(tot)), dim3(256), 0, s, c.low, res, tot);
        const float scale = c.adjoint ? (float)(((double)H * W) / ((double)p->low.h * p->low.w)) : 1.0f;
        if (c.low && (rc = fft2d_c2c(p->low, res, N, false, s, scale))) return rc;
    }
    for (int k = p->nlev - 1; k >= 0; --k) {
        const Size2D &next = k + 1 < p->nlev ? p->lev[k + 1] : p->low;
        float2 *cur = p->lod[k & 1];
        if (!((c.level_mask >> k) & 1ull)) {
            syn_embed(p, k, N, res, next.h, next.w, cur, s);
        } else {
            VFI_REQUIRE(c.phase[k] && ((c.flags & VFI_PYR_COMPLEX_COEFF) || c.amp[k]), VFI_ERR_INVALID_ARG, "%s: null input for level %d", who, k);
            VFI_REQUIRE(!c.grad() || (c.fphase[k] && c.famp[k]), VFI_ERR_INVALID_ARG, "%s: null forward output for level %d", who, k);
            if ((rc = syn_rows(p, k, N, c, s)) || (rc = syn_cols(p, k, N, c.adjoint ? p->lev[k].B : p->lev[k].P_s, res, next.h, next.w, cur, s)))
                return rc;
        }
        res = cur;
    }
    const float2 *hi_half = nullptr;
    if (c.high) {
        if ((rc = fft2d_r2c(p, c.high, p->half0, N, s))) return rc;
        hi_half = p->half0;
    }
    hipLaunchKernelGGL(pyr_final_kernel, dim3(ceil_div(W, 256), H), dim3(256), 0, s, res, hi_half, p->lo0, p->hi0, N, H, W);
    if ((rc = fft2d_c2c(p->frame, res, N, true, s))) return rc;
    const long long tot = (long long)N * H * W;
    hipLaunchKernelGGL(complex_real_kernel, dim3(blocks_1d(tot)), dim3(256), 0, s, res, img, tot, 1.0f / ((float)H * (float)W));
    return VFI_OK;
}

// any N >= 1, in slices as pyr_analyze_impl
int pyr_synthesize_impl(const vfi_pyr_plan *p, const SynthCall &c, float *img, int N, const char *who, vfi_stream_t stream) {
    VFI_REQUIRE(N >= 1, VFI_ERR_INVALID_ARG, "%s: N=%d", who, N);
    VFI_REQUIRE((c.phase && (c.amp || (c.flags & VFI_PYR_COMPLEX_COEFF))) || c.level_mask == 0, VFI_ERR_INVALID_ARG,
                "%s: null phase/amp tables", who);
    hipStream_t s = vfi::as_stream(stream);
    const size_t full = (size_t)p->H * p->W, lowpx = (size_t)p->low.h * p->low.w;
    for (int first = 0; first < N; first += p->max_images) {
        SynthCall sc = c;
        sc.slice = Slice{first, std::min(p->max_images, N - first), N};
        if (c.high) sc.high = c.high + first * full;
        if (c.low) sc.low = c.low + first * lowpx;
        if (const int rc = synthesize_slice(p, sc, img + first * full, who, s)) return rc;
    }
    return vfi::check_launch(who);
}

}  // namespace

extern "C" int vfi_pyr_apply_filter(vfi_pyr_plan *p, int filter_id, const float *img, int N, float *out, vfi_stream_t stream) {
    VFI_REQUIRE(p && img && out, VFI_ERR_INVALID_ARG, "vfi_pyr_apply_filter: null pointer");
    VFI_REQUIRE(filter_id >= 0 && filter_id < (int)p->filters.size(), VFI_ERR_INVALID_ARG, "vfi_pyr_apply_filter: bad filter id %d", filter_id);
    VFI_REQUIRE(N >= 1, VFI_ERR_INVALID_ARG, "vfi_pyr_apply_filter: N=%d", N);
    hipStream_t s = vfi::as_stream(stream);
    const long long per = (long long)p->H * (p->W / 2 + 1);
    const size_t full = (size_t)p->H * p->W;
    for (int first = 0; first < N; first += p->max_images) {      // slices of max_images images (pyr_analyze_impl)
        const int n = std::min(p->max_images, N - first);
        int rc;
        if ((rc = fft2d_r2c(p, img + first * full, p->half0, n, s))) return rc;
        hipLaunchKernelGGL(pyr_gain_kernel, dim3(blocks_1d(per * n)), dim3(256), 0, s, p->half0, p->filters[filter_id], n, per);
        if ((rc = fft2d_c2r(p, p->half0, out + first * full, n, s))) return rc;
    }
    return vfi::check_launch("vfi_pyr_apply_filter");
}

extern "C" int vfi_pyr_apply_filter_pair(vfi_pyr_plan *p, int filter_a, const float *img_a, int filter_b, const float *img_b,
                                         int N, float *out, vfi_stream_t stream) {
    VFI_REQUIRE(p && img_a && img_b && out, VFI_ERR_INVALID_ARG, "vfi_pyr_apply_filter_pair: null pointer");
    const int nf = (int)p->filters.size();
    VFI_REQUIRE(filter_a >= 0 && filter_a < nf && filter_b >= 0 && filter_b < nf, VFI_ERR_INVALID_ARG,
                "vfi_pyr_apply_filter_pair: bad filter ids %d, %d", filter_a, filter_b);
    VFI_REQUIRE(N >= 1 && p->max_images >= 2, VFI_ERR_INVALID_ARG, "vfi_pyr_apply_filter_pair: N=%d (plan max %d images in all)",
                N, p->max_images);
    hipStream_t s = vfi::as_stream(stream);
    const long long per = (long long)p->H * (p->W / 2 + 1);
    const size_t full = (size_t)p->H * p->W;
    const int cap = p->max_images / 2;      // a slice holds this many images of EACH set
    for (int first = 0; first < N; first += cap) {
        const int n = std::min(cap, N - first);
        int rc;
        if ((rc = fft2d_r2c(p, img_a + first * full, p->half0, n, s)) || (rc = fft2d_r2c(p, img_b + first * full, p->half_hi, n, s))) return rc;
        hipLaunchKernelGGL(pyr_gain_pair_kernel, dim3(blocks_1d(per * n)), dim3(256), 0, s, p->half0, p->half_hi, p->filters[filter_a],
                           p->filters[filter_b], n, per);
        if ((rc = fft2d_c2r(p, p->half0, out + first * full, n, s))) return rc;
    }
    return vfi::check_launch("vfi_pyr_apply_filter_pair");
}

extern "C" int vfi_pyr_plan_multi_levels(const vfi_pyr_plan *p, int N, unsigned long long level_mask, unsigned long long *multi_mask) {
    VFI_REQUIRE(p && multi_mask, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_multi_levels: null pointer");
    VFI_REQUIRE(N >= 1 && N <= p->max_images, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_multi_levels: N=%d (plan max %d)", N, p->max_images);
    *multi_mask = multi_levels(p, N, level_mask);
    return VFI_OK;
}

extern "C" int vfi_pyr_analyze(vfi_pyr_plan *p, const float *img, int N, float *high, float *const *phase,
                               float *const *amp, const int *plane_index, float *low, float phase_scale,
                               unsigned long long level_mask, int flags, vfi_stream_t stream) {
    return pyr_analyze_impl(p, img, N, AnalyzeCall{high, phase, amp, plane_index, low, phase_scale, level_mask, flags}, stream);
}

extern "C" int vfi_pyr_analyze_max(vfi_pyr_plan *p, const float *img, int N, float *high, float *const *phase,
                                   float *const *amp, const int *plane_index, float *low, float phase_scale,
                                   unsigned long long level_mask, int flags, float *amp_max, int groups, float eps,
                                   vfi_stream_t stream) {
    VFI_REQUIRE(amp_max, VFI_ERR_INVALID_ARG, "vfi_pyr_analyze_max: null amp_max");
    AnalyzeCall c{high, phase, amp, plane_index, low, phase_scale, level_mask, flags};
    c.amp_max = amp_max; c.groups = groups; c.eps = eps;
    return pyr_analyze_impl(p, img, N, c, stream);
}

extern "C" int vfi_pyr_synthesize(vfi_pyr_plan *p, const float *high, const float *const *phase, const float *const *amp,
                                  const int *plane_index, const float *low, unsigned long long level_mask, int flags,
                                  float *img, int N, vfi_stream_t stream) {
    VFI_REQUIRE(p && img, VFI_ERR_INVALID_ARG, "vfi_pyr_synthesize: null pointer");
    return pyr_synthesize_impl(p, SynthCall{high, phase, amp, plane_index, low, level_mask, flags}, img, N, "vfi_pyr_synthesize", stream);
}

extern "C" int vfi_pyr_synthesize_backward(vfi_pyr_plan *p, const float *grad_img, int N, const float *const *phase,
                                           const float *const *amp, const int *plane_index, unsigned long long level_mask,
                                           int flags, float *grad_high, float *const *grad_phase, float *const *grad_amp,
                                           float *grad_low, vfi_stream_t stream) {
    VFI_REQUIRE(p && grad_img, VFI_ERR_INVALID_ARG, "vfi_pyr_synthesize_backward: null pointer");
    VFI_REQUIRE(p->adjoint, VFI_ERR_INVALID_ARG, "vfi_pyr_synthesize_backward: call vfi_pyr_plan_prepare_adjoint first");
    VFI_REQUIRE((flags & VFI_PYR_COMPLEX_COEFF) || level_mask == 0 || (phase && amp), VFI_ERR_INVALID_ARG,
                "vfi_pyr_synthesize_backward: null forward phase/amp tables");
    AnalyzeCall c{grad_high, grad_phase, grad_amp, plane_index, grad_low, 1.0f, level_mask, flags};
    c.adjoint = true; c.fphase = phase; c.famp = amp;
    return pyr_analyze_impl(p, grad_img, N, c, stream);
}

extern "C" int vfi_pyr_analyze_backward(vfi_pyr_plan *p, const float *grad_high, const float *const *grad_phase,
                                        const float *const *grad_amp, const float *const *phase, const float *const *amp,
                                        const int *plane_index, const float *grad_low, float phase_scale,
                                        unsigned long long level_mask, int flags, float *grad_img, int N, vfi_stream_t stream) {
    VFI_REQUIRE(p && grad_img, VFI_ERR_INVALID_ARG, "vfi_pyr_analyze_backward: null pointer");
    VFI_REQUIRE(p->analysis_adjoint, VFI_ERR_INVALID_ARG, "vfi_pyr_analyze_backward: call vfi_pyr_plan_prepare_analysis_adjoint first");
    const bool polar = !(flags & VFI_PYR_COMPLEX_COEFF);
    VFI_REQUIRE(!polar || level_mask == 0 || (phase && amp), VFI_ERR_INVALID_ARG, "vfi_pyr_analyze_backward: null forward phase/amp tables");
    VFI_REQUIRE(!polar || (phase_scale != 0.0f && phase_scale == phase_scale), VFI_ERR_INVALID_ARG, "vfi_pyr_analyze_backward: phase_scale %g",
                (double)phase_scale);
    SynthCall c{grad_high, grad_phase, grad_amp, plane_index, grad_low, level_mask, flags};
    c.adjoint = true; c.fphase = phase; c.famp = amp; c.phase_scale = phase_scale;
    return pyr_synthesize_impl(p, c, grad_img, N, "vfi_pyr_analyze_backward", stream);
}
