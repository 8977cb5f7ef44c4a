// Complex steerable pyramid (frequency domain, scale_factor-generalised) for gfx950:
// the arithmetic behind Pyramid.filter / inv_filter (reference call sites src/train/pyramid.py:35-46;
// adapters coeff_to_values / values_to_coeff src/train/pyramid.py:48-112 are fused in).
//
// The reference delegates this arithmetic to the third-party `steerable.SCFpyr_PyTorch` (absent, fork
// unknown: see DESIGN.md, "pyramid spec"); the spec implemented here is the one restated in
// oracle/pyramid_cpu.py: level k works on the centred ceil(H/s^k) x ceil(W/s^k) window of the
// spectrum, radial raised-cosine transition shifted by log2(s) per level, nbands oriented analytic bands.
// This file is the plan: every mask table is precomputed once per plan in double precision on the host and stored in the
// unshifted (FFT-native) index order, so that every table read is coalesced with the spectrum access; and every level's
// passes (transform tables, engine, pitch of T, tiling) are resolved once, here.  The kernels and the calls that run on
// a plan are in vfi_pyramid.hip.  No device code in this file.
#include "vfi_pyr_plan.h"

#include <cmath>
#include <cstdlib>
#include <new>

namespace {

using namespace vfi::pyr;
constexpr double kPi = 3.14159265358979323846;

// ---- host-side mask construction (double precision, numpy semantics) -----------------------------------
double interp(double x, const std::vector<double> &xp, const std::vector<double> &fp) {
    const size_t n = xp.size();
    if (x <= xp[0]) return fp[0];
    if (x >= xp[n - 1]) return fp[n - 1];
    size_t lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    const double slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + fp[lo];
}

std::vector<double> linspace_grid(int m) {  // prepare_grid axis
    std::vector<double> v(m);
    const double start = -(double)(m / 2) / (m / 2.0);
    const double stop = (double)(m / 2) / (m / 2.0) - (1 - m % 2) * 2.0 / m;
    const double step = m > 1 ? (stop - start) / (m - 1) : 0.0;
    for (int i = 0; i < m; ++i) v[i] = start + i * step;
    if (m > 1) v[m - 1] = stop;
    return v;
}

inline int level_size(int d, double s, int k) { return (int)std::ceil(d / std::pow(s, k) - 1e-9); }

template <typename T>
int dev_upload(vfi_pyr_plan *p, const std::vector<T> &host, T **dev) {
    if (hipMalloc((void **)dev, host.size() * sizeof(T)) != hipSuccess) return VFI_ERR_NOMEM;
    p->allocs.push_back(*dev);
    if (hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return VFI_ERR_LAUNCH;
    return VFI_OK;
}

int dev_alloc(vfi_pyr_plan *p, void **dev, size_t bytes) {
    if (hipMalloc(dev, bytes) != hipSuccess) return VFI_ERR_NOMEM;
    p->allocs.push_back(*dev);
    return VFI_OK;
}

// shifted-window index (DC at h/2) for an unshifted index u of a length-h axis
inline int shifted_of(int u, int h) { return (u + h / 2) % h; }

// upstream's angular LUTs: abscissae xc, one-sided analysis mask ya, two-sided synthesis mask ys
void angle_luts(int nb, std::vector<double> &xc, std::vector<double> &ya, std::vector<double> &ys) {
    const int lut = 1024, order = nb - 1;
    const int nl = 3 * lut + 3;
    xc.resize(nl); ya.resize(nl); ys.resize(nl);
    double fact_o = 1, fact_2o = 1;
    for (int i = 2; i <= order; ++i) fact_o *= i;
    for (int i = 2; i <= 2 * order; ++i) fact_2o *= i;
    const double cst = std::pow(2.0, 2 * order) * fact_o * fact_o / (nb * fact_2o);
    for (int i = 0; i < nl; ++i) {
        xc[i] = kPi * (double)(i - (2 * lut + 1)) / lut;
        double alpha = std::fmod(xc[i] + kPi, 2 * kPi);
        if (alpha < 0) alpha += 2 * kPi;
        alpha -= kPi;
        const double c = std::pow(std::cos(xc[i]), order);
        ya[i] = 2.0 * std::sqrt(cst) * c * (std::fabs(alpha) < kPi / 2 ? 1.0 : 0.0);
        ys[i] = std::sqrt(cst) * c;
    }
}

// chain(spos, k) = lo0 * prod_{j<k} lomask_j at the full-grid (shifted) position spos: what the build's running low-pass
// spectrum has been multiplied by when level k reads it (`lodft = dft * lo0mask`, then `lodft * lomask` per level)
struct Chain {
    const vfi_pyr_plan *p;
    std::vector<std::vector<double>> xr_of;       // xr_of[j] = xr0 - j * log2(scale)
    explicit Chain(const vfi_pyr_plan *pl) : p(pl), xr_of(pl->nlev + 1, pl->xr0) {
        const double ls = std::log2(p->scale);
        for (int j = 1; j <= p->nlev; ++j)
            for (auto &x : xr_of[j]) x -= j * ls;
    }
    double operator()(size_t spos, int k) const {
        double c = interp(p->log_rad[spos], xr_of[0], p->yir);
        for (int j = 1; j <= k; ++j) c *= interp(p->log_rad[spos], xr_of[j], p->yir);
        return c;
    }
};

int build_tables(vfi_pyr_plan *p) {
    const int H = p->H, W = p->W, nb = p->nbands;
    const std::vector<double> gy = linspace_grid(H), gx = linspace_grid(W);
    // log_rad / angle on the full shifted grid
    std::vector<double> log_rad((size_t)H * W), angle((size_t)H * W);
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            angle[(size_t)i * W + j] = std::atan2(gy[i], gx[j]);
            log_rad[(size_t)i * W + j] = std::sqrt(gx[j] * gx[j] + gy[i] * gy[i]);
        }
    if (W > 1) log_rad[(size_t)(H / 2) * W + W / 2] = log_rad[(size_t)(H / 2) * W + W / 2 - 1];
    for (auto &v : log_rad) v = std::log2(v);
    // rcosFn(1, -0.5)
    const int n = 256;
    std::vector<double> xr(n + 3), yr(n + 3), yir(n + 3);
    for (int i = 0; i < n + 3; ++i) {
        const double x = kPi * (double)(i - n - 1) / 2.0 / n;
        xr[i] = x;
        yr[i] = std::cos(x) * std::cos(x);
    }
    yr[0] = yr[1];
    yr[n + 2] = yr[n + 1];
    for (int i = 0; i < n + 3; ++i) {
        xr[i] = -0.5 + 2.0 / kPi * (xr[i] + kPi / 4.0);
        yr[i] = std::sqrt(yr[i]);
        yir[i] = std::sqrt(std::fabs(1.0 - yr[i] * yr[i]));
    }
    std::vector<double> xc, ya, ys;
    angle_luts(nb, xc, ya, ys);
    const int nl = (int)xc.size();
    std::vector<double> xcb(nl);
    p->log_rad = log_rad; p->xr0 = xr; p->yr = yr; p->yir = yir;

    std::vector<float> t((size_t)H * W), t2((size_t)H * W);
    for (int u = 0; u < H; ++u)
        for (int v = 0; v < W; ++v) {
            const size_t s = (size_t)shifted_of(u, H) * W + shifted_of(v, W);
            t[(size_t)u * W + v] = (float)interp(log_rad[s], xr, yir);
            t2[(size_t)u * W + v] = (float)interp(log_rad[s], xr, yr);
        }
    int rc;
    if ((rc = dev_upload(p, t, &p->lo0)) || (rc = dev_upload(p, t2, &p->hi0))) return rc;

    const double ls = std::log2(p->scale);
    const Chain chain(p);
    for (int k = 0; k < p->nlev; ++k) {
        Level &L = p->lev[k];
        for (auto &x : xr) x -= ls;
        const int h = L.h, w = L.w, sy = H / 2 - h / 2, sx = W / 2 - w / 2;
        std::vector<float> pa((size_t)nb * h * w), ps((size_t)nb * h * w);
        std::vector<float> hm((size_t)h * w);
        std::vector<double> ch((size_t)h * w);
        for (int u = 0; u < h; ++u)
            for (int v = 0; v < w; ++v) {
                const size_t s = (size_t)(sy + shifted_of(u, h)) * W + (sx + shifted_of(v, w));
                hm[(size_t)u * w + v] = (float)interp(log_rad[s], xr, yr);
                ch[(size_t)u * w + v] = chain(s, k);
            }
        for (int b = 0; b < nb; ++b) {
            for (int i = 0; i < nl; ++i) xcb[i] = xc[i] + kPi * b / nb;
            for (int u = 0; u < h; ++u)
                for (int v = 0; v < w; ++v) {
                    const size_t s = (size_t)(sy + shifted_of(u, h)) * W + (sx + shifted_of(v, w));
                    const size_t o = ((size_t)b * h + u) * w + v;
                    // float32 tables of the oracle multiplied in fp32 there; here folded in double
                    pa[o] = (float)((double)(float)interp(angle[s], xcb, ya) * (double)hm[(size_t)u * w + v] * ch[(size_t)u * w + v]);
                    ps[o] = (float)((double)(float)interp(angle[s], xcb, ys) * (double)hm[(size_t)u * w + v]);
                }
        }
        const int h2 = k + 1 < p->nlev ? p->lev[k + 1].h : p->low.h, w2 = k + 1 < p->nlev ? p->lev[k + 1].w : p->low.w;
        const int sy2 = H / 2 - h2 / 2, sx2 = W / 2 - w2 / 2;
        std::vector<float> lm((size_t)h2 * w2);
        for (int u = 0; u < h2; ++u)
            for (int v = 0; v < w2; ++v) {
                const size_t s = (size_t)(sy2 + shifted_of(u, h2)) * W + (sx2 + shifted_of(v, w2));
                lm[(size_t)u * w2 + v] = (float)interp(log_rad[s], xr, yir);
            }
        if ((rc = dev_upload(p, pa, &L.P_a)) || (rc = dev_upload(p, ps, &L.P_s)) || (rc = dev_upload(p, lm, &L.lomask)))
            return rc;
    }
    {   // low residual: real(ifft2(window(dft) * lo0 * prod_j lomask_j))
        const int h2 = p->low.h, w2 = p->low.w, sy2 = H / 2 - h2 / 2, sx2 = W / 2 - w2 / 2;
        std::vector<float> lg((size_t)h2 * w2);
        for (int u = 0; u < h2; ++u)
            for (int v = 0; v < w2; ++v)
                lg[(size_t)u * w2 + v] = (float)chain((size_t)(sy2 + shifted_of(u, h2)) * W + (sx2 + shifted_of(v, w2)), p->nlev);
        if ((rc = dev_upload(p, lg, &p->low_gain))) return rc;
    }
    return VFI_OK;
}

// Column tile width and bands per transform call of a fused level kernel: large levels take the widest tile that fits
// and one band per call; small levels (latency-bound: few workgroups, each a chain of short phases) put 2 or all 4 bands
// through one call as extra lines, with tiles of >= 8 columns.
void level_tiling(const vfi::fft::Plan1D &ph, int w, int *tile, int *bands) {
    using namespace vfi::fft;
    *tile = cols_per_group(ph, w);
    *bands = 1;
    for (int bp : {4, 2}) {
        int c = *tile;
        while (c > 8 && (bp * c * ph.m > max_elems(ph) || bp * c * col_pitch(ph, c) + ph.tw_len > kLdsElems)) c /= 2;
        if (c >= 8 || c == *tile) {
            if (bp * c * ph.m <= max_elems(ph) && bp * c * col_pitch(ph, c) + ph.tw_len <= kLdsElems) {
                *tile = c;
                *bands = bp;
                return;
            }
        }
    }
}

int get_fft(vfi_pyr_plan *p, int n, vfi::fft::Plan1D *out) {
    auto it = p->fft1d.find(n);
    if (it == p->fft1d.end()) {
        vfi::fft::Plan1D pl;
        const int rc = vfi::fft::make_plan(n, &pl, [](void *ctx, void *dev) { static_cast<vfi_pyr_plan *>(ctx)->allocs.push_back(dev); }, p);
        if (rc) return rc;
        it = p->fft1d.emplace(n, pl).first;
    }
    *out = it->second;
    return VFI_OK;
}

// ---- wave engine (vfi_wfft.h) selection: engine length of a pass or 0, and its stage twiddles (built once per plan) ----
// (get_fft / wave_tables are for plan creation only: a call reads what resolve_level / resolve_size left in the plan)
int wave_twiddles(vfi_pyr_plan *p, WavePass kind, int M, const float2 **out) {
    auto &cache = p->wave_tw[kind];
    auto it = cache.find(M);
    if (it == cache.end()) {
        std::vector<float2> tw(4096);
        const int cap = (int)tw.size();
        const int cnt = kind == kWaveRows ? vfi::pyrw::rows_twiddles(M, tw.data(), cap)
                                          : (kind == kWaveAnaCols ? vfi::pyrw::cols_twiddles(M, tw.data(), cap) : vfi::pyrw::syn_twiddles(M, tw.data(), cap));
        if (cnt < 0) return vfi::fail(VFI_ERR_UNSUPPORTED, "pyramid: no wave-engine twiddles for length %d", M);
        tw.resize(cnt > 0 ? cnt : 1);
        float2 *dev = nullptr;
        const int rc = dev_upload(p, tw, &dev);
        if (rc) return rc;
        it = cache.emplace(M, dev).first;
    }
    *out = it->second;
    return VFI_OK;
}
// tables of a pass on the wave engine; tb->M == 0 when the engine has no configuration for this length
int wave_tables(vfi_pyr_plan *p, WavePass kind, const vfi::fft::Plan1D &pl, vfi::pyrw::Tables *tb) {
    // A/B switch: VFI_PYR_WAVE = bit mask of the passes that may run on the wave engine (1 rows, 2 analysis columns and
    // plain column passes, 4 synthesis columns; default all, 0 = the generic LDS engine everywhere)
    static const int allowed = [] { const char *e = getenv("VFI_PYR_WAVE"); return e ? atoi(e) : 7; }();
    *tb = vfi::pyrw::Tables{};
    const bool off = !((allowed >> (int)kind) & 1);
    const int M = off ? 0 : (kind != kWaveRows ? vfi::pyrw::cols_engine_length(pl.n, pl.bluestein ? pl.m : 0) : vfi::pyrw::rows_engine_length(pl.n, pl.bluestein ? pl.m : 0));
    if (!M) return VFI_OK;
    const int rc = wave_twiddles(p, kind, M, &tb->tw);
    if (rc) return rc;
    tb->chirp = pl.chirp; tb->bfilt = pl.bfilt; tb->M = M; tb->n = pl.n; tb->bluestein = pl.bluestein;
    return VFI_OK;
}
inline int round_up16(int x) { return (x + 15) & ~15; }

// the two transforms of one size and which of its passes run on the wave engine (the band levels have a synthesis column
// pass of their own; the plain 2-D transforms of the low residual and the frame run with the analysis column geometry)
int resolve_size(vfi_pyr_plan *p, Size2D *z, bool syn_cols) {
    int rc;
    if ((rc = get_fft(p, z->h, &z->ph)) || (rc = get_fft(p, z->w, &z->pw)) ||
        (rc = wave_tables(p, kWaveAnaCols, z->ph, &z->wave[kWaveAnaCols])) || (rc = wave_tables(p, kWaveRows, z->pw, &z->wave[kWaveRows])))
        return rc;
    return syn_cols ? wave_tables(p, kWaveSynCols, z->ph, &z->wave[kWaveSynCols]) : VFI_OK;
}
int resolve_level(vfi_pyr_plan *p, Level *L) {
    const int rc = resolve_size(p, L, true);
    if (rc) return rc;
    const bool wave_rows = L->wave[kWaveRows].M != 0;      // (the generic kernels address T densely)
    L->tpitch_ana = wave_rows && L->wave[kWaveAnaCols].M ? round_up16(L->w) : L->w;
    L->tpitch_syn = wave_rows && L->wave[kWaveSynCols].M ? round_up16(L->w) : L->w;
    level_tiling(L->ph, L->w, &L->tile, &L->bands);
    return VFI_OK;
}

}  // namespace

extern "C" int vfi_pyr_plan_create(int H, int W, int height, int nbands, double scale_factor, int max_images,
                                   vfi_pyr_plan **out) {
    VFI_REQUIRE(out, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_create: null out");
    *out = nullptr;
    VFI_REQUIRE(H >= 4 && W >= 4 && height >= 3 && height - 2 <= kMaxLevels, VFI_ERR_INVALID_ARG,
                "vfi_pyr_plan_create: bad size %dx%d height %d", H, W, height);
    VFI_REQUIRE(nbands == 4, VFI_ERR_UNSUPPORTED, "vfi_pyr_plan_create: nbands=%d (the path uses 4)", nbands);
    VFI_REQUIRE(scale_factor > 1.0 && scale_factor <= 2.0, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_create: scale_factor %g", scale_factor);
    VFI_REQUIRE(max_images >= 1 && max_images <= kMaxImages, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_create: max_images %d", max_images);
    vfi_pyr_plan *p = new (std::nothrow) vfi_pyr_plan();
    VFI_REQUIRE(p, VFI_ERR_NOMEM, "vfi_pyr_plan_create: host allocation");
    p->H = H; p->W = W; p->height = height; p->nbands = nbands; p->nlev = height - 2; p->scale = scale_factor;
    p->max_images = max_images;
    p->lev.resize(p->nlev);
    for (int k = 0; k < p->nlev; ++k) { p->lev[k].h = level_size(H, scale_factor, k); p->lev[k].w = level_size(W, scale_factor, k); }
    p->low.h = level_size(H, scale_factor, p->nlev);
    p->low.w = level_size(W, scale_factor, p->nlev);
    int rc = VFI_OK;
    if (p->low.h < 2 || p->low.w < 2) rc = vfi::fail(VFI_ERR_SHAPE, "vfi_pyr_plan_create: height %d too large for %dx%d", height, H, W);
    if (!rc) rc = build_tables(p);
    // every transform table the plan can meet and every level's passes, resolved here: no later call allocates or looks up
    p->frame.h = H; p->frame.w = W;
    for (int k = 0; k < p->nlev && !rc; ++k) rc = resolve_level(p, &p->lev[k]);
    if (!rc) rc = resolve_size(p, &p->low, false);
    if (!rc) rc = resolve_size(p, &p->frame, false);
    p->tpitch_max = round_up16(W);
    const size_t N = max_images, HW = (size_t)H * p->tpitch_max, half = (size_t)H * (W / 2 + 1);
    if (!rc) rc = dev_alloc(p, (void **)&p->half0, N * half * sizeof(float2));
    if (!rc) rc = dev_alloc(p, (void **)&p->half_hi, N * half * sizeof(float2));
    if (!rc) rc = dev_alloc(p, (void **)&p->bands, N * nbands * HW * sizeof(float2));
    if (!rc) rc = dev_alloc(p, (void **)&p->lod[0], N * HW * sizeof(float2));
    if (!rc) rc = dev_alloc(p, (void **)&p->lod[1], N * HW * sizeof(float2));
    if (!rc) rc = dev_alloc(p, (void **)&p->amp_bits, kMaxLevels * 4 * sizeof(unsigned));
    if (!rc && getenv("VFI_PYR_POISON")) {      // debugging aid: NaN-fill the workspace, so a read of anything not yet written shows
        (void)hipMemset(p->half0, 0xff, N * half * sizeof(float2));
        (void)hipMemset(p->half_hi, 0xff, N * half * sizeof(float2));
        (void)hipMemset(p->bands, 0xff, N * nbands * HW * sizeof(float2));
        (void)hipMemset(p->lod[0], 0xff, N * HW * sizeof(float2));
        (void)hipMemset(p->lod[1], 0xff, N * HW * sizeof(float2));
    }
    if (rc) {
        if (rc == VFI_ERR_NOMEM) vfi::set_error("vfi_pyr_plan_create: device allocation failed");
        vfi_pyr_plan_destroy(p);
        return rc;
    }
    *out = p;
    return VFI_OK;
}

extern "C" int vfi_pyr_plan_prepare_filter(vfi_pyr_plan *p, unsigned long long level_mask, int keep_high, int keep_low,
                                           int *filter_id) {
    VFI_REQUIRE(p && filter_id, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_prepare_filter: null pointer");
    const int H = p->H, W = p->W, wh = W / 2 + 1;
    const double ls = std::log2(p->scale);
    std::vector<float> g((size_t)H * wh);
    for (int u = 0; u < H; ++u)
        for (int v = 0; v < wh; ++v) {
            const int fy = u <= H - H / 2 - 1 ? u : u - H, fx = v;          // signed frequencies (v < wh: non-negative)
            const double lr = p->log_rad[(size_t)shifted_of(u, H) * W + shifted_of(v, W)];
            const double lo0 = interp(lr, p->xr0, p->yir), hi0 = interp(lr, p->xr0, p->yr);
            double lowchain = 1.0, acc = 0.0;       // prod_{j<k} lomask_j^2 on the running window
            std::vector<double> xr = p->xr0;
            for (int k = 0; k <= p->nlev; ++k) {
                const int h = k < p->nlev ? p->lev[k].h : p->low.h, w = k < p->nlev ? p->lev[k].w : p->low.w;
                const bool inside = fy >= -(h / 2) && fy <= h - h / 2 - 1 && fx >= -(w / 2) && fx <= w - w / 2 - 1;
                if (!inside) { lowchain = 0.0; break; }
                if (k == p->nlev) break;
                for (auto &x : xr) x -= ls;
                const double hm = interp(lr, xr, p->yr), lm = interp(lr, xr, p->yir);
                if ((level_mask >> k) & 1ull) acc += lowchain * hm * hm;
                lowchain *= lm * lm;
            }
            if (keep_low) acc += lowchain;
            const double gain = (keep_high ? hi0 * hi0 : 0.0) + lo0 * lo0 * acc;
            g[(size_t)u * wh + v] = (float)(gain / ((double)H * W));
        }
    float *dev = nullptr;
    int rc = dev_upload(p, g, &dev);
    if (rc) return vfi::fail(rc, "vfi_pyr_plan_prepare_filter: device allocation / upload failed");
    p->filters.push_back(dev);
    *filter_id = (int)p->filters.size() - 1;
    return VFI_OK;
}

extern "C" int vfi_pyr_plan_destroy(vfi_pyr_plan *p) {
    if (!p) return VFI_OK;
    for (void *d : p->allocs) (void)hipFree(d);
    delete p;
    return VFI_OK;
}

extern "C" int vfi_pyr_plan_level_size(const vfi_pyr_plan *p, int level, int *h, int *w) {
    VFI_REQUIRE(p && h && w, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_level_size: null pointer");
    VFI_REQUIRE(level >= 0 && level <= p->nlev, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_level_size: level %d", level);
    *h = level < p->nlev ? p->lev[level].h : p->low.h;
    *w = level < p->nlev ? p->lev[level].w : p->low.w;
    return VFI_OK;
}

// what resolve_level / resolve_size stored for one pass of one size: nothing is looked up again and nothing is launched
extern "C" int vfi_pyr_plan_query_pass(const vfi_pyr_plan *p, int size_index, int pass, int *info) {
    VFI_REQUIRE(p && info, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_query_pass: null pointer");
    VFI_REQUIRE(size_index >= 0 && size_index <= p->nlev + 1, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_query_pass: size index %d", size_index);
    const bool band = size_index < p->nlev;
    VFI_REQUIRE(pass == VFI_PYR_PASS_ROWS || pass == VFI_PYR_PASS_ANA_COLS || (pass == VFI_PYR_PASS_SYN_COLS && band), VFI_ERR_INVALID_ARG,
                "vfi_pyr_plan_query_pass: pass %d of size index %d", pass, size_index);
    const Size2D &z = band ? static_cast<const Size2D &>(p->lev[size_index]) : (size_index == p->nlev ? p->low : p->frame);
    const vfi::fft::Plan1D &pl = pass == VFI_PYR_PASS_ROWS ? z.pw : z.ph;
    static_assert((int)kWaveRows == VFI_PYR_PASS_ROWS && (int)kWaveAnaCols == VFI_PYR_PASS_ANA_COLS && (int)kWaveSynCols == VFI_PYR_PASS_SYN_COLS,
                  "VFI_PYR_PASS_* index Size2D::wave");
    info[0] = pl.n; info[1] = pl.bluestein ? 1 : 0; info[2] = pl.m; info[3] = z.wave[pass].M;
    info[4] = info[5] = info[6] = info[7] = 0;
    if (band) {
        const Level &L = p->lev[size_index];
        info[4] = L.tile; info[5] = L.bands; info[6] = L.tpitch_ana; info[7] = L.tpitch_syn;
    }
    return VFI_OK;
}

// A_k[b] = lo0 * prod_{j<k} lomask_j * himask_k * two-sided angle mask b on level k's window (unshifted order): P_a with the
// synthesis' angle masks.  The synthesis is real-linear in the band coefficients z_{k,b}; its adjoint applied to a gradient
// image g is  grad z_{k,b} = 1/(H W) * IFFT2_k,unnormalised( i * window_k(FFT2(g)) * A_k[b] )  -- an analysis level with
// these tables and the synthesis' final 1/(H W) (conj of the forward's -i is +i, the analysis' rotation).
extern "C" int vfi_pyr_plan_prepare_adjoint(vfi_pyr_plan *p) {
    VFI_REQUIRE(p, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_prepare_adjoint: null plan");
    if (p->adjoint) return VFI_OK;
    const int H = p->H, W = p->W, nb = p->nbands;
    const std::vector<double> gy = linspace_grid(H), gx = linspace_grid(W);
    std::vector<double> xc, ya, ys;
    angle_luts(nb, xc, ya, ys);
    std::vector<double> xcb(xc.size()), xr = p->xr0;
    const double ls = std::log2(p->scale);
    const Chain chain(p);
    std::vector<std::vector<float>> tabs(p->nlev);
    for (int k = 0; k < p->nlev; ++k) {
        const Level &L = p->lev[k];
        for (auto &x : xr) x -= ls;
        const int h = L.h, w = L.w, sy = H / 2 - h / 2, sx = W / 2 - w / 2;
        std::vector<double> g((size_t)h * w);      // himask_k * chain, as build_tables folds P_a
        for (int u = 0; u < h; ++u)
            for (int v = 0; v < w; ++v) {
                const size_t s = (size_t)(sy + shifted_of(u, h)) * W + (sx + shifted_of(v, w));
                g[(size_t)u * w + v] = (double)(float)interp(p->log_rad[s], xr, p->yr) * chain(s, k);
            }
        std::vector<float> &a = tabs[k];
        a.resize((size_t)nb * h * w);
        for (int b = 0; b < nb; ++b) {
            for (size_t i = 0; i < xc.size(); ++i) xcb[i] = xc[i] + kPi * b / nb;
            for (int u = 0; u < h; ++u)
                for (int v = 0; v < w; ++v) {
                    const int i = sy + shifted_of(u, h), j = sx + shifted_of(v, w);
                    a[((size_t)b * h + u) * w + v] = (float)((double)(float)interp(std::atan2(gy[i], gx[j]), xcb, ys) * g[(size_t)u * w + v]);
                }
        }
    }
    for (int k = 0; k < p->nlev; ++k) {
        const int rc = dev_upload(p, tabs[k], &p->lev[k].A);
        if (rc) return vfi::fail(rc, "vfi_pyr_plan_prepare_adjoint: device allocation / upload failed");
    }
    p->adjoint = true;
    return VFI_OK;
}

// B_k[b] = himask_k * one-sided angle mask b * (H W) / (h_k w_k) on level k's window (unshifted order).  The analysis is
// z_{k,b} = 1/(h_k w_k) * IFFT2_k,unnormalised(i * window_k(FFT2(x)) * P_a[k][b]); its adjoint applied to coefficient gradients
// G is  grad x = Re IFFT2,unnormalised( sum_k embed_k( (-i) * P_a[k][b] * FFT2_k(G_{k,b}) / (h_k w_k) ) )  -- the synthesis' passes.
// P_a itself cannot stand in for the synthesis' P_s there: it carries lo0 * prod_{j<k} lomask_j, which the synthesis' column
// pass and final kernel apply again on the way up (lomask_j at every embed, lo0 at the end), and not the constant that
// turns the synthesis' final 1/(H W) into 1/(h_k w_k).  So B_k is P_a without that chain, times H W / (h_k w_k).
extern "C" int vfi_pyr_plan_prepare_analysis_adjoint(vfi_pyr_plan *p) {
    VFI_REQUIRE(p, VFI_ERR_INVALID_ARG, "vfi_pyr_plan_prepare_analysis_adjoint: null plan");
    if (p->analysis_adjoint) return VFI_OK;
    const int H = p->H, W = p->W, nb = p->nbands;
    const std::vector<double> gy = linspace_grid(H), gx = linspace_grid(W);
    std::vector<double> xc, ya, ys;
    angle_luts(nb, xc, ya, ys);
    std::vector<double> xcb(xc.size()), xr = p->xr0;
    const double ls = std::log2(p->scale);
    std::vector<std::vector<float>> tabs(p->nlev);
    for (int k = 0; k < p->nlev; ++k) {
        const Level &L = p->lev[k];
        for (auto &x : xr) x -= ls;
        const int h = L.h, w = L.w, sy = H / 2 - h / 2, sx = W / 2 - w / 2;
        const double c = ((double)H * W) / ((double)h * w);
        std::vector<double> g((size_t)h * w);      // himask_k (the oracle's float32 table) * H W / (h w)
        for (int u = 0; u < h; ++u)
            for (int v = 0; v < w; ++v) {
                const size_t s = (size_t)(sy + shifted_of(u, h)) * W + (sx + shifted_of(v, w));
                g[(size_t)u * w + v] = (double)(float)interp(p->log_rad[s], xr, p->yr) * c;
            }
        std::vector<float> &t = tabs[k];
        t.resize((size_t)nb * h * w);
        for (int b = 0; b < nb; ++b) {
            for (size_t i = 0; i < xc.size(); ++i) xcb[i] = xc[i] + kPi * b / nb;
            for (int u = 0; u < h; ++u)
                for (int v = 0; v < w; ++v) {
                    const int i = sy + shifted_of(u, h), j = sx + shifted_of(v, w);
                    t[((size_t)b * h + u) * w + v] = (float)((double)(float)interp(std::atan2(gy[i], gx[j]), xcb, ya) * g[(size_t)u * w + v]);
                }
        }
    }
    for (int k = 0; k < p->nlev; ++k) {
        const int rc = dev_upload(p, tabs[k], &p->lev[k].B);
        if (rc) return vfi::fail(rc, "vfi_pyr_plan_prepare_analysis_adjoint: device allocation / upload failed");
    }
    p->analysis_adjoint = true;
    return VFI_OK;
}
