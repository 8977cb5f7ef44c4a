// Internal interface between vfi_pyr_plan.hip (the plan: mask tables, transform tables and every level's resolved passes,
// all built at vfi_pyr_plan_create) and vfi_pyramid.hip (the kernels and the calls that run on a plan).  After creation a
// call reads the plan through `const` access and writes the workspace only; vfi_pyr_plan_prepare_filter /
// vfi_pyr_plan_prepare_adjoint / vfi_pyr_plan_prepare_analysis_adjoint add tables, as include/vfi_hip.h documents.
#pragma once
#include "vfi_common.h"
#include "vfi_fft.h"
#include "vfi_pyramid_wave.h"

#include <map>
#include <vector>

namespace vfi {
namespace pyr {

constexpr int kMaxLevels = 40;
constexpr int kMaxImages = 16;

// passes the wave engine (vfi_wfft.h) has its own stage twiddles for; the bit positions of VFI_PYR_WAVE
enum WavePass { kWaveRows = 0, kWaveAnaCols = 1, kWaveSynCols = 2 };

// One 2-D transform size of the plan and how its passes run: a function of (H, W, height, scale) only.
struct Size2D {
    int h = 0, w = 0;
    fft::Plan1D ph = {}, pw = {};   // column (length h) and row (length w) transform on the generic LDS engine (vfi_fft.h)
    pyrw::Tables wave[3] = {};      // [WavePass] the same pass on the wave engine; M == 0: the generic engine runs it
};

struct Level : Size2D {        // h x w: the level's window of the spectrum
    float *P_a;                // [nb][h][w] analysis  : lo0 * prod_{j<k} lomask_j * himask_k * angle mask (one sided), unshifted order
    float *P_s;                // [nb][h][w] synthesis : angle mask (two sided) * himask
    float *lomask;             // [h2][w2]  low-pass applied to the NEXT level's window, unshifted order of that window
    float *A = nullptr;        // [nb][h][w] synthesis adjoint: lo0 * prod_{j<k} lomask_j * P_s (vfi_pyr_plan_prepare_adjoint)
    float *B = nullptr;        // [nb][h][w] analysis adjoint: himask_k * angle mask (one sided) * H W / (h w) (vfi_pyr_plan_prepare_analysis_adjoint)
    int tpitch_ana, tpitch_syn;   // row pitch of T: w rounded up to 16 when both passes run on the wave engine (the generic kernels address T densely)
    int tile, bands;           // generic-engine column pass: columns per workgroup, bands per transform call
};

}  // namespace pyr
}  // namespace vfi

struct vfi_pyr_plan {
    int H, W, height, nbands, nlev, max_images;
    double scale;
    std::vector<vfi::pyr::Level> lev;   // nlev band levels
    vfi::pyr::Size2D low, frame;        // low residual (hl x wl) and the frame (H x W): plain 2-D transforms (wave[kWaveSynCols] unused)
    float *lo0 = nullptr, *hi0 = nullptr;   // [H][W] unshifted
    float *low_gain = nullptr;   // [hl][wl] lo0 * prod_j lomask_j on the low residual's window, unshifted
    int tpitch_max = 0;          // row pitch of T the workspace is sized for (W rounded up to 16)
    // de-duplication while the plan is built (several levels share a length); calls read Size2D instead
    std::map<int, vfi::fft::Plan1D> fft1d;      // transform length -> tables (vfi_fft.h)
    std::map<int, const float2 *> wave_tw[3];   // [WavePass] engine length -> stage twiddles (vfi_wfft.h)
    // workspace (complex64 unless noted)
    float2 *half0 = nullptr;     // N x H x (W/2+1)   R2C spectrum of the input / FFT of high on synthesis
    float2 *half_hi = nullptr;   // N x H x (W/2+1)   high-pass half spectrum (C2R input)
    float2 *bands = nullptr;     // N x nb x H x W    band spectra / coefficients of the current level
    float2 *lod[2] = {nullptr, nullptr};   // N x H x W each: running low-pass spectrum (ping-pong)
    unsigned *amp_bits = nullptr;            // kMaxLevels * 4 words: vfi_pyr_analyze_max
    std::vector<void *> allocs;
    // kept for vfi_pyr_plan_prepare_filter
    std::vector<double> log_rad, xr0, yr, yir;
    std::vector<float *> filters;   // [id] -> H x (W/2+1) radial gain tables
    bool adjoint = false;           // Level::A built (vfi_pyr_plan_prepare_adjoint)
    bool analysis_adjoint = false;  // Level::B built (vfi_pyr_plan_prepare_analysis_adjoint)
};
