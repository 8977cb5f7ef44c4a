// Analysis column pass of the steerable pyramid on the wave-private FFT engine: ana_cols_kernel (vfi_pyrw_kernels.h)
// instantiated for every column configuration of vfi_wfft_configs.h, plus the column-side lookups of vfi_pyramid_wave.h.
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

int cols_engine_length(int n, int bluestein_m) { return engine_length<kColConfigs>(n, bluestein_m); }
int cols_twiddles(int M, float2 *out, int cap) { return twiddles<kColConfigs>(M, out, cap); }

int launch_ana_cols(const AnaColsArgs &a, hipStream_t s) {
    return dispatch<kColConfigs>(a.tb, "pyramid columns", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        return launch_cols<C, BLU, ana_cols_kernel<C, BLU>>(a, a.w, a.N * kBands, s);
    });
}

}  // namespace pyrw
}  // namespace vfi
