// Analysis row pass of the steerable pyramid on the wave-private FFT engine: rows_polar_kernel (vfi_pyrw_kernels.h)
// instantiated for every row configuration of vfi_wfft_configs.h, plus the row-side lookups of vfi_pyramid_wave.h.
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

int rows_engine_length(int n, int bluestein_m) { return engine_length<kRowConfigs>(n, bluestein_m); }
int rows_twiddles(int M, float2 *out, int cap) { return twiddles<kRowConfigs>(M, out, cap); }

int launch_rows_polar(const RowsArgs &a, hipStream_t s) {
    return dispatch<kRowConfigs>(a.tb, "pyramid rows", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        return launch_rows<C, BLU, rows_polar_kernel<C, BLU>>(a, (a.planes * a.h + C::L - 1) / C::L, s);
    });
}

}  // namespace pyrw
}  // namespace vfi
