// Synthesis row pass of the steerable pyramid on the wave-private FFT engine: rows_from_polar_kernel
// (vfi_pyrw_kernels.h) instantiated for every row configuration of vfi_wfft_configs.h.
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

int launch_rows_from_polar(const RowsArgs &a, hipStream_t s) {
    return dispatch<kRowConfigs>(a.tb, "pyramid rows", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        return launch_rows<C, BLU, rows_from_polar_kernel<C, BLU>>(a, (a.planes * a.h + C::L - 1) / C::L, s);
    });
}

}  // namespace pyrw
}  // namespace vfi
