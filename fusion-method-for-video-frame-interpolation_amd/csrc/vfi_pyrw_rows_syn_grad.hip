// Adjoint row pass of the steerable pyramid's analysis on the wave-private FFT engine: rows_from_polar_kernel
// (vfi_pyrw_kernels.h) with its gradient prologue, instantiated for every row configuration of vfi_wfft_configs.h
// (vfi_pyr_analyze_backward).
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

int launch_rows_from_polar_grad(const RowsGradArgs &a, hipStream_t s) {
    return dispatch<kRowConfigs>(a.tb, "pyramid rows", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        return launch_rows<C, BLU, rows_from_polar_kernel<C, BLU, true>>(a, (a.planes * a.h + C::L - 1) / C::L, s);
    });
}

}  // namespace pyrw
}  // namespace vfi
