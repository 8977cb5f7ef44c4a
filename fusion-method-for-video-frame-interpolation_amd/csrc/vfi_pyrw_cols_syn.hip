// Synthesis column pass of the steerable pyramid on the wave-private FFT engine: syn_cols_kernel (vfi_pyrw_kernels.h)
// instantiated for every synthesis column configuration of vfi_wfft_configs.h.
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

// (the synthesis column configurations own fewer lines per wave than the analysis ones, so their radix order -- and with
// it the stage twiddles -- may differ for the same length)
int syn_twiddles(int M, float2 *out, int cap) { return twiddles<kSynConfigs>(M, out, cap); }

int launch_syn_cols(const SynColsArgs &a, hipStream_t s) {
    return dispatch<kSynConfigs>(a.tb, "pyramid columns", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        return launch_syn<C, BLU, syn_cols_kernel<C, BLU>>(a, s);
    });
}

}  // namespace pyrw
}  // namespace vfi
