// Plain column passes on the wave-private FFT engine: gen_cols_kernel (vfi_pyrw_passes.h) for every analysis column
// configuration (the long lengths on a team of waves: 8 columns = 64-byte row segments for 1080 rows).
#include "vfi_pyrw_passes.h"
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

int launch_gen_cols(const GenColsArgs &a, bool inverse, hipStream_t s) {
    return dispatch<kColConfigs>(a.tb, "fft columns", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        return inverse ? launch_cols<C, BLU, gen_cols_kernel<C, BLU, true>>(a, a.cols, a.planes, s)
                       : launch_cols<C, BLU, gen_cols_kernel<C, BLU, false>>(a, a.cols, a.planes, s);
    });
}

}  // namespace pyrw
}  // namespace vfi
