// Plain row passes on the wave-private FFT engine: gen_rows_kernel (vfi_pyrw_passes.h) for every row configuration.
#include "vfi_pyrw_passes.h"
#include "vfi_pyrw_dispatch.h"

namespace vfi {
namespace pyrw {

int launch_gen_rows(const GenRowsArgs &a, int load, int store, bool inverse, hipStream_t s) {
    return dispatch<kRowConfigs>(a.tb, "fft rows", [&](auto c, auto blu) {
        using C = typename decltype(c)::C;
        constexpr bool BLU = decltype(blu)::value;
        const int nbatch = (a.rows + C::L - 1) / C::L;
        if (load == kGenReal && store == kGenHalf && !inverse)
            return launch_rows<C, BLU, gen_rows_kernel<C, BLU, kGenReal, kGenHalf, false>>(a, nbatch, s);
        if (load == kGenHalf && store == kGenReal && inverse)
            return launch_rows<C, BLU, gen_rows_kernel<C, BLU, kGenHalf, kGenReal, true>>(a, nbatch, s);
        if (load == kGenComplex && store == kGenComplex)
            return inverse ? launch_rows<C, BLU, gen_rows_kernel<C, BLU, kGenComplex, kGenComplex, true>>(a, nbatch, s)
                           : launch_rows<C, BLU, gen_rows_kernel<C, BLU, kGenComplex, kGenComplex, false>>(a, nbatch, s);
        return vfi::fail(VFI_ERR_UNSUPPORTED, "fft row pass: load %d / store %d / inverse %d", load, store, (int)inverse);
    });
}

}  // namespace pyrw
}  // namespace vfi
