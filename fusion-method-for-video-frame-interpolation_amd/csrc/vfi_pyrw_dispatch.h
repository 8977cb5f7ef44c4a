// From a run-time (engine length, Bluestein or plain) to the kernel instantiation of a wave-engine pass: what the
// vfi_pyrw_*.hip files share.  Each of them is one pass -- its kernel for every configuration of one list of
// vfi_wfft_configs.h -- and is a translation unit of its own only to keep the build parallel.
#pragma once
#include <climits>
#include <cmath>
#include <type_traits>
#include "vfi_pyrw_kernels.h"

namespace vfi {
namespace pyrw {

#define VFI_ROW_CFG(M, L, TEAM, PITCH, P0, P1, P2, R0, R1, R2, R3) Cfg<M, L, TEAM, false, PITCH, P0, P1, P2, R0, R1, R2, R3>
#define VFI_COL_CFG(M, L, TEAM, PITCH, P0, P1, P2, R0, R1, R2, R3) Cfg<M, L, TEAM, true, PITCH, P0, P1, P2, R0, R1, R2, R3>

enum ConfigList { kRowConfigs, kColConfigs, kSynConfigs };      // VFI_WFFT_ROW_CONFIGS / _COL_CONFIGS / _SYN_CONFIGS
template <class C_> struct Tag { using C = C_; };
constexpr int kNoConfig = INT_MIN;

// f(Tag<C>()) for the configuration C of engine length M in the list, or kNoConfig
template <ConfigList LIST, typename F>
inline int for_config(int M, F f) {
#define VFI_ROW_CASE(M, ...) case M: return f(Tag<VFI_ROW_CFG(M, __VA_ARGS__)>());
#define VFI_COL_CASE(M, ...) case M: return f(Tag<VFI_COL_CFG(M, __VA_ARGS__)>());
    if constexpr (LIST == kRowConfigs) {
        switch (M) { VFI_WFFT_ROW_CONFIGS(VFI_ROW_CASE) }
    } else if constexpr (LIST == kColConfigs) {
        switch (M) { VFI_WFFT_COL_CONFIGS(VFI_COL_CASE) }
    } else {
        switch (M) { VFI_WFFT_SYN_CONFIGS(VFI_COL_CASE) }
    }
#undef VFI_ROW_CASE
#undef VFI_COL_CASE
    return kNoConfig;
}

// launch(Tag<C>(), std::bool_constant<BLU>()) for the tables' engine length, in Bluestein's form where they ask for it;
// `what` names the pass in the error text ("pyramid rows")
template <ConfigList LIST, typename F>
inline int dispatch(const Tables &tb, const char *what, F launch) {
    const int rc = for_config<LIST>(tb.M, [&](auto c) {
        using C = typename decltype(c)::C;
        if (!tb.bluestein) return launch(c, std::false_type());
        if constexpr (blu_capable(C::M)) return launch(c, std::true_type());
        return vfi::fail(VFI_ERR_UNSUPPORTED, "%s: engine length %d does not serve Bluestein", what, C::M);
    });
    return rc != kNoConfig ? rc : vfi::fail(VFI_ERR_UNSUPPORTED, "%s: no engine configuration for length %d", what, tb.M);
}

// the lookups of vfi_pyramid_wave.h
template <ConfigList LIST>
inline int engine_length(int n, int bluestein_m) {
    const int m = bluestein_m ? bluestein_m : n;
    if (bluestein_m && (!blu_capable(m) || 2 * n > m)) return 0;
    const int rc = for_config<LIST>(m, [](auto c) { return decltype(c)::C::M; });
    return rc != kNoConfig ? rc : 0;
}
template <ConfigList LIST>
inline int twiddles(int M, float2 *out, int cap) {
    const int rc = for_config<LIST>(M, [&](auto c) {
        using C = typename decltype(c)::C;
        if (C::TW > cap) return -1;
        for_twiddles<C>([&](int idx, int e) {
            const double ang = -2.0 * 3.14159265358979323846 * (double)e / (double)C::M;
            out[idx] = make_float2((float)std::cos(ang), (float)std::sin(ang));
        });
        return C::TW;
    });
    return rc != kNoConfig ? rc : -1;
}

}  // namespace pyrw
}  // namespace vfi
