// Tile geometry of vfi_phasenet_level_tail (vfi_phasenet_tail.hip), shared with the host so that the ownership rule can be
// checked without a GPU (tests/native/phasenet_tail_check.cpp).
//
// A workgroup writes one TY x TX tile of the up-scaled level.  Along each axis the tile [t0, t0 + T) of the `out` target
// positions reads the source positions lo..hi (the window, inclusive: the same bounds resize_bilinear_tile_kernel stages) and
// OWNS the source positions [own_lo, own_hi): own_lo = src(t0), own_hi = src(t0 + T), or `in` for the last tile, with
// src(o) = min((int)coordinate(o), in - 1).  src is monotonic, so the owned ranges of consecutive tiles partition 0..in-1; the
// product of a row range and a column range is the set of source pixels whose level outputs (phase, amplitude) the tile emits.
// Pixels of the window outside the owned range are the halo: their prediction is recomputed, only for the resize.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace vfi {
namespace tail {

constexpr int TY = 16, TX = 128;                          // target tile of one workgroup
constexpr int MAX_ROWS = TY + 2, MAX_COLS = TX + 2;       // its source window when the source step is <= 1 (up-scaling)

// torch's align_corners=False source coordinate of target index o; scale = (float)in / (float)out.  One fused multiply-add,
// written out so that host and device round alike.
__host__ __device__ inline float src_coord(float scale, int o) { return fmaxf(fmaf(scale, (float)o + 0.5f, -0.5f), 0.0f); }
__host__ __device__ inline int src_index(float scale, int o, int in) {
    const int i = (int)src_coord(scale, o);
    return i < in - 1 ? i : in - 1;
}

struct Span {
    int lo, hi;              // source window, inclusive
    int own_lo, own_hi;      // owned source positions [own_lo, own_hi)
};

__host__ __device__ inline Span tile_span(int t0, int T, int in, int out) {
    const float scale = (float)in / (float)out;
    const int last = t0 + T - 1 < out - 1 ? t0 + T - 1 : out - 1;
    const int hi = src_index(scale, last, in) + 1;
    Span s;
    s.lo = src_index(scale, t0, in);
    s.hi = hi < in - 1 ? hi : in - 1;
    s.own_lo = s.lo;
    s.own_hi = t0 + T >= out ? in : src_index(scale, t0 + T, in);
    return s;
}

}  // namespace tail
}  // namespace vfi
