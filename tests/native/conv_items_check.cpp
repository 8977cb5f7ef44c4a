// Host-side check of the item order the persistent Winograd kernels walk (csrc/vfi_conv_common.h: w2::decode_item of the
// F(2x2) kernel with its K splits; csrc/vfi_conv_winograd4_common.h: w4::decode_item of the two F(4x4) kernels).  The
// ConvArgs are filled the way launch_winograd / launch_winograd4 fill them.  For every geometry:
//   * every (split, sample, tile, channel block) is decoded from exactly one valid item;
//   * an invalid (padding) item lies past the batch, n >= wino_batch;
//   * x0 / y0 name a tile of the grid;
//   * the channel blocks of one tile sit in slots L, L + 8, ... : the same XCD, back to back (the locality rule the
//     order exists for).
// Built and run by tests/test_conv_host.py (hipcc --cuda-host-only).
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "vfi_conv_winograd4_common.h"

using namespace vfi::conv;

namespace {

struct Geometry {
    int tiles_x, tiles_y, N, cb, run, splits;
};

ConvArgs make_args(const Geometry &g) {
    ConvArgs a{};
    a.Cout_pad = g.cb * 32;
    a.Cout = a.Cout_pad;
    a.tiles_x = g.tiles_x;
    a.wino_tiles = g.tiles_x * g.tiles_y;
    a.wino_batch = g.N;
    a.wino_run = g.run;
    a.wino_items = round_up(a.wino_tiles * g.N, 8 * g.run) * g.cb;
    a.splits = g.splits;
    a.fd_items = make_fastdiv((unsigned)a.wino_items);
    a.fd_cb = make_fastdiv((unsigned)g.cb);
    a.fd_run = make_fastdiv((unsigned)g.run);
    a.fd_tiles = make_fastdiv((unsigned)a.wino_tiles);
    a.fd_tiles_x = make_fastdiv((unsigned)g.tiles_x);
    a.fd_splits = make_fastdiv((unsigned)g.splits);
    return a;
}

// One decoded item in the kernels' common terms (split = 0 for F(4x4)).
struct Decoded {
    int split, n, x0, y0, nb;
    bool valid;
};

template <class Decode>
long check(const Geometry &g, int TW, int TH, Decode decode, std::vector<int> &first, const char *what) {
    const ConvArgs a = make_args(g);
    const int tiles = a.wino_tiles, per_split = g.N * tiles * g.cb;
    const long total = (long)a.wino_items * g.splits;
    first.assign((size_t)per_split * g.splits, -1);        // slot of (split, n, tile, nb), -1: not seen yet
    long bad = 0, valid = 0;
    for (long L = 0; L < total; ++L) {
        const Decoded d = decode(a, (int)L);
        const bool grid = d.x0 >= 0 && d.y0 >= 0 && d.x0 % TW == 0 && d.y0 % TH == 0 && d.x0 / TW < g.tiles_x && d.y0 / TH < g.tiles_y;
        const bool range = d.split >= 0 && d.split < g.splits && d.split == L / a.wino_items && d.nb >= 0 && d.nb < g.cb && d.n >= 0;
        if (!grid || !range || d.valid != (d.n < g.N)) {
            ++bad;
            continue;
        }
        if (!d.valid) continue;
        ++valid;
        const int tile = d.y0 / TH * g.tiles_x + d.x0 / TW;
        int &slot = first[(((size_t)d.split * g.N + d.n) * tiles + tile) * g.cb + d.nb];
        if (slot >= 0) ++bad;                              // decoded twice
        slot = (int)L;
    }
    if (valid != (long)per_split * g.splits) ++bad;       // (with "never twice": exactly once)
    for (size_t e = 0; e < first.size(); e += g.cb)
        for (int nb = 0; nb < g.cb; ++nb)
            if (first[e] < 0 || first[e + nb] != first[e] + 8 * nb) ++bad;
    if (bad)
        std::printf("%s: tiles %dx%d N %d cb %d run %d splits %d: %ld violations\n", what, g.tiles_x, g.tiles_y, g.N, g.cb, g.run, g.splits, bad);
    return bad;
}

}  // namespace

int main() {
    long bad = 0, combos = 0;
    std::vector<int> first;
    for (int tx : {1, 2, 3, 5, 30, 60})
        for (int ty : {1, 2, 3, 7, 17, 68})
            for (int N : {1, 2, 3})
                for (int cb : {1, 2, 3, 16})
                    for (int run : {1, 2, 4, 8}) {
                        ++combos;
                        bad += check(Geometry{tx, ty, N, cb, run, 1}, 64, 16, [](const ConvArgs &a, int L) {
                            const w4::Item it = w4::decode_item(a, L);
                            return Decoded{0, it.n, it.x0, it.y0, it.nb, it.valid};
                        }, first, "F(4x4)");
                        for (int splits : {1, 2, 4, 8, 16}) {
                            ++combos;
                            bad += check(Geometry{tx, ty, N, cb, run, splits}, 32, 8, [](const ConvArgs &a, int L) {
                                const w2::Item it = w2::decode_item(a, L);
                                return Decoded{it.split, it.n, it.x0, it.y0, it.nb, it.valid};
                            }, first, "F(2x2)");
                        }
                    }
    std::printf("checked %ld geometries, %ld violations\n", combos, bad);
    return bad ? 1 : 0;
}
