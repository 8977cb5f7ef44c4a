// Host-side check of the tile geometry of vfi_phasenet_level_tail (csrc/vfi_phasenet_tail.h: tile_span).  For a source level
// (h, w) up-scaled to (H, W), over the kernel's grid of TY x TX target tiles:
//   * every source pixel is owned by exactly one tile (the tile that emits its phase and amplitude);
//   * every owned pixel lies inside its tile's source window (so its prediction is there to emit);
//   * the window fits the kernel's LDS planes (MAX_ROWS x MAX_COLS);
//   * both bilinear taps of every target pixel of a tile lie inside its window.
// Run over the 15 consecutive level pairs of a 1080p and of a 720p pyramid (sqrt(2) steps) and 400 random pairs with
// 1 <= H / h <= 2; then over what the entry point accepts beyond that: 20 pairs with an exact scale of 1 along one axis or
// both, exact x2, x3 and x8 and the shapes tests/test_phasenet_head_f64_gpu.py launches, and 1500 random pairs with
// 1 <= H / h <= 8 and 1 <= W / w <= 8 drawn independently.  Built and run by tests/test_phasenet_tail_host.py (hipcc --cuda-host-only).
#include <cmath>
#include <cstdio>
#include <vector>

#include "vfi_phasenet_tail.h"

using namespace vfi::tail;

namespace {

// one axis: windows, capacity and taps; returns violations
long check_axis(int in, int out, int T, int max_window) {
    long bad = 0;
    const float scale = (float)in / (float)out;
    int expect = 0;
    for (int t0 = 0; t0 < out; t0 += T) {
        const Span s = tile_span(t0, T, in, out);
        if (s.own_lo != expect || s.own_hi < s.own_lo) ++bad;         // owned ranges follow one another without gap or overlap
        expect = s.own_hi;
        if (s.lo < 0 || s.hi > in - 1 || s.hi - s.lo + 1 > max_window) ++bad;
        if (s.own_hi > s.own_lo && (s.own_lo < s.lo || s.own_hi - 1 > s.hi)) ++bad;
        for (int o = t0; o < t0 + T && o < out; ++o) {
            const int a = src_index(scale, o, in), b = a + 1 < in - 1 ? a + 1 : in - 1;
            if (a < s.lo || b > s.hi) ++bad;
        }
    }
    if (expect != in) ++bad;
    return bad;
}

long check_pair(int h, int w, int H, int W, std::vector<unsigned char> &count) {
    long bad = check_axis(h, H, TY, MAX_ROWS) + check_axis(w, W, TX, MAX_COLS);
    count.assign((size_t)h * w, 0);
    for (int Y0 = 0; Y0 < H; Y0 += TY)
        for (int X0 = 0; X0 < W; X0 += TX) {
            const Span sy = tile_span(Y0, TY, h, H), sx = tile_span(X0, TX, w, W);
            for (int y = sy.own_lo; y < sy.own_hi; ++y)
                for (int x = sx.own_lo; x < sx.own_hi; ++x) {
                    if (y < 0 || y >= h || x < 0 || x >= w) { ++bad; continue; }
                    if (y < sy.lo || y > sy.hi || x < sx.lo || x > sx.hi) ++bad;
                    if (++count[(size_t)y * w + x] > 1) ++bad;
                }
        }
    for (size_t i = 0; i < count.size(); ++i)
        if (count[i] != 1) ++bad;
    if (bad) std::printf("%dx%d -> %dx%d: %ld violations\n", h, w, H, W, bad);
    return bad;
}

int level_size(int d, int k) { return (int)std::ceil(d / std::pow(std::sqrt(2.0), k) - 1e-9); }

}  // namespace

int main() {
    long bad = 0, pairs = 0;
    std::vector<unsigned char> count;
    const int frames[2][2] = {{1080, 1920}, {720, 1280}};
    for (const auto &f : frames)
        for (int k = 15; k >= 1; --k, ++pairs)
            bad += check_pair(level_size(f[0], k), level_size(f[1], k), level_size(f[0], k - 1), level_size(f[1], k - 1), count);
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](int n) {        // 0 .. n-1
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((state >> 33) % (unsigned long long)n);
    };
    for (int i = 0; i < 400; ++i, ++pairs) {
        const int h = 1 + rnd(i % 4 == 0 ? 900 : 200), w = 1 + rnd(i % 4 == 0 ? 1400 : 300);
        bad += check_pair(h, w, h + rnd(h + 1), w + rnd(w + 1), count);
    }
    // What the entry point accepts beyond that (h <= H, w <= W, any ratio): an exact scale along one axis or both, exact
    // multiples, and 1500 random pairs of ratio 1..8 per axis.
    const int exact[][4] = {{64, 64, 64, 64},     {1, 1, 1, 1},        {17, 300, 17, 300},  {48, 86, 48, 258},   {200, 130, 283, 130},
                            {37, 129, 37, 183},   {64, 66, 128, 132},  {1, 1, 2, 2},        {135, 240, 270, 480}, {33, 47, 99, 141},
                            {1, 129, 3, 387},     {32, 128, 256, 1024}, {1, 1, 8, 8},       {17, 131, 136, 1048}, {4, 1024, 5, 1449},
                            {1024, 4, 1449, 6},   {46, 90, 65, 127},   {50, 82, 71, 129},   {135, 240, 191, 340},
                            {62, 68, 64, 70}};
    for (const auto &e : exact) {
        bad += check_pair(e[0], e[1], e[2], e[3], count);
        ++pairs;
    }
    for (int i = 0; i < 1500; ++i, ++pairs) {
        const int h = 1 + rnd(i % 8 == 0 ? 300 : 60), w = 1 + rnd(i % 8 == 0 ? 500 : 150);
        const int H = h + rnd(7 * h + 1), W = w + rnd(7 * w + 1);         // h <= H <= 8 h
        bad += check_pair(h, w, H, W, count);
    }
    std::printf("checked %ld level pairs, %ld violations\n", pairs, bad);
    return bad ? 1 : 0;
}
