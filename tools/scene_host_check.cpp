// Host walk of the scene-cut kernels' address arithmetic (csrc/vfi_scene_body.h), thread by thread over exact-size heap
// buffers, meant to be built with -fsanitize=address,undefined: a read or write outside a buffer, in a misaligned head
// or tail for instance, stops the program.  It also compares every result with a plain loop.  No device is involved.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DVFI_SCENE_HOST \
//       -I fusion-method-for-video-frame-interpolation_amd/csrc tools/scene_host_check.cpp -o scene_host_check && ./scene_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vfi_scene_body.h"

#if defined(__SANITIZE_ADDRESS__)
#define VFI_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define VFI_ASAN 1
#endif
#endif
#ifdef VFI_ASAN
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

namespace {

unsigned rnd_state = 12345u;
unsigned char rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return (unsigned char)(rnd_state >> 24); }

// malloc(n + off) ends exactly at the last byte; the `off` bytes in front (malloc aligns to 16, so `off` is the buffer's
// misalignment) are poisoned by hand, which the sanitizer honours in whole 8-byte granules: an access past the last byte is
// reported exactly, one before the first byte from the previous 8-byte boundary down
struct Exact {
    unsigned char *raw, *p;
    int off;
    Exact(long long n, int off_) : raw(static_cast<unsigned char *>(malloc((size_t)(n + off_)))), p(raw + off_), off(off_) {
        POISON(raw, off);
    }
    ~Exact() { UNPOISON(raw, off); free(raw); }
};

int failures = 0;

void check_sad(long long n, int oa, int ob, int blocks, int fill) {
    Exact A(n, oa), B(n, ob);
    for (long long i = 0; i < n; ++i) {
        A.p[i] = fill == 0 ? rnd() : (fill == 1 ? 77 : 0);
        B.p[i] = fill == 0 ? rnd() : (fill == 1 ? 77 : 255);
    }
    unsigned long long want = 0, got = 0;
    for (long long i = 0; i < n; ++i) want += (unsigned long long)abs((int)A.p[i] - (int)B.p[i]);
    const long long T = 256ll * blocks;
    for (long long g = 0; g < T; ++g) got += vfi_scene::sad_partial(A.p, B.p, n, g, T);
    if (got != want) {
        ++failures;
        printf("sad n=%lld offsets (%d,%d) blocks=%d fill=%d: got %llu want %llu\n", n, oa, ob, blocks, fill, got, want);
    }
}

void check_copy(long long n, int od, int os, int blocks) {
    Exact D(n, od), S(n, os);
    std::vector<unsigned char> mark((size_t)n), final((size_t)n);
    for (long long i = 0; i < n; ++i) { S.p[i] = rnd(); mark[(size_t)i] = final[(size_t)i] = (unsigned char)~S.p[i]; }
    std::vector<int> writes((size_t)n, 0);
    const long long T = 256ll * blocks;
    for (long long g = 0; g < T; ++g) {                       // a written byte is src's, which differs from the mark
        memcpy(D.p, mark.data(), (size_t)n);
        vfi_scene::copy_partial(D.p, S.p, n, g, T);
        for (long long i = 0; i < n; ++i)
            if (D.p[i] != mark[(size_t)i]) { ++writes[(size_t)i]; final[(size_t)i] = D.p[i]; }
    }
    memcpy(D.p, final.data(), (size_t)n);
    bool ok = memcmp(D.p, S.p, (size_t)n) == 0;
    for (long long i = 0; i < n; ++i) ok = ok && writes[(size_t)i] == 1;
    if (!ok) {
        ++failures;
        printf("copy n=%lld offsets (%d,%d) blocks=%d: wrong bytes or a byte with other than one writer\n", n, od, os, blocks);
    }
}

}  // namespace

int main() {
    const long long sad_n[] = {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 4097, 64 * 96, 8192 * 3 + 5};
    const long long copy_n[] = {1, 2, 3, 15, 16, 17, 31, 33, 4099, 64 * 96 * 3 / 2};
    int cases = 0;
    for (long long n : sad_n)
        for (int oa = 0; oa < 17; ++oa)
            for (int ob : {0, 1, 2, 3, 4, 8, 15, oa})
                for (int blocks : {1, 2, 3})
                    for (int fill = 0; fill < 3; ++fill, ++cases) check_sad(n, oa, ob, blocks, fill);
    for (long long n : copy_n)
        for (int od = 0; od < 17; ++od)
            for (int os : {0, 1, 2, 3, 4, 8, 12, 15, od})
                for (int blocks : {1, 2}) { check_copy(n, od, os, blocks); ++cases; }
    // the decision, where unsigned wrap would get it wrong
    struct { unsigned long long s, p, m; bool cut; } d[] = {
        {100, 0, 100, true}, {100, 0, 101, false}, {100, 30, 70, true}, {100, 30, 71, false}, {30, 100, 30, true},
        {30, 100, 31, false}, {100, 250, 100, true}, {100, 250, 101, false}, {5, 5, 0, true}, {5, 5, 1, false},
        {0, 0, 0, true}, {~0ull, 0, ~0ull, true}, {1, ~0ull, 2, false}};
    for (auto &c : d) {
        ++cases;
        if (vfi_scene::is_cut(c.s, c.p, c.m) != c.cut) { ++failures; printf("is_cut(%llu, %llu, %llu) != %d\n", c.s, c.p, c.m, (int)c.cut); }
    }
    printf("scene_host_check: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
