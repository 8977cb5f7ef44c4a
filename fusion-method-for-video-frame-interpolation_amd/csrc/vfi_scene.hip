// Clip I/O: scene cuts decided on the device.  DESIGN.md section 31.
//   vfi_luma_sad    sum of absolute byte differences of two luma planes, exact, into one 64-bit device word
//   vfi_frame_pick  reads that word and the previous pair's, decides "cut" in every thread, and on a cut replaces the
//                   encoded frame by the bytes of an original; otherwise it writes nothing but the flag
// The host never sees the statistic or the decision while it enqueues: both stay in device words on the pair's stream.
// The address arithmetic of both kernels lives in vfi_scene_body.h, which also compiles as host C++.
#include "vfi_common.h"
#include "vfi_scene_body.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr long long kSadBytesPerThread = 32;      // two 16-byte segments of each plane per thread below the block cap

// Workgroups for n bytes at `per` bytes a thread, 1 ... kMaxBlocks; the threads stride over the rest.
int blocks_for(long long n, long long per) {
    const long long b = (n + kThreads * per - 1) / (kThreads * per);
    return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// 32-bit accumulator per thread: a thread adds fewer than n / T + 18 bytes of at most 255.  Below the block cap
// T >= n / 32, so that is < 50 bytes; at the cap T = 2^18 and n < 2^31 give < 8210 bytes, 2.1e6 per thread, 1.4e8 per
// wave: both far inside 2^32.  Waves are combined in 64 bits, and the workgroup adds one 64-bit integer to the word, so
// the sum is exact and the same bits in any order.
__global__ __launch_bounds__(kThreads) void luma_sad_kernel(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b,
                                                            long long n, unsigned long long *__restrict__ sad) {
    __shared__ unsigned long long part[kThreads / vfi::kWave];
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x, T = (long long)gridDim.x * kThreads;
    unsigned acc = vfi_scene::sad_partial(a, b, n, g, T);
#pragma unroll
    for (int o = vfi::kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, vfi::kWave);
    if ((threadIdx.x & (vfi::kWave - 1)) == 0) part[threadIdx.x / vfi::kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < kThreads / vfi::kWave; ++k) sum += part[k];
        atomicAdd(sad, sum);
    }
}

__global__ __launch_bounds__(kThreads) void frame_pick_kernel(unsigned char *__restrict__ dst, const unsigned char *__restrict__ src,
                                                              long long nbytes, const unsigned long long *__restrict__ sad,
                                                              const unsigned long long *__restrict__ sad_prev,
                                                              unsigned long long min_sad, int *__restrict__ cut) {
    const bool is_cut = vfi_scene::is_cut(*sad, sad_prev ? *sad_prev : 0ull, min_sad);
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (cut && g == 0) *cut = is_cut ? 1 : 0;
    if (!is_cut) return;
    vfi_scene::copy_partial(dst, src, nbytes, g, (long long)gridDim.x * kThreads);
}

int check_bytes(const char *who, bool pointers, long long n) {
    VFI_REQUIRE(pointers, VFI_ERR_INVALID_ARG, "%s: null pointer", who);
    VFI_REQUIRE(n > 0, VFI_ERR_INVALID_ARG, "%s: bad size %lld", who, n);
    VFI_REQUIRE(n < (1ll << 31), VFI_ERR_UNSUPPORTED, "%s: %lld bytes is 2^31 or more", who, n);
    return VFI_OK;
}

}  // namespace

extern "C" int vfi_luma_sad(const unsigned char *a, const unsigned char *b, long long n, unsigned long long *sad,
                            vfi_stream_t stream) {
    if (int e = check_bytes("vfi_luma_sad", a && b && sad, n)) return e;
    hipStream_t s = vfi::as_stream(stream);
    const hipError_t e = hipMemsetAsync(sad, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return vfi::fail(VFI_ERR_LAUNCH, "vfi_luma_sad: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(luma_sad_kernel, dim3(blocks_for(n, kSadBytesPerThread)), dim3(kThreads), 0, s, a, b, n, sad);
    return vfi::check_launch("vfi_luma_sad");
}

extern "C" int vfi_frame_pick(unsigned char *dst, const unsigned char *src, long long nbytes, const unsigned long long *sad,
                              const unsigned long long *sad_prev, unsigned long long min_sad, int *cut, vfi_stream_t stream) {
    if (int e = check_bytes("vfi_frame_pick", dst && src && sad, nbytes)) return e;
    hipLaunchKernelGGL(frame_pick_kernel, dim3(blocks_for(nbytes, 16)), dim3(kThreads), 0, vfi::as_stream(stream), dst, src,
                       nbytes, sad, sad_prev, min_sad, cut);
    return vfi::check_launch("vfi_frame_pick");
}
