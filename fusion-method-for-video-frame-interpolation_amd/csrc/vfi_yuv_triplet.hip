// Training input side, from clips: everything between "the Y'CbCr frames of a batch's triplets are on the device" and "the
// tensors a training step takes", in one launch -- vfi_yuv_to_rgb's decode of each frame followed by
// vfi_triplet_batch_prepare's crop, flips and slot choice, without the whole-frame intermediates: only the blocks of the
// frame's grid that intersect a sample's crop are decoded, straight into the batch tensors.
// A thread owns one block of the frame's own grid (2 x 4 luma pixels in 4:2:0, 1 x 4 in 4:4:4), the ownership of
// yuv_to_rgb_kernel, and decodes it with the same decode_block (vfi_yuv_pixel.h); it then stores only its pixels inside
// the crop, at their flipped positions.  Streaming pass: no LDS, no atomics, one writer per float.  The per-thread body and
// all its index arithmetic are in vfi_yuv_triplet_body.h.
#include "vfi_common.h"
#include "vfi_yuv_triplet_body.h"

namespace {

using vfi::ceil_div;
using namespace vfi_yuv;

// grid: x = blocks of the frame's grid inside the largest crop span of the launch's samples (256 per workgroup),
// y = 3 * sample-in-chunk + source frame
template <bool S420, bool LEFT>
__global__ __launch_bounds__(256) void yuv_triplet_batch_prepare_kernel(
    const unsigned char *__restrict__ src, long long frame_stride, YuvCoef k, YtParams prm, int b0, float *__restrict__ rgb,
    long long rgb_slot, long long rgb_batch, float *__restrict__ lab, long long lab_slot, long long lab_batch, int Hs, int Ws, int h,
    int w) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int bl = blockIdx.y / 3, frame = blockIdx.y - 3 * bl, b = b0 + bl;
    triplet_thread<S420, LEFT>(src + ((size_t)b * 3 + frame) * (size_t)frame_stride, Hs, Ws, k, prm.v[bl][0], prm.v[bl][1],
                               prm.v[bl][2], frame, g, rgb ? rgb + (size_t)b * rgb_batch : nullptr, rgb_slot,
                               lab ? lab + (size_t)b * lab_batch : nullptr, lab_slot, h, w);
}

}  // namespace

extern "C" int vfi_yuv_triplet_batch_prepare(const unsigned char *src, long long frame_stride, const int *format, const int *params,
                                             float *rgb, long long rgb_slot_stride, long long rgb_batch_stride, float *lab,
                                             long long lab_slot_stride, long long lab_batch_stride, int B, int Hs, int Ws, int h, int w,
                                             vfi_stream_t stream) {
    const char *who = "vfi_yuv_triplet_batch_prepare";
    VFI_REQUIRE(src && format && params, VFI_ERR_INVALID_ARG, "%s: null pointer", who);
    VFI_REQUIRE(rgb || lab, VFI_ERR_INVALID_ARG, "%s: both outputs are NULL", who);
    VFI_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && h > 0 && w > 0, VFI_ERR_INVALID_ARG, "%s: bad sizes", who);
    VFI_REQUIRE(format[0] == VFI_YUV_420 || format[0] == VFI_YUV_444, VFI_ERR_INVALID_ARG, "%s: unknown subsampling %d", who, format[0]);
    VFI_REQUIRE(format[1] == VFI_YUV_SITING_CENTRE || format[1] == VFI_YUV_SITING_LEFT, VFI_ERR_INVALID_ARG, "%s: unknown chroma siting %d", who, format[1]);
    VFI_REQUIRE(format[2] == VFI_YUV_BT709 || format[2] == VFI_YUV_BT601, VFI_ERR_INVALID_ARG, "%s: unknown matrix %d", who, format[2]);
    VFI_REQUIRE(format[3] == VFI_YUV_LIMITED || format[3] == VFI_YUV_FULL, VFI_ERR_INVALID_ARG, "%s: unknown range %d", who, format[3]);
    const bool s420 = format[0] == VFI_YUV_420, left = format[1] == VFI_YUV_SITING_LEFT;
    VFI_REQUIRE(!s420 || (Hs % 2 == 0 && Ws % 2 == 0), VFI_ERR_SHAPE, "%s: 4:2:0 needs even sizes, got %dx%d", who, Hs, Ws);
    VFI_REQUIRE((long long)Hs * Ws <= (1ll << 28), VFI_ERR_UNSUPPORTED, "%s: source %dx%d too large", who, Hs, Ws);
    VFI_REQUIRE(h <= Hs && w <= Ws, VFI_ERR_INVALID_ARG, "%s: crop %dx%d larger than the source %dx%d", who, h, w, Hs, Ws);
    const long long block = 3ll * h * w;
    VFI_REQUIRE(!rgb || (rgb_slot_stride >= block && rgb_batch_stride >= block), VFI_ERR_INVALID_ARG,
                "%s: rgb strides (%lld, %lld) below a sample's %lld floats", who, rgb_slot_stride, rgb_batch_stride, block);
    VFI_REQUIRE(!lab || (lab_slot_stride >= block && lab_batch_stride >= block), VFI_ERR_INVALID_ARG,
                "%s: lab strides (%lld, %lld) below a sample's %lld floats", who, lab_slot_stride, lab_batch_stride, block);
    const long long frame_bytes = (long long)Hs * Ws + 2 * (s420 ? (long long)(Hs / 2) * (Ws / 2) : (long long)Hs * Ws);
    VFI_REQUIRE(frame_stride >= frame_bytes, VFI_ERR_INVALID_ARG, "%s: frame stride %lld below the frame's %lld bytes", who,
                frame_stride, frame_bytes);
    for (int b = 0; b < B; ++b) {      // before anything is enqueued: a refused call writes nothing
        const int i = params[3 * b], j = params[3 * b + 1], flags = params[3 * b + 2];
        VFI_REQUIRE(i >= 0 && i <= Hs - h, VFI_ERR_INVALID_ARG, "%s: sample %d: crop rows %d + %d leave the %d source rows", who, b, i, h, Hs);
        VFI_REQUIRE(j >= 0 && j <= Ws - w, VFI_ERR_INVALID_ARG, "%s: sample %d: crop columns %d + %d leave the %d source columns", who, b, j, w, Ws);
        VFI_REQUIRE(flags >= 0 && flags < 8, VFI_ERR_INVALID_ARG, "%s: sample %d: flags %d (bits 0-2 only)", who, b, flags);
    }
    const YuvCoef k = make_coef(format[2], format[3]);
    hipStream_t s = vfi::as_stream(stream);
    for (int b0 = 0; b0 < B; b0 += kYtChunk) {
        const int nb = B - b0 < kYtChunk ? B - b0 : kYtChunk;
        YtParams prm = {};
        int most = 1;                  // only blocks that intersect a crop are launched: the largest span of the chunk
        for (int b = 0; b < nb; ++b) {
            for (int q = 0; q < 3; ++q) prm.v[b][q] = params[3 * (b0 + b) + q];
            const int n = block_count(block_span(prm.v[b][0], prm.v[b][1], h, w, s420 ? 2 : 1));
            most = n > most ? n : most;
        }
        const dim3 grid(ceil_div(most, 256), 3 * nb), block_dim(256);
        if (!s420)
            hipLaunchKernelGGL((yuv_triplet_batch_prepare_kernel<false, false>), grid, block_dim, 0, s, src, frame_stride, k, prm, b0, rgb,
                               rgb_slot_stride, rgb_batch_stride, lab, lab_slot_stride, lab_batch_stride, Hs, Ws, h, w);
        else if (left)
            hipLaunchKernelGGL((yuv_triplet_batch_prepare_kernel<true, true>), grid, block_dim, 0, s, src, frame_stride, k, prm, b0, rgb,
                               rgb_slot_stride, rgb_batch_stride, lab, lab_slot_stride, lab_batch_stride, Hs, Ws, h, w);
        else
            hipLaunchKernelGGL((yuv_triplet_batch_prepare_kernel<true, false>), grid, block_dim, 0, s, src, frame_stride, k, prm, b0, rgb,
                               rgb_slot_stride, rgb_batch_stride, lab, lab_slot_stride, lab_batch_stride, Hs, Ws, h, w);
    }
    return vfi::check_launch("vfi_yuv_triplet_batch_prepare");
}
