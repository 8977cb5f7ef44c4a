// Training input side: everything between "the decoded uint8 frames of a batch are on the device" and "the tensors a
// training step takes", in one launch (reference src/train/datareader.py:45-69 on the host with PIL / torchvision, then
// src/train/trainer.py:115-121: float upload, `preprocess` = rgb2lab per slot, and the `torch.cat` of :103).
//   crop (i, j, h, w) -> hflip -> vflip of each of the three frames of a sample, the temporal swap as a choice of output
//   slot, uint8 -> float32 / 255, and the scaled Lab of rgb2lab_kernel (vfi_image.hip) of the same registers.
// One thread owns four consecutive output pixels of one row of one frame: it reads their 12 source bytes once and writes the
// six output planes (r, g, b, L, a, b) from them, as float4 where the row length and the pointers allow.
#include "vfi_common.h"

namespace {

using vfi::ceil_div;

// v / 255 in IEEE float32, folded by the host compiler: the device never divides, so the rgb output is torch's
// `uint8.float() / 255` bit for bit whatever the device's division expands to.
struct U8Table { float v[256]; };
constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int i = 0; i < 256; ++i) t.v[i] = (float)i / 255.0f;
    return t;
}
__constant__ U8Table kU8 = make_u8_table();

constexpr int kTbChunk = 64;       // samples per launch: their parameters travel as a kernel argument (768 bytes)
constexpr int kTbPix = 4;          // pixels per thread
struct TripletParams { int v[kTbChunk][3]; };   // (crop row i, crop column j, flags: 1 hflip, 2 vflip, 4 temporal swap)

// the formulas of rgb2lab_kernel (vfi_image.hip), which stays as it is; the compiler may contract them differently here
__device__ __forceinline__ void lab_of(const float rgb[3], float lab[3]) {
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = rgb[k];
        c[k] = v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
    }
    float x = 0.412453f * c[0] + 0.357580f * c[1] + 0.180423f * c[2];
    float y = 0.212671f * c[0] + 0.715160f * c[1] + 0.072169f * c[2];
    float z = 0.019334f * c[0] + 0.119193f * c[1] + 0.950227f * c[2];
    x /= 0.95047f; z /= 1.08883f;
    auto f = [](float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; };
    const float fx = f(x), fy = f(y), fz = f(z);
    lab[0] = (116.0f * fy - 16.0f) / 100.0f;
    lab[1] = (500.0f * (fx - fy) + 128.0f) / 255.0f;
    lab[2] = (200.0f * (fy - fz) + 128.0f) / 255.0f;
}

// grid: x = groups of four pixels of one frame (h * ceil(w / 4), 256 per workgroup), y = 3 * sample-in-chunk + source frame
__global__ __launch_bounds__(256) void triplet_batch_prepare_kernel(
    const unsigned char *__restrict__ src, TripletParams prm, int b0, float *__restrict__ rgb, long long rgb_slot, long long rgb_batch,
    float *__restrict__ lab, long long lab_slot, long long lab_batch, int Hs, int Ws, int h, int w, int vec_rgb, int vec_lab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = kU8.v[threadIdx.x];
    __syncthreads();
    const int gw = ceil_div(w, kTbPix);
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= gw * h) return;                                  // (no barrier below)
    const int y = g / gw, x0 = (g - y * gw) * kTbPix;
    const int bl = blockIdx.y / 3, frame = blockIdx.y - 3 * bl, b = b0 + bl;
    const int ci = prm.v[bl][0], cj = prm.v[bl][1], flags = prm.v[bl][2];
    const bool hflip = flags & 1, vflip = flags & 2, swap = flags & 4;
    // slots: [first frame, last frame, middle frame] after the swap
    const int slot = frame == 1 ? 2 : ((frame == 2) != swap ? 1 : 0);
    const int nvalid = min(kTbPix, w - x0);
    const int sy = ci + (vflip ? h - 1 - y : y);
    const unsigned char *row = src + (((size_t)b * 3 + frame) * Hs + sy) * (size_t)Ws * 3;
    float px[kTbPix][3];
#pragma unroll
    for (int k = 0; k < kTbPix; ++k) {
        const int x = x0 + k;
        const int sx = cj + (hflip ? w - 1 - x : x);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[k][c] = k < nvalid ? lut[row[(size_t)sx * 3 + c]] : 0.0f;
    }
    const size_t hw = (size_t)h * w, at = (size_t)y * w + x0;
    if (rgb) {
        float *d = rgb + (size_t)slot * rgb_slot + (size_t)b * rgb_batch + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (vec_rgb) {                                     // (w % 4 == 0: every group is whole)
                *reinterpret_cast<float4 *>(d + c * hw) = make_float4(px[0][c], px[1][c], px[2][c], px[3][c]);
            } else {
#pragma unroll
                for (int k = 0; k < kTbPix; ++k)
                    if (k < nvalid) d[c * hw + k] = px[k][c];
            }
        }
    }
    if (lab) {
        float q[kTbPix][3];
#pragma unroll
        for (int k = 0; k < kTbPix; ++k) lab_of(px[k], q[k]);
        float *d = lab + (size_t)slot * lab_slot + (size_t)b * lab_batch + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (vec_lab) {
                *reinterpret_cast<float4 *>(d + c * hw) = make_float4(q[0][c], q[1][c], q[2][c], q[3][c]);
            } else {
#pragma unroll
                for (int k = 0; k < kTbPix; ++k)
                    if (k < nvalid) d[c * hw + k] = q[k][c];
            }
        }
    }
}

// float4 stores need every plane row start on 16 bytes: the base, both strides and the row length
bool vectorisable(const float *p, long long slot, long long batch, int w) {
    return p && w % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && slot % 4 == 0 && batch % 4 == 0;
}

}  // namespace

extern "C" int vfi_triplet_batch_prepare(const unsigned char *src, const int *params, float *rgb, long long rgb_slot_stride,
                                         long long rgb_batch_stride, float *lab, long long lab_slot_stride,
                                         long long lab_batch_stride, int B, int Hs, int Ws, int h, int w, vfi_stream_t stream) {
    VFI_REQUIRE(src && params, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: null pointer");
    VFI_REQUIRE(rgb || lab, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: both outputs are NULL");
    VFI_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && h > 0 && w > 0, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: bad sizes");
    VFI_REQUIRE(h <= Hs && w <= Ws, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: crop %dx%d larger than the source %dx%d", h, w, Hs, Ws);
    VFI_REQUIRE((long long)Hs * Ws <= (1ll << 28), VFI_ERR_UNSUPPORTED, "vfi_triplet_batch_prepare: source %dx%d too large", Hs, Ws);
    const long long block = 3ll * h * w;
    VFI_REQUIRE(!rgb || (rgb_slot_stride >= block && rgb_batch_stride >= block), VFI_ERR_INVALID_ARG,
                "vfi_triplet_batch_prepare: rgb strides (%lld, %lld) below a sample's %lld floats", rgb_slot_stride, rgb_batch_stride, block);
    VFI_REQUIRE(!lab || (lab_slot_stride >= block && lab_batch_stride >= block), VFI_ERR_INVALID_ARG,
                "vfi_triplet_batch_prepare: lab strides (%lld, %lld) below a sample's %lld floats", lab_slot_stride, lab_batch_stride, block);
    for (int b = 0; b < B; ++b) {      // before anything is enqueued: a refused call writes nothing
        const int i = params[3 * b], j = params[3 * b + 1], flags = params[3 * b + 2];
        VFI_REQUIRE(i >= 0 && i <= Hs - h, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: sample %d: crop rows %d + %d leave the %d source rows", b, i, h, Hs);
        VFI_REQUIRE(j >= 0 && j <= Ws - w, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: sample %d: crop columns %d + %d leave the %d source columns", b, j, w, Ws);
        VFI_REQUIRE(flags >= 0 && flags < 8, VFI_ERR_INVALID_ARG, "vfi_triplet_batch_prepare: sample %d: flags %d (bits 0-2 only)", b, flags);
    }
    const int vec_rgb = vectorisable(rgb, rgb_slot_stride, rgb_batch_stride, w);
    const int vec_lab = vectorisable(lab, lab_slot_stride, lab_batch_stride, w);
    const int groups = ceil_div(w, kTbPix) * h;
    hipStream_t s = vfi::as_stream(stream);
    for (int b0 = 0; b0 < B; b0 += kTbChunk) {
        const int nb = B - b0 < kTbChunk ? B - b0 : kTbChunk;
        TripletParams prm = {};
        for (int b = 0; b < nb; ++b)
            for (int k = 0; k < 3; ++k) prm.v[b][k] = params[3 * (b0 + b) + k];
        hipLaunchKernelGGL(triplet_batch_prepare_kernel, dim3(ceil_div(groups, 256), 3 * nb), dim3(256), 0, s, src, prm, b0, rgb,
                           rgb_slot_stride, rgb_batch_stride, lab, lab_slot_stride, lab_batch_stride, Hs, Ws, h, w, vec_rgb, vec_lab);
    }
    return vfi::check_launch("vfi_triplet_batch_prepare");
}
