// Per-thread body of the training-side crop decoder (vfi_yuv_triplet.hip): everything that computes an address.  The block
// and crop index arithmetic is plain functions of integers -- which blocks of the frame's grid a crop launches, which of a
// block's pixels are inside, where they land after the flips, which path a store takes -- and triplet_thread puts them
// together around decode_block (vfi_yuv_pixel.h).  The text also compiles as host C++ with VFI_YUV_HOST defined, where a
// stand-alone program walks it thread by thread over exact-size heap buffers under AddressSanitizer
// (tools/yuv_triplet_host_check.cpp).  The launches and the argument checks stay in vfi_yuv_triplet.hip.
#pragma once
#include "vfi_yuv_pixel.h"

namespace vfi_yuv {

constexpr int kYtChunk = 64;            // samples per launch: their parameters travel as a kernel argument (768 bytes)
struct YtParams { int v[kYtChunk][3]; };   // (crop row i, crop column j, flags: 1 hflip, 2 vflip, 4 temporal swap)

struct alignas(16) Float4 { float x, y, z, w; };      // one dwordx4 store

// The blocks of the frame's grid (R luma rows x 4 luma columns, R = 2 in 4:2:0) that intersect the crop of h x w at (i, j):
// block rows by0 ... by0 + nby - 1, block columns bx0 ... bx0 + nbx - 1.
struct BlockSpan { int by0, nby, bx0, nbx; };

VFI_YUV_FN BlockSpan block_span(int i, int j, int h, int w, int R) {
    BlockSpan s;
    s.by0 = i / R;
    s.nby = (i + h - 1) / R - s.by0 + 1;
    s.bx0 = j / kDecPix;
    s.nbx = (j + w - 1) / kDecPix - s.bx0 + 1;
    return s;
}

// threads a (sample, frame) needs; a launch's x dimension covers the largest count among its samples
VFI_YUV_FN int block_count(const BlockSpan &s) { return s.nby * s.nbx; }

// thread g of a (sample, frame): its block (chroma row, first luma column), false where the sample has fewer blocks
VFI_YUV_FN bool block_of(const BlockSpan &s, int g, int *ry, int *x0) {
    if (g >= block_count(s)) return false;
    const int q = g / s.nbx;
    *ry = s.by0 + q;
    *x0 = (s.bx0 + (g - q * s.nbx)) * kDecPix;
    return true;
}

// source row sy is inside the crop rows [i, i + h); likewise the columns
VFI_YUV_FN bool row_inside(int sy, int i, int h) { return sy >= i && sy < i + h; }
// the block's columns inside the crop columns [j, j + w): c_lo <= c < c_hi, 0 <= c_lo, c_hi <= 4
VFI_YUV_FN void cols_inside(int x0, int j, int w, int *c_lo, int *c_hi) {
    *c_lo = imax(j - x0, 0);
    *c_hi = imin(j + w - x0, kDecPix);
}

// where source pixel (sy, sx) lands in the h x w output: the crop first, then hflip, then vflip
VFI_YUV_FN int out_row(int sy, int i, int h, bool vflip) { return vflip ? h - 1 - (sy - i) : sy - i; }
VFI_YUV_FN int out_col(int sx, int j, int w, bool hflip) { return hflip ? w - 1 - (sx - j) : sx - j; }

// slots: [first frame, last frame, middle frame] after the temporal swap
VFI_YUV_FN int slot_of(int frame, bool swap) { return frame == 1 ? 2 : ((frame == 2) != swap ? 1 : 0); }

// one float4 where the block's four outputs are whole, in order and on 16 bytes; one float at a time otherwise
VFI_YUV_FN bool store_is_vector(int c_lo, int c_hi, bool hflip, const float *first) {
    return !hflip && c_lo == 0 && c_hi == kDecPix && aligned(first, 15);
}

// One plane row of a block: v[c_lo ... c_hi - 1] to row[out_col(x0 + c)].
VFI_YUV_FN void store_row(float *__restrict__ row, int x0, int j, int w, bool hflip, int c_lo, int c_hi, const float v[kDecPix]) {
    if (c_lo >= c_hi) return;
    float *first = row + out_col(x0 + c_lo, j, w, false);
    if (store_is_vector(c_lo, c_hi, hflip, first)) {
        Float4 q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<Float4 *>(first) = q;
    } else {
#pragma unroll
        for (int c = 0; c < kDecPix; ++c)
            if (c >= c_lo && c < c_hi) row[out_col(x0 + c, j, w, hflip)] = v[c];
    }
}

// Thread g of source frame `frame` (0, 1, 2) of one sample.  `src` is that frame; rgb / lab are the sample's (3, h, w)
// blocks of slot 0 (NULL: not wanted), *_slot the distance to the next slot in floats.
template <bool S420, bool LEFT>
VFI_YUV_FN void triplet_thread(const unsigned char *__restrict__ src, int Hs, int Ws, const YuvCoef &k, int ci, int cj, int flags,
                               int frame, int g, float *__restrict__ rgb, long long rgb_slot, float *__restrict__ lab,
                               long long lab_slot, int h, int w) {
    constexpr int R = S420 ? 2 : 1;
    int ry, x0;
    if (!block_of(block_span(ci, cj, h, w, R), g, &ry, &x0)) return;
    const bool hflip = flags & 1, vflip = flags & 2, swap = flags & 4;
    const int slot = slot_of(frame, swap);
    float px[R][kDecPix][3];
    decode_block<S420, LEFT>(src, Hs, Ws, k, ry, x0, px);
    int c_lo, c_hi;
    cols_inside(x0, cj, w, &c_lo, &c_hi);
    const size_t hw = (size_t)h * w;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int sy = ry * R + r;
        if (!row_inside(sy, ci, h)) continue;
        const size_t at = (size_t)out_row(sy, ci, h, vflip) * w;
        if (rgb) {
            float *d = rgb + (size_t)slot * rgb_slot + at;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v[kDecPix] = {px[r][0][c], px[r][1][c], px[r][2][c], px[r][3][c]};
                store_row(d + c * hw, x0, cj, w, hflip, c_lo, c_hi, v);
            }
        }
        if (lab) {
            float q[kDecPix][3];
#pragma unroll
            for (int i = 0; i < kDecPix; ++i) lab_of(px[r][i], q[i]);
            float *d = lab + (size_t)slot * lab_slot + at;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v[kDecPix] = {q[0][c], q[1][c], q[2][c], q[3][c]};
                store_row(d + c * hw, x0, cj, w, hflip, c_lo, c_hi, v);
            }
        }
    }
}

}  // namespace vfi_yuv
