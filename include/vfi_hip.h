/*
 * vfi_hip.h -- C ABI of libvfi_hip.so, the MI355X (gfx950) implementation of the
 * per-frame inference hot path of "Fusion Method for Video Frame Interpolation":
 * steerable-pyramid phase decomposition + PhaseNet, AdaCoF deformable sampling and
 * the FusionNet blend.
 *
 * Conventions (every entry point):
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - Returns VFI_OK (0) or a negative vfi_status; never throws, never exits.
 *     vfi_status_string() names a code, vfi_last_error() gives the detail of the last
 *     failure on the calling thread.
 *   - Every data pointer is a DEVICE pointer owned by the caller (the Python host passes
 *     torch-allocated HBM); tensors are dense fp32, NCHW unless stated otherwise.
 *   - `stream` is a hipStream_t passed as void* (the host passes torch's current HIP
 *     stream).  Calls only enqueue work; none synchronises the device, allocates or
 *     frees device memory, so a sequence of calls can be captured into a hipGraph.
 *     Workspace is caller-provided or owned by an explicit plan object.
 *   - Process-wide state is limited to idempotent per-device launch setup (the dynamic-LDS
 *     attribute of three kernels, the CU count), tuning switches read once from the
 *     environment (VFI_CONV_WINOGRAD, VFI_CONV_WINOGRAD4, VFI_CONV_STREAM1X1, VFI_ADACOF_VARIANT, VFI_ADACOF_MARGIN; VFI_CONV_WINOGRAD4M and VFI_MEDIAN_PATH at every call) and the
 *     thread-local last-error string; everything else lives in explicit plan objects,
 *     whose tables are immutable after creation and whose workspace belongs to ONE stream
 *     at a time (frames in flight on different streams use different plans).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef VFI_HIP_H
#define VFI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFI_ABI_VERSION 1

typedef void *vfi_stream_t; /* hipStream_t */

typedef enum vfi_status {
    VFI_OK = 0,
    VFI_ERR_INVALID_ARG = -1, /* null pointer, non-positive size, unsupported value */
    VFI_ERR_SHAPE = -2,       /* shape relation violated (mirrors the reference's asserts) */
    VFI_ERR_LAUNCH = -3,      /* HIP launch / runtime error */
    VFI_ERR_UNSUPPORTED = -4, /* valid request this build has no kernel for */
    VFI_ERR_FFT = -5,         /* reserved (round 1 linked an FFT library; the transforms are hand-written kernels now) */
    VFI_ERR_NOMEM = -6        /* host or device allocation failed (plan creation only) */
} vfi_status;

int vfi_abi_version(void);
const char *vfi_status_string(int status);
const char *vfi_last_error(void);
/* Test aid (no reference counterpart): fills the LDS of every CU with NaNs, so that the kernels enqueued next on `stream`
 * start on NaN-filled LDS -- a kernel whose result depends on LDS it has not written itself then shows deterministically
 * (tests/test_pyramid_gpu.py::test_results_do_not_depend_on_stale_lds). */
int vfi_debug_poison_lds(vfi_stream_t stream);
/* Test aid (no reference counterpart), process-global, affects later calls only (tests/test_conv_walk_gpu.py).
 *   winograd4_mode  -1: as configured (VFI_CONV_WINOGRAD4 or the default); 0, 1, 2: as that variable -- 0 = every 3x3
 *                   layer on the F(2x2) Winograd kernel, 1 = the cost model, 2 = every eligible layer on the F(4x4) kernels.
 *                   vfi_conv2d_algo answers accordingly.
 *   max_workgroups  0: no cap; k >= 1: the persistent Winograd kernels are launched with min(grid, k) workgroups, so that a
 *                   small layer gives every workgroup several work items.  Only the launch grid changes -- K split, item
 *                   order and workspace use do not -- so the output bits do not depend on it.
 * Anything else is VFI_ERR_INVALID_ARG and changes nothing.  (-1, 0) restores the library's own behaviour. */
int vfi_debug_conv_override(int winograd4_mode, int max_workgroups);

/* ------------------------------------------------------------------------------------
 * AdaCoF deformable sampling
 * ---------------------------------------------------------------------------------- */

/* Replaces FunctionAdaCoF.forward + kernel_AdaCoF_updateOutput
 * (src/adacof/cupy_module/adacof.py:313-361 and :6-65).
 *   input    (N, C, Hin, Win)   already padded by the caller, as in the reference
 *   weight, offset_i, offset_j  (N, F*F, H, W)
 *   output   (N, C, H, W)
 * Shape relation of adacof.py:326-327 is enforced: Hin - ((F-1)*dilation + 1) == H - 1
 * (same for W), otherwise VFI_ERR_SHAPE.  Sampling semantics are the reference's:
 * (int) truncation of the offsets, each of the four taps clamped to the input
 * independently, bilinear weights from the un-clamped fractional parts. */
int vfi_adacof_forward(const float *input, const float *weight, const float *offset_i,
                       const float *offset_j, float *output, int N, int C, int Hin, int Win,
                       int H, int W, int F, int dilation, vfi_stream_t stream);

/* Replaces FunctionAdaCoF.backward + kernel_AdaCoF_updateGradWeight / ...updateGradAlpha / ...updateGradBeta
 * (src/adacof/cupy_module/adacof.py:364-445 and :67-258) with ONE launch that produces all three gradients.
 *   grad_output (N, C, H, W);  input, weight, offset_i, offset_j as in vfi_adacof_forward
 *   grad_weight, grad_offset_i, grad_offset_j  (N, F*F, H, W), each may be NULL (not produced; at least one
 *   is required).  weight may be NULL when both offset gradients are NULL.
 * Semantics are the reference's (same truncation, per-corner clamps and fractions as the forward; A = (int)alpha
 * carries no gradient), except that the channel sum runs over all C channels (the reference stops at c < 3).
 * Deterministic: every output element is written by exactly one thread.  No input gradient (the reference's is
 * an unfilled zero tensor). */
int vfi_adacof_backward(const float *grad_output, const float *input, const float *weight,
                        const float *offset_i, const float *offset_j,
                        float *grad_weight, float *grad_offset_i, float *grad_offset_j,
                        int N, int C, int Hin, int Win, int H, int W, int F, int dilation,
                        vfi_stream_t stream);

/* One fused pass over both sampling sides of AdaCoFNet.forward
 * (src/fusion_net/fusion_adacofnet.py:195-213; plain variant src/adacof/models/adacofnet.py:195-199):
 *   t1 = AdaCoF(ReplicationPad(frame0), W1, A1, B1);  t2 = AdaCoF(ReplicationPad(frame2), W2, A2, B2)
 *   frame1 = Occ * t1 + (1 - Occ) * t2
 *   mask   = clip(max(sum Var(W1; A1, B1), sum Var(W2; A2, B2)), 0, 20) / 20
 * The replication pad of (F-1)*dilation/2 pixels is folded into the tap clamp, so
 * frame0/frame2 are the UN-padded (N, C, H, W) frames.  w*, a*, b* are (N, F*F, H, W),
 * occ is (N, 1, H, W).  out_t1 / out_t2 / out_mask may be NULL (not produced);
 * out_frame is required.  (F-1)*dilation must be even (as in the reference, where
 * kernel_pad = int((F-1)*dilation/2)). */
int vfi_adacof_fused(const float *frame0, const float *frame2,
                     const float *w1, const float *a1, const float *b1,
                     const float *w2, const float *a2, const float *b2, const float *occ,
                     float *out_t1, float *out_t2, float *out_frame, float *out_mask,
                     int N, int C, int H, int W, int F, int dilation, vfi_stream_t stream);

/* Same computation on PIXEL-INTERLEAVED frames (N, H, W, 4) = (r, g, b, unused), as written by
 * vfi_adacof_prepare(..., rgbx=1): one 16-byte gather per bilinear corner instead of three 4-byte ones
 * (the kernel is bound by gather issue, not by HBM).  Outputs stay planar (N, 3, H, W).
 * weights_are_logits != 0: w1 / w2 are the pre-softmax outputs of Subnet_weight and the channel softmax
 * (fusion_adacofnet.py:56) is folded into the accumulation, so the normalised weights never touch HBM. */
int vfi_adacof_fused_rgbx(const float *frame0_rgbx, const float *frame2_rgbx,
                          const float *w1, const float *a1, const float *b1,
                          const float *w2, const float *a2, const float *b2, const float *occ,
                          float *out_t1, float *out_t2, float *out_frame, float *out_mask,
                          int N, int H, int W, int F, int dilation, int weights_are_logits, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Dense convolution on the fp32 matrix cores (exact fp32: v_mfma_f32_16x16x4_f32 in the Winograd
 * kernels that take the 3x3 layers, v_mfma_f32_32x32x2_f32 in the direct 1x1 / 5x5 kernels)
 * ---------------------------------------------------------------------------------- */

typedef enum vfi_act {
    VFI_ACT_NONE = 0,
    VFI_ACT_RELU = 1,
    VFI_ACT_ELU = 2, /* alpha = 1 */
    VFI_ACT_TANH = 3,
    VFI_ACT_SIGMOID = 4
} vfi_act;

typedef enum vfi_pad { VFI_PAD_ZERO = 0, VFI_PAD_REFLECT = 1 } vfi_pad;

/* Number of floats of the packed weight buffer for an (Cout, Cin, KS, KS) filter bank, -1 on bad arguments.
 * The buffer is opaque to the caller: [round_up(Cin,8)][KS*KS][round_up(Cout,32)] (zero filled) and, for KS = 3,
 * the Winograd F(2x2,3x3) transformed weights G g G^T as [round_up(Cin,8)][4][round_up(Cout,32)][4] behind it. */
long long vfi_conv2d_packed_floats(int Cout, int Cin, int KS);

/* Packs torch-layout (Cout, Cin, KS, KS) weights once at model-load time.  `scale` (Cout) or NULL
 * multiplies each output channel (BatchNorm2d in eval mode folded into the preceding conv:
 * reference src/phase_net/phase_net.py:191-193). */
int vfi_conv2d_pack(const float *w_oihw, const float *scale, float *packed, int Cout, int Cin, int KS,
                    vfi_stream_t stream);

/* y = act(conv2d(x, w) + bias) (+ residual): stride 1, padding (KS-1)/2 in `pad_mode`, KS in {1,3,5}.
 * Replaces every nn.Conv2d (+ following BatchNorm / ReLU / ELU / Tanh / Sigmoid, + the additive U-Net
 * skip) on the path: reference src/phase_net/phase_net.py:190-200, src/fusion_net/fusion_adacofnet.py:18-155,
 * src/fusion_net/fusion_net.py:24-41,56-69.
 * KS = 3 runs Winograd on the fp32 matrix cores -- F(4x4,3x3) (16x64-pixel x 32-channel work items, one workgroup per
 * CU) or F(2x2,3x3) (8x32-pixel items, two per CU, K split for few long items), whichever a cost model of the two kernels
 * (rounds of resident workgroups x time per item, fitted to a per-layer A/B of the 1080p frame) puts ahead;
 * vfi_conv2d_algo tells which kernel a layer gets; same result up to fp32 rounding of the transforms: rms 3e-7 resp.
 * 2e-6 of the output rms, <= 3e-5 resp. 1e-4 at worst on unit-variance data (2.5e-4 on the statistics of trained PhaseNet
 * weights with folded BatchNorm).  Environment (A/B aids): VFI_CONV_WINOGRAD4=0 keeps F(2x2) everywhere, =2 sends every
 * plain 3x3 layer to F(4x4); VFI_CONV_WINOGRAD4M=0 (read at every call) runs F(4x4) on round 3's kernel -- 16 channels per
 * wave, two waves per SIMD; bit-identical outputs -- instead of the 32-channel-per-wave one; VFI_CONV_WINOGRAD=0 selects
 * the direct kernel.  KS = 5: the direct one.  KS = 1: the direct one, except layers with at most 16 output channels on an even
 * number of >= 4096 pixels without a residual (8-byte-aligned operands): a streaming kernel that reads the input once at the HBM
 * rate (vector ALU, fp32 FMA chain over the input channels in order; VFI_CONV_STREAM1X1=0 keeps the direct kernel).
 *   x        (N, Cin, H, W); consecutive samples are x_bstride floats apart, so x may be a channel
 *            slice of a wider tensor (no concat / split copies)
 *   residual NULL or (N, Cout, H, W) with stride res_bstride, added AFTER the activation
 *   y        (N, Cout, H, W) with stride y_bstride
 *   workspace / workspace_floats  optional scratch (NULL / 0 = none).  When the launch would otherwise fill only a
 *            fraction of a round of resident workgroups (deep U-Net levels: few, long workgroups) the channel
 *            loop is split over several workgroups whose partial sums go through the workspace and are reduced
 *            in a fixed order (deterministic).  16 * N*Cout*H*W floats always suffice; results do not depend on
 *            whether a workspace is given beyond fp32 summation order. */
enum { VFI_CONV_ALGO_DIRECT = 0, VFI_CONV_ALGO_WINOGRAD2 = 1, VFI_CONV_ALGO_WINOGRAD4 = 2, VFI_CONV_ALGO_STREAM1X1 = 3 };
/* Which kernel vfi_conv2d / vfi_conv2d_pool2 runs for a layer on the current device (>= 0: VFI_CONV_ALGO_*; < 0: status):
 * direct implicit GEMM, Winograd F(2x2,3x3), Winograd F(4x4,3x3), or the streaming kernel of 1x1 layers with at most 16 output
 * channels (an even number of >= 4096 pixels, no residual; operands assumed 8-byte aligned).  For profiling labels and flop
 * counts: the selection rule lives in the library only. */
int vfi_conv2d_algo(int N, int Cin, int H, int W, int Cout, int KS, int has_residual, int pooled, int act);

int vfi_conv2d(const float *x, long long x_bstride, const float *packed_w, const float *bias,
               const float *residual, long long res_bstride, float *y, long long y_bstride, int N, int Cin,
               int H, int W, int Cout, int KS, int pad_mode, int act, float *workspace,
               long long workspace_floats, vfi_stream_t stream);

/* vfi_conv2d followed by 2x2 / stride-2 pooling of its result (AvgPool2d after every encoder block of the U-Net,
 * src/fusion_net/fusion_adacofnet.py:76-89,116-126; MaxPool2d in FusionNet, src/fusion_net/fusion_net.py:41,59):
 * y as vfi_conv2d (no residual), pooled (N, Cout, H/2, W/2) = pool(y).  For KS = 3 ReLU layers the pooled value is
 * written by the convolution's epilogue (the lane that holds a 2x2 output block averages / maximises it); other
 * layers run the pooling pass afterwards.  Same results as the two calls. */
int vfi_conv2d_pool2(const float *x, long long x_bstride, const float *packed_w, const float *bias, float *y,
                     long long y_bstride, float *pooled, long long pooled_bstride, int is_max, int N, int Cin, int H, int W,
                     int Cout, int KS, int pad_mode, int act, float *workspace, long long workspace_floats,
                     vfi_stream_t stream);

/* conv2d( nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)(x_lowres) ) in one launch: the
 * `Upsample -> Conv2d` pairs of KernelEstimation (src/fusion_net/fusion_adacofnet.py:28-33 and the heads'
 * tails :41-43,53-56,67-70).  x_lowres is (N, Cin, H/2, W/2); H, W are the OUTPUT size (even); the upsampled
 * tensor is never written to HBM (the tile loader interpolates it).  KS = 3, zero padding only. */
int vfi_conv2d_upsample2x(const float *x_lowres, long long x_bstride, const float *packed_w, const float *bias,
                          const float *residual, long long res_bstride, float *y, long long y_bstride, int N,
                          int Cin, int H, int W, int Cout, int KS, int pad_mode, int act, float *workspace,
                          long long workspace_floats, vfi_stream_t stream);

/* conv2d over the virtual concat [ resize(x2) | x[:, prefix_channels:] ]: the first prefix_channels input channels
 * are torch's bilinear resize (align_corners=False) of x2 (N, prefix_channels, Hs, Ws) to (H, W), the remaining
 * Cin - prefix_channels channels are read from x (N, Cin, H, W) -- whose first prefix_channels channels are never
 * touched.  This is PhaseNet's block input `cat(Upsample(feature), phase, amp, Upsample(prediction))`
 * (src/phase_net/phase_net.py:138-141, channels permuted at pack time) without writing the resized maps.
 * KS = 3, Cout % 64 == 0, prefix_channels % 8 == 0. */
int vfi_conv2d_resized_prefix(const float *x, long long x_bstride, const float *x2, long long x2_bstride,
                              int prefix_channels, int Hs, int Ws, const float *packed_w, const float *bias,
                              float *y, long long y_bstride, int N, int Cin, int H, int W, int Cout, int KS,
                              int pad_mode, int act, float *workspace, long long workspace_floats,
                              vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Glue between the convolutions (HBM-bound; batch strides as for vfi_conv2d)
 * ---------------------------------------------------------------------------------- */

/* AdaCoFNet.forward prologue (src/fusion_net/fusion_adacofnet.py:182-193, src/adacof/utility.py:86-87):
 * reflect-pads both (N,3,H,W) frames at the bottom/right to (Hp,Wp) (multiples of 32), writes the padded
 * raw frames pad0/pad2 for the sampler -- planar (N,3,Hp,Wp) when rgbx == 0, pixel-interleaved (N,Hp,Wp,4)
 * when rgbx == 1 (4th float left untouched) -- and x6 = cat(pad0 - mean, pad2 - mean) (N,6,Hp,Wp). */
int vfi_adacof_prepare(const float *frame0, const float *frame2, float *pad0, float *pad2, float *x6, int N,
                       int H, int W, int Hp, int Wp, int rgbx, vfi_stream_t stream);

/* 2x2 / stride-2 pooling, floor output size.  is_max=0: AvgPool2d (fusion_adacofnet.py:76-89);
 * is_max=1: MaxPool2d (src/fusion_net/fusion_net.py:41,59). */
int vfi_pool2(const float *x, long long x_bstride, float *y, long long y_bstride, int N, int C, int H, int W,
              int is_max, vfi_stream_t stream);

/* torch bilinear interpolation to (Hout,Wout): align_corners=1 is nn.Upsample(scale_factor=2,
 * align_corners=True) of fusion_adacofnet.py:30,42,54,68; align_corners=0 is nn.Upsample(size) of
 * src/phase_net/phase_net.py:138-139 and nn.Upsample(scale_factor=2) of fusion_net.py:42.
 * relu_input=1 applies ReLU to the source first and residual (NULL or (N,C,Hout,Wout)) is added
 * to the result: `deconvolution(relu(x)) + s` of fusion_net.py:65-66 in one pass. */
int vfi_resize_bilinear(const float *x, long long x_bstride, const float *residual, long long res_bstride,
                        float *y, long long y_bstride, int N, int C, int Hin, int Win, int Hout, int Wout,
                        int align_corners, int relu_input, vfi_stream_t stream);

/* Tail of `Upsample(x2, bilinear, align_corners=True) -> Conv2d(C, 1, 3, padding=1) -> act` (Subnet_occlusion,
 * fusion_adacofnet.py:68-70) after the channel reduction has been done at LOW resolution: taps_lowres (N,9,Hs,Ws)
 * holds m_t = sum_c w[0][c][t] * x_c (a 1x1 vfi_conv2d with the 3x3 filter's taps as output channels);
 * out (N,1,2Hs,2Ws) = act(bias + sum_t U(m_t) shifted by tap t, zero outside).  Exact by linearity of both maps;
 * replaces a 64->1 conv at full resolution that would waste 31/32 of each matrix-core tile. */
int vfi_upsample2x_tapsum(const float *taps_lowres, float *out, int N, int Hs, int Ws, float bias, int act,
                          vfi_stream_t stream);

/* Softmax over the channel axis of (N,C,HW) (Subnet_weight, fusion_adacofnet.py:56).  In place allowed. */
int vfi_softmax_channels(const float *x, long long x_bstride, float *y, long long y_bstride, int N, int C, int HW,
                         vfi_stream_t stream);

/* dst[n][e] = src[n][e] / div_per_sample[n] * mul for e < count (div_per_sample may be NULL).
 * Slice copies into concat buffers; phase/pi and amplitude/max of PhaseNet.normalize_vals
 * (src/phase_net/phase_net.py:61-70). */
int vfi_affine_slice(const float *src, long long src_bstride, float *dst, long long dst_bstride, int N,
                     long long count, const float *div_per_sample, float mul, vfi_stream_t stream);

/* out_max[n] = max(x[n][0..count)) + eps (phase_net.py:55,69).  workspace_u32: N 32-bit words. */
int vfi_batch_max(const float *x, long long x_bstride, int N, long long count, float eps, float *out_max,
                  void *workspace_u32, vfi_stream_t stream);

/* PhaseNet per-level outputs (phase_net.py:155-168 + reverse_normalize :80-90), pred (N,8,HW) from the
 * block's tanh head, amp_in (N,8,HW) the normalised input amplitudes:
 *   phase_out (N,4,HW) = pred[:,0:4]*pi ; amp_out (N,4,HW) = (b*amp_in[:,4:8] + (1-b)*amp_in[:,0:4])*max_amp[n],
 *   b = (pred[:,4:8]+1)/2. */
int vfi_phasenet_emit(const float *pred, long long pred_bstride, const float *amp_in, long long amp_bstride,
                      const float *max_amp, float *phase_out, float *amp_out, int N, int HW, vfi_stream_t stream);

/* The prediction head of one PhaseNet level in one pass (phase_net.py:149-168, 190-207): pred (N,8,H*W) = tanh(1x1 conv of feat
 * (N,Cin,H*W) with packed_w / bias: the weights of vfi_conv2d_pack for Cout = 8, KS = 1), written out (the next level resizes
 * it), and vfi_phasenet_emit's outputs from the same registers.  Same results as vfi_conv2d(act = tanh) followed by
 * vfi_phasenet_emit, which is what small or odd-sized levels still run. */
int vfi_phasenet_predict(const float *feat, long long feat_bstride, const float *packed_w, const float *bias,
                         const float *amp_in, long long amp_bstride, const float *max_amp, float *pred, long long pred_bstride,
                         float *phase_out, float *amp_out, int N, int Cin, int H, int W, vfi_stream_t stream);

/* A band level's head and the next level's resize in one pass (phase_net.py:138-168): vfi_phasenet_predict's phase_out and
 * amp_out from feat (N,64,H*W), and x_next[:, 0:72] (a channel slice of the next level's block input, N x (>= 72) x Hout x Wout
 * with its batch stride) = bilinear resize, align_corners=False, of [feat 64 | pred 8].  The un-resized pred is not an output.
 * phase_out and amp_out have the bits of vfi_phasenet_predict.  One kernel where vfi_phasenet_predict streams and the target is
 * no smaller than the source: its resized planes evaluate vfi_resize_bilinear's expression and may differ from it in the last
 * bit (fused multiply-adds chosen by the compiler).  Else vfi_phasenet_predict and vfi_resize_bilinear themselves (pred then
 * passes through the head of x_next, so 8*H*W <= 64*Hout*Wout is required). */
int vfi_phasenet_level_tail(const float *feat, long long feat_bstride, const float *packed_w, const float *bias,
                            const float *amp_in, long long amp_bstride, const float *max_amp, float *x_next,
                            long long next_bstride, float *phase_out, float *amp_out, int N, int H, int W, int Hout, int Wout,
                            vfi_stream_t stream);
/* Which launches vfi_phasenet_level_tail takes for these arguments (no GPU call; >= 0: VFI_TAIL_PATH_*, < 0: the status the
 * entry point would return for them): vfi_phasenet_predict and vfi_resize_bilinear, the one-pass kernel with element / 4-byte
 * aligned stores, or the one-pass kernel with 16-byte aligned vector stores (Wout a multiple of 4, x_next and its batch stride
 * 16-byte aligned).  The one-pass kernel runs for an even number of >= 4096 source pixels, 8-byte-aligned feat, amp_in,
 * phase_out, amp_out and batch strides, H <= Hout and W <= Wout.  For tests: the rule lives in the library only, as with
 * vfi_conv2d_algo. */
enum { VFI_TAIL_PATH_TWO_LAUNCHES = 0, VFI_TAIL_PATH_ONE_PASS = 1, VFI_TAIL_PATH_ONE_PASS_VEC = 2 };
int vfi_phasenet_level_tail_path(const float *feat, long long feat_bstride, const float *packed_w, const float *bias,
                                 const float *amp_in, long long amp_bstride, const float *max_amp, const float *x_next,
                                 long long next_bstride, const float *phase_out, const float *amp_out, int N, int H, int W,
                                 int Hout, int Wout);

/* phase_net.py:113-116 + :96-98: low_out (N,HW) = (a*low_in[:,0] + (1-a)*low_in[:,1])*max_low[n], a = (pred+1)/2. */
int vfi_phasenet_emit_low(const float *pred, long long pred_bstride, const float *low_in, long long low_bstride,
                          const float *max_low, float *low_out, int N, int HW, vfi_stream_t stream);

/* The three entry points above for PhaseNet with num_img = 2, 3 or 4 input images (the fusion variants of
 * src/phase_net/phase_net.py:21-35: four images = the two frames and AdaCoF's two warped sides, three = the two frames and
 * AdaCoF's result).  num_img = 2 gives the bits of the entry points above; any other value is VFI_ERR_UNSUPPORTED.
 *
 * vfi_phasenet_emit_n (phase_net.py:155-168 + :80-90): amp_in (N,4*num_img,HW); pred (N,8,HW), or (N,12,HW) for num_img = 3.
 * The first blend as in vfi_phasenet_emit; for num_img = 3 then a second one (phase_net.py:158-162):
 *   amp = fb*amp + (1-fb)*amp_in[:,8:12], fb = (pred[:,8:12]+1)/2, before the multiplication by max_amp[n].
 * For num_img = 4 the planes 8..15 of amp_in are never read (phase_net.py:156). */
int vfi_phasenet_emit_n(const float *pred, long long pred_bstride, const float *amp_in, long long amp_bstride,
                        const float *max_amp, float *phase_out, float *amp_out, int N, int HW, int num_img, vfi_stream_t stream);

/* vfi_phasenet_predict for num_img images (phase_net.py:149-168, 190-207): the prediction map is 64 -> 8, or 64 -> 12 for
 * num_img = 3 (packed_w / bias of vfi_conv2d_pack for that Cout, KS = 1); pred (N,8 or 12,H*W), amp_in (N,4*num_img,H*W).  Same
 * results as vfi_conv2d(act = tanh) followed by vfi_phasenet_emit_n -- bit for bit where both stream -- which is what small or
 * odd-sized levels run. */
int vfi_phasenet_predict_n(const float *feat, long long feat_bstride, const float *packed_w, const float *bias,
                           const float *amp_in, long long amp_bstride, const float *max_amp, float *pred, long long pred_bstride,
                           float *phase_out, float *amp_out, int N, int Cin, int H, int W, int num_img, vfi_stream_t stream);

/* vfi_phasenet_emit_low for num_img images (phase_net.py:113-121 + :96-98): low_in (N,num_img,HW); pred (N,1,HW), or (N,2,HW)
 * for num_img = 3, where low = fa*low + (1-fa)*low_in[:,2], fa = (pred[:,1]+1)/2, follows the first blend.  For num_img = 4
 * the planes 2 and 3 of low_in are never read. */
int vfi_phasenet_emit_low_n(const float *pred, long long pred_bstride, const float *low_in, long long low_bstride,
                            const float *max_low, float *low_out, int N, int HW, int num_img, vfi_stream_t stream);

/* FusionNet tail (fusion_net.py:70-77): y = clamp(base + tanh(x), 0, 1) over `count` floats. */
int vfi_tanh_residual_clamp(const float *x, const float *base, float *y, long long count, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Backward of FusionNet's layers (training, src/fusion_net/train.py + trainer.py:222-260): gradients of
 * src/fusion_net/fusion_net.py:24-41 (convolutions) and :46-77 (forward).  Deterministic: no float atomics; every
 * sum runs in a fixed order, so a call repeats its bits.
 * ---------------------------------------------------------------------------------- */

/* Minimum workspace (floats) of vfi_conv2d_backward_weight for a layer (-1 on bad arguments): one partial slab. */
long long vfi_conv2d_backward_weight_workspace_floats(int Cout, int Cin, int KS);

/* Weight (and bias) gradient of a vfi_conv2d layer, stride 1, KS in {1,3,5}, pad_mode zeros | reflect:
 *   dw (Cout, Cin, KS, KS) plain OIHW: dw[co][ci][ky][kx] = sum_{n,y,x} dy[n,co,y,x] * xpad[n,ci,y+ky,x+kx]
 *   dbias (Cout) = sum_{n,y,x} dy[n,co,y,x], or NULL (not produced)
 * x (N, Cin, H, W) is the layer's input (the padding is resolved while loading, never materialised), dy (N, Cout, H, W)
 * the gradient of its output; batch strides as for vfi_conv2d.  fp32 MFMA GEMM split over the pixels into S partial
 * slabs of `workspace`, summed in slab order by a second pass.  S depends only on the shape and workspace_floats
 * (at least vfi_conv2d_backward_weight_workspace_floats; about 1024 workgroups' worth is used when it fits). */
int vfi_conv2d_backward_weight(const float *x, long long x_bstride, const float *dy, long long dy_bstride, float *dw,
                               float *dbias, int N, int Cin, int H, int W, int Cout, int KS, int pad_mode, float *workspace,
                               long long workspace_floats, vfi_stream_t stream);

/* Number of partial slabs vfi_conv2d_backward_weight sums for this layer and workspace (-1 on bad arguments).  Two calls
 * over the same (N, H, W) with the same count accumulate every element in the same order, whatever their Cout: a bank of
 * filters (the AdaCoF heads' shared 64 -> 448 first convolution) then gives the bits of its members' own calls. */
int vfi_conv2d_backward_weight_splits(int N, int Cin, int H, int W, int Cout, int KS, long long workspace_floats);

/* Minimum workspace (floats) of vfi_conv2d_backward_data (-1 on bad arguments): N*(Cin+Cout)*(H+2p)*(W+2p) for
 * reflect padding p = (KS-1)/2 > 0, else 0. */
long long vfi_conv2d_backward_data_workspace_floats(int N, int Cin, int H, int W, int Cout, int KS, int pad_mode);

/* Input gradient of the same layer: dx (N, Cin, H, W) from dy (N, Cout, H, W).  packed_wt is vfi_conv2d_pack of the
 * transposed, flipped weights W.transpose(0,1).flip(2,3) (Cout' = Cin, Cin' = Cout).  Zero padding (and KS = 1): one
 * vfi_conv2d of dy with the same padding.  Reflect: dy zero-embedded into (H+2p) x (W+2p), vfi_conv2d with zero padding
 * gives the gradient of the padded input, and each pad row / column is folded onto the interior pixel it mirrors
 * (torch's reflection-pad backward).  Workspace beyond the minimum goes to vfi_conv2d's split-K. */
int vfi_conv2d_backward_data(const float *dy, long long dy_bstride, const float *packed_wt, float *dx, long long dx_bstride,
                             int N, int Cin, int H, int W, int Cout, int KS, int pad_mode, float *workspace,
                             long long workspace_floats, vfi_stream_t stream);

/* Backward of vfi_tanh_residual_clamp (fusion_net.py:70-77): m = [0 <= base + tanh x <= 1] (inclusive, as
 * torch.clamp), grad_x = grad_y (1 - tanh^2 x) m, grad_base = grad_y m; either output may be NULL. */
int vfi_tanh_residual_clamp_backward(const float *x, const float *base, const float *grad_y, float *grad_x,
                                     float *grad_base, long long count, vfi_stream_t stream);

/* Backward of FusionNet's encoder block glue (fusion_net.py:55-59): y = relu(conv) (N, C, H, W) feeds MaxPool2d(2) and
 * the skip.  grad_y = ([first maximal element of each 2x2 window in row-major order] * grad_pooled + grad_skip) * [y > 0]
 * (torch's max_pool2d routing).  grad_skip may be NULL.  H, W even. */
int vfi_pool2_max_backward(const float *y, long long y_bstride, const float *grad_pooled, long long gp_bstride,
                           const float *grad_skip, long long gs_bstride, float *grad_y, long long gy_bstride, int N, int C,
                           int H, int W, vfi_stream_t stream);

/* Adjoint of vfi_resize_bilinear with align_corners = 0 and Hout = 2 Hin, Wout = 2 Win (nn.Upsample(scale_factor=2) of
 * fusion_net.py:42,65): grad_x (N, C, Hin, Win) gathered from grad_y (no atomics); relu_input multiplies by [x > 0]
 * (x: the forward's source, may be NULL without relu_input).  The residual's gradient is grad_y itself. */
int vfi_resize_bilinear_backward(const float *x, long long x_bstride, const float *grad_y, long long gy_bstride,
                                 float *grad_x, long long gx_bstride, int N, int C, int Hin, int Win, int Hout, int Wout,
                                 int relu_input, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Backward of the plain AdaCoF network (training, src/adacof/trainer.py:36-54): the glue between the convolution
 * gradients above and vfi_adacof_backward.  Differentiates src/adacof/models/adacofnet.py:13-153 (KernelEstimation) and
 * :191-217 (blend, smoothness terms) and src/adacof/utility.py:67-77 (Charbonnier).  Same rules: no float atomics, one
 * writer per element, reductions in an order fixed by the shape.  Operands with a batch stride may be channel slices.
 * ---------------------------------------------------------------------------------- */

/* Floats of the `workspace` of the two reductions below. */
#define VFI_REDUCE_WORKSPACE_FLOATS 4096

/* out = a + b over N blocks of `count` floats: the additive skip of adacofnet.py:128-146, which the training forward keeps
 * apart from relu(conv) so that the ReLU's mask stays exact. */
int vfi_add(const float *a, long long a_bstride, const float *b, long long b_bstride, float *out, long long out_bstride,
            int N, long long count, vfi_stream_t stream);

/* out = (grad + addend) * [y > 0] (ReLU backward between the convolutions of a block, adacofnet.py:14-23; y is the ReLU's
 * output, y == 0 passes nothing).  addend may be NULL; out may be grad itself (in place). */
int vfi_relu_mask(const float *grad, long long g_bstride, const float *addend, long long a_bstride, const float *y,
                  long long y_bstride, float *out, long long out_bstride, int N, long long count, vfi_stream_t stream);

/* grad_z = grad * s * (1 - s): backward of s = sigmoid(z) over `count` floats (the occlusion head, adacofnet.py:98-99, when
 * KernelEstimation is trained on its own; AdaCoFNet's backward folds it into vfi_adacof_blend_backward). */
int vfi_sigmoid_backward(const float *grad, const float *s, float *grad_z, long long count, vfi_stream_t stream);

/* out (N, C, H + 2 pad, W + 2 pad) dense = ReplicationPad2d(pad) of x (N, C, H, W) (adacofnet.py:166,193-194): the planar
 * padded frames vfi_adacof_backward reads. */
int vfi_replicate_pad(const float *x, long long x_bstride, float *out, int N, int C, int H, int W, int pad,
                      vfi_stream_t stream);

/* Backward of an encoder block's glue (adacofnet.py:112-125): y = relu(conv) (N, C, H, W) feeds AvgPool2d(2) and the skip.
 * grad_y = (0.25 * grad_pooled over its 2x2 window + grad_skip) * [y > 0].  grad_skip may be NULL.  H, W even; operands
 * 8-byte aligned with even batch strides. */
int vfi_pool2_avg_backward(const float *y, long long y_bstride, const float *grad_pooled, long long gp_bstride,
                           const float *grad_skip, long long gs_bstride, float *grad_y, long long gy_bstride, int N, int C,
                           int H, int W, vfi_stream_t stream);

/* Adjoint of Upsample(scale_factor=2, bilinear, align_corners=True) (adacofnet.py:30,42,54,68,76,88), gather form:
 * grad_x (N, C, Hin, Win) from grad_y (N, C, 2 Hin, 2 Win) with the weights of align_corners=1 from exact integer cell / remainder arithmetic
 * (Hin = 1 or Win = 1: every output reads source 0).  mask_src (may be NULL) is the upsample's source when it is a ReLU's
 * output: grad_x is multiplied by [mask_src > 0]. */
int vfi_upsample2x_backward(const float *grad_y, long long gy_bstride, const float *mask_src, long long ms_bstride,
                            float *grad_x, long long gx_bstride, int N, int C, int Hin, int Win, vfi_stream_t stream);

/* Smoothness terms of adacofnet.py:204-215.  w*, a*, b* (N, F*F, H, W) dense (w* after the softmax), occ (N, 1, H, W).
 *   m (N, 4, H, W) <- (mean_k W1 A1, mean_k W1 B1, mean_k W2 A2, mean_k W2 B2)   [m_Alpha1, m_Beta1, m_Alpha2, m_Beta2]
 *   out[0] = g_Spatial, out[1] = g_Occlusion with CharbonnierFunc(d) = mean sqrt(d^2 + epsilon^2) of the horizontal plus
 *   that of the vertical differences.  Two-stage reduction over `workspace` (VFI_REDUCE_WORKSPACE_FLOATS). */
int vfi_adacof_smooth_forward(const float *w1, const float *a1, const float *b1, const float *w2, const float *a2,
                              const float *b2, const float *occ, float *m, float *workspace, float *out, int N, int F,
                              int H, int W, float epsilon, vfi_stream_t stream);

/* Backward of frame1 = occ t1 + (1 - occ) t2 cropped to (h0, w0) (adacofnet.py:196-200) and of g_Occlusion (:213), through
 * the sigmoid that made occ.  grad_frame (N, C, h0, w0) dense; t1, t2 (N, C, H, W); occ (N, 1, H, W); up_occ: device
 * scalar, the upstream gradient of g_Occlusion (NULL: none).
 *   grad_t1 = g occ, grad_t2 = g (1 - occ), grad_z = (sum_c g_c (t1_c - t2_c) + up_occ * dCharbonnier/d occ) occ (1 - occ)
 * with g = grad_frame inside the crop and 0 outside. */
int vfi_adacof_blend_backward(const float *grad_frame, const float *t1, const float *t2, const float *occ,
                              const float *up_occ, float *grad_t1, float *grad_t2, float *grad_z, int N, int C, int H,
                              int W, int h0, int w0, float epsilon, vfi_stream_t stream);

/* One side's head gradients from vfi_adacof_backward's (gw, ga, gb) and g_Spatial (adacofnet.py:204-212,215).  m_a, m_b:
 * that side's two planes of vfi_adacof_smooth_forward's m (batch stride m_bstride); up_spatial: device scalar (NULL: none).
 * With q_X = up_spatial * dCharbonnier/d m_X:  gW_k = gw_k + (q_A a_k + q_B b_k) / F^2,
 *   grad_logit_k = w_k (gW_k - sum_j w_j gW_j)  (softmax backward),  grad_alpha_k = ga_k + q_A w_k / F^2,  grad_beta alike. */
int vfi_adacof_head_backward(const float *gw, const float *ga, const float *gb, const float *w, const float *a,
                             const float *b, const float *m_a, const float *m_b, long long m_bstride,
                             const float *up_spatial, float *grad_logit, float *grad_alpha, float *grad_beta, int N, int F,
                             int H, int W, float epsilon, vfi_stream_t stream);

/* out[0] = mean sqrt((a - b)^2 + epsilon^2) over `count` floats (utility.py:67-77; b may be NULL = 0).  Two-stage
 * reduction over `workspace` (VFI_REDUCE_WORKSPACE_FLOATS). */
int vfi_charbonnier_forward(const float *a, const float *b, long long count, float epsilon, float *workspace, float *out,
                            vfi_stream_t stream);

/* grad_a = upstream[0] * d / sqrt(d^2 + epsilon^2) / count with d = a - b, grad_b = -grad_a; either may be NULL. */
int vfi_charbonnier_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b,
                             long long count, float epsilon, vfi_stream_t stream);

/* out[0] = mean (a - b)^2 over `count` floats (nn.MSELoss: src/adacof/losses/__init__.py:17, losses/vgg.py:20).  a and b may
 * be two parts of one allocation.  Two-stage reduction over `workspace` (VFI_REDUCE_WORKSPACE_FLOATS). */
int vfi_mse_forward(const float *a, const float *b, long long count, float *workspace, float *out, vfi_stream_t stream);

/* grad_a = upstream[0] * 2 (a - b) / count, grad_b = -grad_a; either may be NULL. */
int vfi_mse_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b, long long count,
                     vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Backward of one PhaseNet level (training, src/phase_net/train.py with src/train/loss.py): the glue between the
 * convolution gradients above.  Differentiates src/phase_net/phase_net.py:113-116,138-139,155-168,190-200 with
 * reverse_normalize :80-98, and src/train/loss.py:10-20.  Same rules: no float atomics, one writer per element,
 * reductions in an order fixed by the shape, fp32.  Operands with a batch stride may be channel slices.
 * ---------------------------------------------------------------------------------- */

/* Adjoint of vfi_resize_bilinear with align_corners = 0, relu_input = 0 and no residual, for any sizes >= 1 (up- and
 * down-sampling): nn.Upsample((res1, res2), mode='bilinear') of phase_net.py:138-139.  Gather form: grad_x (N, C, Hin, Win)
 * element s sums grad_y (N, C, Hout, Wout) over the outputs whose forward taps hit s, found by re-evaluating the forward's
 * own fp32 index and weight arithmetic over a candidate range, rows outermost, both ascending.  A source that no output
 * reads gets 0.  Sizes below 2^20. */
int vfi_resize_bilinear_adjoint(const float *grad_y, long long gy_bstride, float *grad_x, long long gx_bstride, int N, int C,
                                int Hin, int Win, int Hout, int Wout, vfi_stream_t stream);

/* out = grad * f'(y) over N blocks of `count` floats, from the activation's OUTPUT y (phase_net.py:193,195,199):
 * act = VFI_ACT_ELU (alpha = 1): f' = y > 0 ? 1 : y + 1;  VFI_ACT_TANH: f' = 1 - y^2.  out may be grad itself (in place). */
int vfi_act_backward(const float *grad, long long g_bstride, const float *y, long long y_bstride, float *out,
                     long long out_bstride, int N, long long count, int act, vfi_stream_t stream);

/* Adjoint of vfi_phasenet_emit with respect to pred (phase_net.py:155-168, :80-90).  grad_phase, grad_amp (N, 4, HW) dense,
 * either may be NULL (= zero); amp_in, max_amp as in the forward (they get no gradient):
 *   grad_pred[:, 0:4] = pi * grad_phase;  grad_pred[:, 4:8] = grad_amp * max_amp[n] * (amp_in[:, 4:8] - amp_in[:, 0:4]) / 2. */
int vfi_phasenet_emit_backward(const float *grad_phase, const float *grad_amp, const float *amp_in, long long amp_bstride,
                               const float *max_amp, float *grad_pred, long long gp_bstride, int N, int HW,
                               vfi_stream_t stream);

/* Adjoint of vfi_phasenet_emit_low with respect to pred (phase_net.py:113-116, :96-98): grad_low (N, HW) dense,
 *   grad_pred (N, HW) = grad_low * max_low[n] * (low_in[:, 0] - low_in[:, 1]) / 2. */
int vfi_phasenet_emit_low_backward(const float *grad_low, const float *low_in, long long low_bstride, const float *max_low,
                                   float *grad_pred, long long gp_bstride, int N, int HW, vfi_stream_t stream);

/* Adjoint of vfi_phasenet_predict (one band level's head: 1x1 64 -> 8, tanh, vfi_phasenet_emit) in one pass over the pixels.
 * feat (N, 64, HW) and pred (N, 8, HW; the forward's post-tanh output) with batch strides, amp_in / max_amp as in the forward,
 * weight (8, 64) the prediction map's nn.Conv2d weight as it is (not packed).  Upstream: grad_phase, grad_amp (N * 4, HW)
 * dense, grad_pred_in (N, 8, HW) with a batch stride -- what the next finer level's resize adjoint sends back to pred; any of
 * the three may be NULL (= zero).  Per pixel
 *   g[0:4] = pi * grad_phase + grad_pred_in[0:4]
 *   g[4:8] = grad_amp * max_amp[n] * (amp_in[4:8] - amp_in[0:4]) / 2 + grad_pred_in[4:8]
 *   gz     = g * (1 - pred^2)
 * and grad_feat[k] = sum_j weight[j][k] gz[j] (N, 64, HW; written, not accumulated), grad_weight[j][k] = sum gz[j] feat[k]
 * (8, 64), grad_bias[j] = sum gz[j] (8), the sums over all pixels and samples.  An output that is NULL is skipped (at least
 * one is given; feat is read only for the parameter gradients, weight only for grad_feat).  The parameter gradients are a
 * two-stage reduction over `workspace` (VFI_PHASENET_HEAD_WORKSPACE_FLOATS; at most 1024 block partials, then one block) in an
 * order fixed by (N, HW).  16-byte accesses when HW, every stride and every base allow, 4-byte otherwise.  64 * HW < 2^31. */
#define VFI_PHASENET_HEAD_WORKSPACE_FLOATS (1024 * 520)
int vfi_phasenet_predict_backward(const float *feat, long long feat_bstride, const float *pred, long long pred_bstride,
                                  const float *amp_in, long long amp_bstride, const float *max_amp, const float *weight,
                                  const float *grad_phase, const float *grad_amp, const float *grad_pred_in,
                                  long long gpi_bstride, float *grad_feat, long long gf_bstride, float *grad_weight,
                                  float *grad_bias, float *workspace, int N, int HW, vfi_stream_t stream);

/* The three adjoints above for PhaseNet with num_img = 2, 3 or 4 input images: the adjoints of vfi_phasenet_emit_n,
 * vfi_phasenet_emit_low_n and vfi_phasenet_predict_n.  Same rules.  For num_img = 2 and 4 each runs the kernel of its two-image
 * counterpart (the blend reads the first two images only: planes 8..15 of amp_in and 2..3 of low_in are never read, and pred
 * is not read by the two emit adjoints); any other num_img is VFI_ERR_UNSUPPORTED.  For num_img = 3 pred is an input of all
 * three, because the second blend's adjoint needs it.
 *
 * vfi_phasenet_emit_n_backward, num_img = 3: pred (N,12,HW), amp_in (N,12,HW), grad_pred (N,12,HW).  With b = (pred[4:8]+1)/2,
 * fb = (pred[8:12]+1)/2 and amp1 = b*amp_in[4:8] + (1-b)*amp_in[0:4]:
 *   grad_pred[0:4]  = pi * grad_phase
 *   grad_pred[4:8]  = grad_amp * max_amp[n] * fb * (amp_in[4:8] - amp_in[0:4]) / 2
 *   grad_pred[8:12] = grad_amp * max_amp[n] * (amp1 - amp_in[8:12]) / 2
 * Either upstream gradient may be NULL (= zero); pred, amp_in and max_amp are read only with grad_amp. */
int vfi_phasenet_emit_n_backward(const float *grad_phase, const float *grad_amp, const float *pred, long long pred_bstride,
                                 const float *amp_in, long long amp_bstride, const float *max_amp, float *grad_pred,
                                 long long gp_bstride, int N, int HW, int num_img, vfi_stream_t stream);

/* vfi_phasenet_emit_low_n_backward, num_img = 3: pred (N,2,HW), low_in (N,3,HW), grad_pred (N,2,HW).  With a = (pred[0]+1)/2,
 * fa = (pred[1]+1)/2 and low1 = a*low_in[0] + (1-a)*low_in[1]:
 *   grad_pred[0] = grad_low * max_low[n] * fa * (low_in[0] - low_in[1]) / 2
 *   grad_pred[1] = grad_low * max_low[n] * (low1 - low_in[2]) / 2 */
int vfi_phasenet_emit_low_n_backward(const float *grad_low, const float *pred, long long pred_bstride, const float *low_in,
                                     long long low_bstride, const float *max_low, float *grad_pred, long long gp_bstride, int N,
                                     int HW, int num_img, vfi_stream_t stream);

/* vfi_phasenet_predict_n_backward: vfi_phasenet_predict_backward's contract.  num_img = 2 and 4 ARE that entry point (same
 * launches, VFI_PHASENET_HEAD_WORKSPACE_FLOATS suffice).  num_img = 3: pred, grad_pred_in (N,12,HW), weight (12,64),
 * grad_weight (12,64), grad_bias (12); g = the emit adjoint above + grad_pred_in, gz = g * (1 - pred^2), grad_feat[k] =
 * sum_j weight[j][k] gz[j] (written, not accumulated).  Block partials are 12 * 64 + 12 floats:
 * `workspace` holds VFI_PHASENET_HEAD_N_WORKSPACE_FLOATS. */
#define VFI_PHASENET_HEAD_N_WORKSPACE_FLOATS (1024 * 780)
int vfi_phasenet_predict_n_backward(const float *feat, long long feat_bstride, const float *pred, long long pred_bstride,
                                    const float *amp_in, long long amp_bstride, const float *max_amp, const float *weight,
                                    const float *grad_phase, const float *grad_amp, const float *grad_pred_in,
                                    long long gpi_bstride, float *grad_feat, long long gf_bstride, float *grad_weight,
                                    float *grad_bias, float *workspace, int N, int HW, int num_img, vfi_stream_t stream);

/* Batch-statistics BatchNorm of a block (reference src/phase_net/block.py:17, nn.BatchNorm2d in training mode, with the ELU
 * of block.py:18): per-channel mean[c] and BIASED variance var[c] of y (N, C, HW; batch stride y_bstride) over the samples
 * and pixels.  Two stages: every channel's N * HW values are cut into equal chunks by (N, C, HW) alone, one block writes
 * (count, mean, M2) of each chunk, one final block per channel merges them in chunk order with Chan's formula -- never
 * E[y^2] - E[y]^2.  `workspace`: VFI_REDUCE_WORKSPACE_FLOATS (C * chunks * 3 partials fit by the choice of the cut;
 * C <= 1365).  N * HW < 2 is VFI_ERR_SHAPE (torch: "Expected more than 1 value per channel when training").  16-byte
 * accesses when HW, the stride and the base allow, 4-byte otherwise. */
int vfi_bn_stats(const float *y, long long y_bstride, int N, int C, int HW, float *mean, float *var, float *workspace,
                 vfi_stream_t stream);

/* out = act(gamma (y - mean) / sqrt(var + eps) + beta) per channel (block.py:17-18 in training mode, F.batch_norm's
 * normalisation): act = VFI_ACT_NONE or VFI_ACT_ELU; mean, var as vfi_bn_stats wrote them (or any statistics); one read and
 * one write, the scale formed once per block.  out may be y itself. */
int vfi_bn_act_forward(const float *y, long long y_bstride, const float *mean, const float *var, const float *gamma,
                       const float *beta, float eps, int act, float *out, long long out_bstride, int N, int C, int HW,
                       vfi_stream_t stream);

/* Adjoint of vfi_bn_stats + vfi_bn_act_forward (block.py:17-18, nn.BatchNorm2d in training mode: the statistics depend on
 * y).  g_t: gradient of the output t; t: that output (read for VFI_ACT_ELU only, may be NULL otherwise); y: the kept input.
 * With g_z = g_t act'(t) (ELU' from the output: t > 0 ? 1 : t + 1), xhat = (y - mean) / sqrt(var + eps), n = N * HW:
 *   g_beta[c] = sum g_z,  g_gamma[c] = sum g_z xhat           (two stages over `workspace`, VFI_REDUCE_WORKSPACE_FLOATS,
 *                                                              the cut and the order of vfi_bn_stats)
 *   g_y = gamma / sqrt(var + eps) * (g_z - g_beta / n - xhat g_gamma / n)
 * g_y may be g_t itself; g_y NULL skips that pass (gamma may then be NULL). */
int vfi_bn_act_backward(const float *g_t, long long gt_bstride, const float *t, long long t_bstride, const float *y,
                        long long y_bstride, const float *mean, const float *var, const float *gamma, float eps, int act,
                        float *g_y, long long gy_bstride, float *g_gamma, float *g_beta, float *workspace, int N, int C,
                        int HW, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The AdaCoF trainer's discriminator (reference src/adacof/losses/discriminator.py)
 * ---------------------------------------------------------------------------------- */

/* BatchNorm2d (batch statistics) + LeakyReLU(slope) of a discriminator block: vfi_bn_act_forward / vfi_bn_act_backward with
 * act(z) = z > 0 ? z : slope z, the same kernels and the same fixed-order reductions (statistics: vfi_bn_stats).  The
 * derivative is read off the sign of the output t, so slope must be positive (VFI_ERR_INVALID_ARG otherwise) and t is
 * required.  Everything else as the vfi_bn_act_* pair. */
int vfi_bn_leaky_forward(const float *y, long long y_bstride, const float *mean, const float *var, const float *gamma,
                         const float *beta, float eps, float slope, float *out, long long out_bstride, int N, int C, int HW,
                         vfi_stream_t stream);
int vfi_bn_leaky_backward(const float *g_t, long long gt_bstride, const float *t, long long t_bstride, const float *y,
                          long long y_bstride, const float *mean, const float *var, const float *gamma, float eps, float slope,
                          float *g_y, long long gy_bstride, float *g_gamma, float *g_beta, float *workspace, int N, int C,
                          int HW, vfi_stream_t stream);

/* Phase split: xs (N, 4C, ceil(H/2), ceil(W/2)) from x (N, C, H, W),
 *   xs[n, (2 py + px) C + c, i, j] = x[n, c, 2 i + py, 2 j + px], zero beyond the edge.
 * A 3x3 / stride 2 / pad 1 convolution of x is the 3x3 / stride 1 / zero pad 1 vfi_conv2d of xs with the weights expanded to
 * (Cout, 4C, 3, 3): tap k of an axis goes to (phase, tap) 0 -> (1, 0), 1 -> (0, 1), 2 -> (1, 1); its data gradient is
 * vfi_conv2d_backward_data followed by vfi_phase_merge, its weight gradient vfi_conv2d_backward_weight on xs.
 * One read and one write; batch strides in floats; 16-byte accesses when W is a multiple of 8, the strides are multiples
 * of 4 and the bases are 16-byte aligned, 4-byte ones otherwise. */
int vfi_phase_split(const float *x, long long x_bstride, float *xs, long long xs_bstride, int N, int C, int H, int W,
                    vfi_stream_t stream);
/* The adjoint (and inverse on the image of vfi_phase_split): gx (N, C, H, W) from gs (N, 4C, ceil(H/2), ceil(W/2)); the
 * positions of the zero fill are dropped. */
int vfi_phase_merge(const float *gs, long long gs_bstride, float *gx, long long gx_bstride, int N, int C, int H, int W,
                    vfi_stream_t stream);

/* y (B, J) = leaky(x (B, K) w^T + bias), w (J, K) as nn.Linear holds it, leaky(z) = z > 0 ? z : slope z; slope = 1: no
 * activation; slope <= 0: VFI_ERR_INVALID_ARG.  bias may be NULL.  Dense row-major operands.  w is streamed once per slice of
 * four samples (16-byte loads when K is a multiple of 4 and x, w are 16-byte aligned), x comes from the caches; any B >= 1.
 * Sums in an order fixed by K alone. */
int vfi_linear_forward(const float *x, const float *w, const float *bias, float *y, int B, int K, int J, float slope,
                       vfi_stream_t stream);
/* Adjoint, g (B, J) the gradient of y: gm = g * (y > 0 ? 1 : slope) (y may be NULL when slope = 1),
 *   dx (B, K) = gm w,  dw (J, K) = gm^T x,  dbias (J) = sum_b gm;  each may be NULL (not produced), not all three.
 * x may be NULL without dw, w without dx.  One pass: every workgroup owns a slab of columns k and walks j in order, so w is
 * read once and dw written once when both are wanted (B <= 4; further slices of four samples add to dw in order).  One writer
 * per element, no atomics. */
int vfi_linear_backward(const float *x, const float *w, const float *y, float slope, const float *g, float *dx, float *dw,
                        float *dbias, int B, int K, int J, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * The WGAN_GP term: LeakyReLU as a mask, the interpolate, the gradient penalty (reference
 * src/adacof/losses/adversarial.py:54-68)
 * ---------------------------------------------------------------------------------- */

/* out[n][e] = s[n][e] > 0 ? a[n][e] : slope * a[n][e] over N batch-strided runs of `count` floats (strides in floats).
 * s may be a itself (LeakyReLU of a convolution's output), out may be a itself (the mask of a gradient or of a tangent, in
 * place, s the activation's output: its sign is the pre-activation's for slope > 0), and all three may be one tensor.
 * slope <= 0: VFI_ERR_INVALID_ARG, as vfi_bn_leaky_*.  16-byte accesses when count, the strides and the bases allow,
 * 4-byte ones otherwise: the same bits either way. */
int vfi_leaky_mask(const float *a, long long a_bstride, const float *s, long long s_bstride, float *out, long long out_bstride,
                   int N, long long count, float slope, vfi_stream_t stream);

/* hat = fake * (1 - eps) + real * eps per float, eps of fake's shape: the four operations rounded one by one (no fused
 * multiply-add), so the bits are those of the float32 expression `fake.mul(1 - eps) + real.mul(eps)`.  Layout and access
 * widths as vfi_leaky_mask; hat aliases no operand. */
int vfi_gp_mix(const float *fake, long long f_bstride, const float *real, long long r_bstride, const float *eps,
               long long e_bstride, float *hat, long long h_bstride, int N, long long count, vfi_stream_t stream);

/* norms[b] = ||g[b]||_2 over the n floats of sample b (batch stride g_bstride floats), value[0] = weight / B *
 * sum_b (norms[b] - 1)^2.  One workgroup per sample: every thread's chain in index order, the lanes of a 16-byte load as
 * (x + y) + (z + w), then the block tree; a last workgroup of one launch more sums the B terms the same way.  The order is
 * fixed by n, B and the access width alone. */
int vfi_grad_penalty_forward(const float *g, long long g_bstride, float *norms, float *value, int B, long long n, float weight,
                             vfi_stream_t stream);

/* out[b] = upstream[0] * weight * 2 (norms[b] - 1) / (B norms[b]) * g[b]: the gradient of upstream[0] * value to g.  A row
 * whose norm is 0 gives zeros (torch's norm backward).  The factor of a row is formed once, in double. */
int vfi_grad_penalty_backward(const float *g, long long g_bstride, const float *norms, const float *upstream, float *out,
                              long long out_bstride, int B, long long n, float weight, vfi_stream_t stream);

/* out[0] = scale / count * sum |w(a - b)| over `count` floats, w(d) = atan2(sin d, cos d) when wrap != 0, else d.
 * wrap = 0, scale = 1: nn.L1Loss (loss.py:8,20).  wrap = 1, scale = nbands, a = the target's and b = the output's phases
 * of one level: that level's term of the phase loss, the sum over the orientations of the mean |delta_psi| (loss.py:10-16).
 * Two-stage reduction over `workspace` (VFI_REDUCE_WORKSPACE_FLOATS), tree fixed by `count`. */
int vfi_l1_forward(const float *a, const float *b, long long count, int wrap, float scale, float *workspace, float *out,
                   vfi_stream_t stream);

/* grad_a = sign(w(a - b)) * upstream[0] * scale / count, grad_b = -grad_a; either may be NULL. */
int vfi_l1_backward(const float *a, const float *b, const float *upstream, float *grad_a, float *grad_b, long long count,
                    int wrap, float scale, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Complex steerable pyramid (frequency domain), scale_factor-generalised
 * ---------------------------------------------------------------------------------- */

/* Opaque plan: level geometry, mask tables, the tables of the hand-written FFT kernels (twiddles, Bluestein chirps and
 * filters; no FFT library is linked) and workspace for one (H, W, height, nbands, scale_factor).  Replaces the
 * per-frame construction of `SCFpyr_PyTorch(height, nbands, scale_factor, device)` (reference
 * src/train/pyramid.py:28-33, rebuilt for every frame at src/fusion_net/interpolate_twoframe.py:124-129).  Creation
 * allocates device memory and synchronises; everything else only enqueues.  A plan's workspace belongs to one stream
 * at a time: frames in flight use one plan each.
 * max_images (1..16) sizes the workspace: it is the number of images ONE SLICE of a call holds, not a limit on N.
 * vfi_pyr_analyze, vfi_pyr_synthesize, their two backward calls and vfi_pyr_apply_filter take any N >= 1 and process
 * consecutive slices of max_images images (the last one shorter; vfi_pyr_apply_filter_pair: max_images / 2 images of each
 * set), each through the same passes on the one workspace, in stream order: nothing is allocated, synchronised or copied,
 * and a call of N <= max_images is one slice.  Every slice addresses the caller's tensors of the whole call: with
 * VFI_PYR_BAND_MAJOR the bands lie N planes apart, and a plane_index table has N entries per level.
 * vfi_pyr_analyze_max reduces its maxima inside one launch and keeps N <= max_images; vfi_pyr_plan_multi_levels answers
 * for one slice (N <= max_images). */
typedef struct vfi_pyr_plan vfi_pyr_plan;

enum {
    VFI_PYR_BAND_MAJOR = 1,    /* default plane of image d, band b is d*nbands+b; with this flag b*N+d */
    VFI_PYR_COMPLEX_COEFF = 2  /* bands are interleaved (re, im) coefficients instead of (phase, amplitude) */
};

/* Every level size must be transformable: any length with prime factors 2, 3, 5 up to 8704, any other length up to 4096
 * (frames up to 3840x2160 qualify; VFI_ERR_UNSUPPORTED otherwise).  Lengths the wave-private register engine has a
 * configuration for (the level sizes of 256x256 ... 1920x1080 frames among them) run on it, the others on the generic
 * LDS engine; results agree to fp32 rounding. */
int vfi_pyr_plan_create(int H, int W, int height, int nbands, double scale_factor, int max_images,
                        vfi_pyr_plan **out);
int vfi_pyr_plan_destroy(vfi_pyr_plan *plan);
/* Size of band level `level` (0 = finest .. height-3) or of the low residual (level == height-2):
 * ceil(H / scale_factor^level) x ceil(W / scale_factor^level). */
int vfi_pyr_plan_level_size(const vfi_pyr_plan *plan, int level, int *h, int *w);

/* Read-only queries of what a plan will do (no GPU call; for tests and profiling labels: the selection rules live in the
 * library only, as with vfi_conv2d_algo).
 * vfi_pyr_plan_query_pass: how one pass of one 2-D size runs, as the plan resolved it at creation.
 *   size_index  band level 0 .. height-3, height-2 = the low residual, height-1 = the frame
 *   pass        VFI_PYR_PASS_ROWS, VFI_PYR_PASS_ANA_COLS (also the plain column pass of the low residual's and the frame's
 *               transforms), VFI_PYR_PASS_SYN_COLS (band levels only)
 *   info        8 ints: [0] transform length n, [1] 1 when n goes through Bluestein, [2] the length m that is transformed
 *               (n, or Bluestein's 2^k / 3*2^k), [3] wave-engine length M of the pass, 0 = the generic LDS engine runs it,
 *               and for band levels (0 otherwise) [4] columns per workgroup and [5] bands per transform call of the generic
 *               column kernels, [6] / [7] row pitch of the half-transformed array in the analysis / synthesis direction.
 * vfi_pyr_plan_multi_levels: the levels of level_mask that an analysis (vfi_pyr_analyze, vfi_pyr_analyze_max,
 * vfi_pyr_synthesize_backward) of N images runs in the batched launches of the small levels on the generic engine instead
 * of their own passes; 0 when every level runs its own. */
enum { VFI_PYR_PASS_ROWS = 0, VFI_PYR_PASS_ANA_COLS = 1, VFI_PYR_PASS_SYN_COLS = 2 };
int vfi_pyr_plan_query_pass(const vfi_pyr_plan *plan, int size_index, int pass, int *info);
int vfi_pyr_plan_multi_levels(const vfi_pyr_plan *plan, int N, unsigned long long level_mask, unsigned long long *multi_mask);

/* Analysis followed by synthesis of an UNMODIFIED subset of the pyramid is a real, radially symmetric linear
 * filter (the four orientation masks form a partition of unity):
 *   inv_filter(keep(filter(x))) = real(ifft2(fft2(x) * G)),
 *   G = [keep_high] hi0^2 + lo0^2 * ( sum_{k in level_mask} (prod_{j<k} lomask_j^2) himask_k^2 + [keep_low] prod_j lomask_j^2 ).
 * vfi_pyr_plan_prepare_filter builds G once (allocates; returns an id), vfi_pyr_apply_filter applies it to
 * N images (N,H,W) with one R2C, one multiply and one C2R.  Replaces
 * `pyr.inv_filter(get_last_value_levels(vals, 1))` of src/fusion_net/interpolate_twoframe.py:205-209
 * (24 band FFTs forward and back per call) wherever the kept values are not modified in between. */
int vfi_pyr_plan_prepare_filter(vfi_pyr_plan *plan, unsigned long long level_mask, int keep_high, int keep_low,
                                int *filter_id);
int vfi_pyr_apply_filter(vfi_pyr_plan *plan, int filter_id, const float *img, int N, float *out, vfi_stream_t stream);
/* out = real(ifft2(fft2(img_a) * G_a + fft2(img_b) * G_b)): the sum of two such filters applied to two image sets of N
 * images each (any N; the plan needs max_images >= 2), one C2R per slice.  Replaces the "baseline" mix of
 * src/fusion_net/interpolate_twoframe.py:288-322 -- filter(lab_ada), filter(lab_phase), a DecompValues assembled from the
 * fine levels + low residual of one and the coarse levels + high residual of the other, inv_filter -- which only moves
 * UNMODIFIED values: two full analyses and one full synthesis become two R2C, one multiply-add and one C2R. */
int vfi_pyr_apply_filter_pair(vfi_pyr_plan *plan, int filter_a, const float *img_a, int filter_b, const float *img_b, int N,
                              float *out, vfi_stream_t stream);

/* Pyramid.filter = SCFpyr_PyTorch.build + coeff_to_values (src/train/pyramid.py:35-39,48-78).
 *   img    (N, H, W)
 *   high   (N, H, W) or NULL;  low (N, hL, wL) or NULL
 *   phase[k], amp[k] (k < height-2; host arrays of device pointers): band level k, finest first.
 *          The plane (h_k*w_k floats) of image d, band b starts at plane index
 *          plane_index[k*N + d] + b*band_stride from phase[k] / amp[k]; plane_index == NULL gives the
 *          reference's per-image layout (N*nbands, 1, h, w) with index d*nbands+b.  A custom table lets
 *          the bands land directly in PhaseNet's (colour, frame*nbands+band) block-input buffers
 *          (separate_vals + get_concat_layers_inf, src/train/utils.py:47-127, without the copies).
 *   phase_scale multiplies the phase (1, or 1/pi for PhaseNet.normalize_vals, src/phase_net/phase_net.py:64)
 *   level_mask  bit k set = produce band level k (clear bits skip that level's inverse FFTs)
 *   flags       VFI_PYR_* */
int vfi_pyr_analyze(vfi_pyr_plan *plan, const float *img, int N, float *high, float *const *phase,
                    float *const *amp, const int *plane_index, float *low, float phase_scale,
                    unsigned long long level_mask, int flags, vfi_stream_t stream);
/* The same, plus the maxima PhaseNet.normalize_vals needs (src/phase_net/phase_net.py:55: max over the 8 channels
 * x pixels of each colour, per level), reduced inside the row kernel that writes the amplitudes (wave shuffles, one
 * atomic per wave): amp_max[k * groups + g] = max amplitude of level k over the images d with d % groups == g,
 * + eps.  amp_max must hold (height-2) * groups floats; levels outside level_mask get eps. */
int vfi_pyr_analyze_max(vfi_pyr_plan *plan, const float *img, int N, float *high, float *const *phase,
                        float *const *amp, const int *plane_index, float *low, float phase_scale,
                        unsigned long long level_mask, int flags, float *amp_max, int groups, float eps,
                        vfi_stream_t stream);

/* Pyramid.inv_filter = values_to_coeff + SCFpyr_PyTorch.reconstruct (src/train/pyramid.py:41-46,85-112).
 * high / low may be NULL (treated as zeros, e.g. PhaseNet's high_level, src/phase_net/phase_net.py:127-128);
 * band levels whose level_mask bit is clear are treated as zeros (get_last_value_levels /
 * get_first_value_levels, src/train/utils.py:242-320, without materialising the zero tensors). */
int vfi_pyr_synthesize(vfi_pyr_plan *plan, const float *high, const float *const *phase,
                       const float *const *amp, const int *plane_index, const float *low,
                       unsigned long long level_mask, int flags, float *img, int N, vfi_stream_t stream);

/* Gradient of vfi_pyr_synthesize with respect to its inputs, for training through Pyramid.inv_filter /
 * SCFpyr_PyTorch.reconstruct.  The synthesis is real-linear in the band coefficients, so its adjoint applied to the
 * gradient image is an analysis: grad z_{k,b} = 1/(H W) * unnormalised IFFT2_k(i * window_k(FFT2(g)) * A_k[b]) with
 * A_k[b] = lo0 * prod_{j<k} lomask_j * himask_k * (two-sided) angle mask b; grad high = the analysis' high output of g;
 * grad low = hL wL / (H W) * the analysis' low output of g.
 * vfi_pyr_plan_prepare_adjoint builds the A_k tables once per plan (allocates nbands floats per band coefficient of
 * every level; a second call is a no-op).  vfi_pyr_synthesize_backward returns VFI_ERR_INVALID_ARG without them.
 *   grad_img  (N, H, W): gradient of the loss with respect to vfi_pyr_synthesize's img
 *   phase, amp: the forward's inputs (same layout as vfi_pyr_synthesize; unused with VFI_PYR_COMPLEX_COEFF)
 *   grad_phase[k], grad_amp[k]: d phase = A (Im G cos p - Re G sin p), d amplitude = Re G cos p + Im G sin p for the
 *          coefficient gradient G; with VFI_PYR_COMPLEX_COEFF grad_phase[k] receives G as interleaved (re, im)
 *   levels whose level_mask bit is clear, and NULL grad_high / grad_low, are skipped. */
int vfi_pyr_plan_prepare_adjoint(vfi_pyr_plan *plan);
int vfi_pyr_synthesize_backward(vfi_pyr_plan *plan, const float *grad_img, int N, const float *const *phase,
                                const float *const *amp, const int *plane_index, unsigned long long level_mask, int flags,
                                float *grad_high, float *const *grad_phase, float *const *grad_amp, float *grad_low,
                                vfi_stream_t stream);

/* Gradient of vfi_pyr_analyze with respect to img, for training through Pyramid.filter / SCFpyr_PyTorch.build.  The
 * analysis is real-linear from the image to the band coefficients z_{k,b} = 1/(h_k w_k) * unnormalised IFFT2_k(i *
 * window_k(FFT2(img)) * P_a[k][b]), so its adjoint applied to coefficient gradients G is a synthesis:
 *   grad img = Re unnormalised IFFT2( lo0 * R_0 + hi0 * FFT2(grad_high) / (H W) ),
 *   R_k = embed_k(R_{k+1} * lomask_k) + sum_b (-i) * himask_k * (one-sided) angle mask b * FFT2_k(G_{k,b}) / (h_k w_k),
 *   R_L = FFT2_L(grad_low) / (hL wL)
 * -- the passes of vfi_pyr_synthesize with the tables B_k[b] = himask_k * angle mask b * H W / (h_k w_k) in place of P_s.
 * P_a cannot be read in place there (it carries lo0 * prod_{j<k} lomask_j, which the synthesis' passes apply on the way
 * up), so vfi_pyr_plan_prepare_analysis_adjoint builds the B_k once per plan (allocates nbands floats per band
 * coefficient of every level; a second call is a no-op).  vfi_pyr_analyze_backward returns VFI_ERR_INVALID_ARG without them.
 *   grad_high (N, H, W) or NULL (zeros);  grad_low (N, hL, wL) or NULL (zeros)
 *   grad_phase[k], grad_amp[k]: gradients of vfi_pyr_analyze's phase[k], amp[k] (same layout, plane_index and flags);
 *          phase[k], amp[k]: the forward's outputs, phase_scale the forward's.  The row pass forms
 *          G = (d A + i * phase_scale * d p / A) * exp(i * p / phase_scale); where A == 0 the d p term is dropped (the phase
 *          has no gradient at the origin; torch.atan2 yields NaN there).
 *          With VFI_PYR_COMPLEX_COEFF grad_phase[k] holds G as interleaved (re, im); phase, amp, grad_amp are unused.
 *   levels whose level_mask bit is clear contribute nothing (they only embed the coarser levels).
 * fp32, one writer per element, no atomics: results are bit-identical from run to run. */
int vfi_pyr_plan_prepare_analysis_adjoint(vfi_pyr_plan *plan);
int vfi_pyr_analyze_backward(vfi_pyr_plan *plan, const float *grad_high, const float *const *grad_phase,
                             const float *const *grad_amp, const float *const *phase, const float *const *amp,
                             const int *plane_index, const float *grad_low, float phase_scale,
                             unsigned long long level_mask, int flags, float *grad_img, int N, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Image-space stages the reference runs on the host CPU (skimage / scipy round trips)
 * ---------------------------------------------------------------------------------- */

/* rgb2lab_single / lab2rgb_single (src/train/transform.py:17-25,40-49): skimage D65/2deg conversion
 * with the reference's scaling L/100, (a+128)/255, (b+128)/255.  (N,3,HW) planar. */
int vfi_rgb2lab(const float *rgb, float *lab, int N, int HW, vfi_stream_t stream);
int vfi_lab2rgb(const float *lab, float *rgb, int N, int HW, vfi_stream_t stream);

/* out (N,HW) = mean_c a  (b == NULL)   or   |mean_c a - mean_c b|,  times scale; clamp01 is a flag word:
 * bit 0 clamps to [0,1], bit 1 keeps the SIGNED difference (no abs)
 * (src/fusion_net/interpolate_twoframe.py:207-211,219-220: `.mean(1)`, abs, `*100`/`*30`, clamp). */
int vfi_channel_mean_diff(const float *a, const float *b, float *out, int N, int C, int HW, float scale,
                          int clamp01, vfi_stream_t stream);

/* out = |x - y| * scale, or |x| * scale when y is NULL (clamped to [0,1] if clamp01): subtract_values (src/train/utils.py:322-346) and
 * `abs(freq_diff - median) * 5` clamp (interpolate_twoframe.py:223-224). */
int vfi_absdiff(const float *x, const float *y, float *out, long long count, float scale, int clamp01,
                vfi_stream_t stream);

/* scipy.ndimage.gaussian_filter(x, sigma, truncate=truncate) per (H,W) image, mode='reflect'
 * (interpolate_twoframe.py:212-213 uses sigma=5, default truncate=4 -> 41 taps).  tmp: N*H*W floats. */
int vfi_gaussian_filter(const float *x, float *tmp, float *y, int N, int H, int W, float sigma, float truncate,
                        vfi_stream_t stream);

/* scipy.ndimage.median_filter(x, size=size) per (H,W) image: size x size window covering
 * [i - size/2, i - size/2 + size - 1], mode='reflect', rank size*size/2 (interpolate_twoframe.py:221-222,
 * size=50).  Exact selection (returns an element of the window).  VFI_MEDIAN_PATH (read at every call) picks
 * the kernel: walk (default), rank or bisect; all three return the same bits. */
int vfi_median_filter(const float *x, float *y, int N, int H, int W, int size, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Quality scoring on device (src/evaluation/evaluate_image.py:7-30)
 * ---------------------------------------------------------------------------------- */

/* out2[0] = sum(a - b), out2[1] = sum((a - b)^2) over `count` floats, accumulated in double in a fixed order
 * (deterministic).  PSNR / SSD / L1 / MSE / variance of evaluate_image.py:22-28 follow from the two sums.
 * workspace: 2 * 1024 doubles. */
int vfi_diff_sums(const float *a, const float *b, long long count, double *out2, void *workspace, vfi_stream_t stream);

/* Sum of the SSIM map (piq.ssim formula) over the interior [border, H-border) x [border, W-border) of `planes`
 * planes, from the Gaussian-filtered moments mu_x, mu_y, E[xx], E[yy], E[xy]; out2[0] = sum.  workspace as above. */
int vfi_ssim_sum(const float *mu_x, const float *mu_y, const float *e_xx, const float *e_yy, const float *e_xy,
                 int planes, int H, int W, int border, float c1, float c2, double *out2, void *workspace,
                 vfi_stream_t stream);

/* out = a * b elementwise. */
int vfi_mul(const float *a, const float *b, float *out, long long count, vfi_stream_t stream);

/* F.avg_pool2d(kernel_size=f) on `planes` dense (H,W) planes -> (H/f, W/f) (floor): the down-sampling step of piq.ssim
 * (called at src/evaluation/evaluate_image.py:21) for images whose short side exceeds 384 px. */
int vfi_avg_pool(const float *x, float *y, int planes, int H, int W, int f, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training input side
 * ---------------------------------------------------------------------------------- */

/* One batch of Vimeo triplets from decoded uint8 frames to the tensors a training step takes: the host-side crop / hflip /
 * vflip / temporal swap of DBreader_Vimeo90k.__getitem__ (src/train/datareader.py:45-69), ToTensor's / 255, and
 * `preprocess` of the three frames (src/train/utils.py:174-206, called at src/train/trainer.py:115-117), in one pass.
 *   src     DEVICE uint8 (B, 3, Hs, Ws, 3): im1, im2, im3 of each sample, HWC as decoded; rows of 3 * Ws bytes, any alignment
 *   params  HOST int32 (B, 3) = (crop row i, crop column j, flags), read and checked before anything is enqueued and baked
 *           into the launch (a captured graph replays them); flags: bit 0 hflip, bit 1 vflip, bit 2 temporal swap
 *           (im3 takes im1's place and the other way round).  Order as the reference: crop, hflip, vflip.
 *   rgb     (3, B, 3, h, w) float32 or NULL: slot s = [first frame, last frame, middle frame] after the swap;
 *           rgb[s][b][c][y][x] = source byte / 255, bit-identical to `uint8.float() / 255`;
 *           element strides rgb_slot_stride (between slots) and rgb_batch_stride (between samples), the (3, h, w) block dense
 *   lab     (3, 3B, h, w) float32 or NULL: lab[s] = preprocess(rgb[s]), sample-major then L, a, b (vfi_rgb2lab's formulas
 *           and accuracy); lab_slot_stride between slots, lab_batch_stride between the (3, h, w) blocks of two samples.
 *           Dense, (9B, h, w) is the `torch.cat((lab_frame1, lab_frame2, target), 0)` of trainer.py:103.
 * VFI_ERR_INVALID_ARG, with nothing written: i < 0, i + h > Hs, j < 0, j + w > Ws, flags outside 0..7, both outputs NULL,
 * a stride below 3 * h * w.  One launch per 64 samples. */
int vfi_triplet_batch_prepare(const unsigned char *src, const int *params, float *rgb, long long rgb_slot_stride,
                              long long rgb_batch_stride, float *lab, long long lab_slot_stride, long long lab_batch_stride,
                              int B, int Hs, int Ws, int h, int w, vfi_stream_t stream);

/* The same batch from the frames of a clip as they lie in a YUV4MPEG2 file: the crop, flips and slot
 * choice above applied to what vfi_yuv_to_rgb gives for each whole frame, in one pass that decodes only the blocks of the
 * frame a crop touches.
 *   src     DEVICE uint8: frame f (0, 1, 2) of sample b starts at src + (3 b + f) * frame_stride, in the frame layout of
 *           "Clip I/O" below (luma, Cb, Cr; 4:2:0 or 4:4:4); frame_stride >= the frame's bytes, any alignment
 *   format  HOST int[4] of vfi_yuv_to_rgb (subsampling, siting, matrix, range)
 *   params, rgb, lab and their strides: as vfi_triplet_batch_prepare; i and j may be odd in 4:2:0
 * Chroma is up-sampled with indices clamped at the frame's edges, never at the crop's; range, matrix and the clamp to
 * [0, 1] are vfi_yuv_to_rgb's, and a pixel gets that call's bits (same block ownership, same per-pixel code); Lab is computed
 * from the clamped rgb in registers.  One launch per 64 samples, no workspace, no atomics, one writer per float.
 * Checked before anything is enqueued, nothing written: VFI_ERR_INVALID_ARG for a null src, format or params, both outputs
 * NULL, a size <= 0, an unknown format field, a crop that leaves the source, flags outside 0..7, a stride below 3 * h * w,
 * frame_stride below the frame's bytes; VFI_ERR_SHAPE for odd Hs or Ws in 4:2:0; VFI_ERR_UNSUPPORTED for Hs * Ws > 2^28. */
int vfi_yuv_triplet_batch_prepare(const unsigned char *src, long long frame_stride, const int *format, const int *params,
                                  float *rgb, long long rgb_slot_stride, long long rgb_batch_stride, float *lab,
                                  long long lab_slot_stride, long long lab_batch_stride, int B, int Hs, int Ws, int h, int w,
                                  vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * LPIPS (piq.LPIPS, reference src/evaluation/evaluate_image.py:22): the head on one tap of the VGG16 trunk, its adjoint,
 * and the input normalisation.  DESIGN.md section 24.  Same rules as the training paths above: no float atomics, one
 * writer per element, an order of summation fixed by C and HW alone -- the bits of image n's value depend neither on N
 * nor on n.
 * ---------------------------------------------------------------------------------- */

/* out[n] = (prior ? prior[n] : 0) + 1 / HW * sum_p sum_c w[c] (xh_c - yh_c)^2 with xh_c = x_c / (sqrt(sum_k x_k^2) + 1e-10)
 * at every pixel, yh likewise.  x, y (N, C, HW) fp32 with a batch stride each, any 4-byte alignment (they may be the two
 * halves of one tensor); w: C floats; prior, out: N floats (out may be prior).  `workspace`: VFI_REDUCE_WORKSPACE_FLOATS.
 * x == y gives exactly 0. */
int vfi_lpips_head_forward(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *w,
                           const float *prior, float *out, float *workspace, int N, int C, int HW, vfi_stream_t stream);

/* grad_x = (above + upstream[n] * d(head value of image n) / dx) * [x > 0 when relu_mask], in one pass; no gradient for y
 * or w.  With s = |x| + 1e-10, t = |y| + 1e-10, e_c = 2 w_c (x_c / s - y_c / t):
 *   d/dx_c = 1 / HW * (e_c / s - (sum_k e_k x_k) x_c / (|x| s^2)),   and 0 at a pixel with |x| = 0.
 * above (optional, NULL = 0): the gradient arriving at x from the layers above, added exactly; grad_x may be `above`. */
int vfi_lpips_head_backward(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *w,
                            const float *upstream, const float *above, long long above_bstride, float *grad_x,
                            long long gx_bstride, int N, int C, int HW, int relu_mask, vfi_stream_t stream);

/* out = (x - mean_c) / std_c per channel of (N, 3, HW) images in [0, 1], mean = (0.485, 0.456, 0.406),
 * std = (0.229, 0.224, 0.225); adjoint != 0: out = x / std_c, the gradient's way back.  In place allowed. */
int vfi_lpips_normalize(const float *x, long long x_bstride, float *out, long long out_bstride, int N, int HW, int adjoint,
                        vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * SSIM as a loss (piq.SSIMLoss, imported at reference src/fusion_net/trainer.py:13).  DESIGN.md section 26.  The rules of
 * the training paths: no float atomics, one writer per element, an order of summation fixed by (C, H, W) alone -- the
 * bits of image n's value and gradient depend neither on N nor on n.
 *   taps g[i] ~ exp(-(i - r)^2 / (2 sigma^2)), r = kernel_size / 2, normalised (made on the host in double, rounded once)
 *   mu_x = G*x, mu_y = G*y, Exx = G*x^2, Eyy = G*y^2, Exy = G*xy, separable, valid region (H - 2r) x (W - 2r) only
 *   sxx = Exx - mu_x^2, syy = Eyy - mu_y^2, sxy = Exy - mu_x mu_y
 *   ssim = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * (2 sxy + c2) / (sxx + syy + c2)
 * x, y: (N, C, H, W) fp32 with a batch stride each, any 4-byte alignment (they may be the two halves of one tensor).
 * kernel_size odd, 3 ... 11, sigma > 0, N, C >= 1, else VFI_ERR_INVALID_ARG; H or W below kernel_size is VFI_ERR_SHAPE;
 * nothing is written in either case.
 * ---------------------------------------------------------------------------------- */

/* out[n] = 1 - mean of ssim over C * (H - 2r) * (W - 2r), in one pass over x and y (the moments stay on the CU).
 * `workspace`: VFI_REDUCE_WORKSPACE_FLOATS.  x == y gives exactly 0. */
int vfi_ssim_loss_forward(const float *x, long long x_bstride, const float *y, long long y_bstride, float *out,
                          float *workspace, int N, int C, int H, int W, int kernel_size, float sigma, float c1, float c2,
                          vfi_stream_t stream);

/* grad_x = upstream[n] * d out[n] / dx, gather form; x and y are all it reads.  No gradient for y: SSIM is symmetric, call
 * with x and y exchanged.  With count = C (H - 2r) (W - 2r), l and cs the two factors above, D1 and D2 their denominators,
 *   B = -l cs / D2,  Cm = 2 l / D2,  A = cs (2 mu_y / D1 - 2 mu_x l / D1) - 2 mu_x B - mu_y Cm   (0 outside the valid region)
 *   grad_x(q) = -upstream[n] / count * ((G (*) A)(q) + 2 x(q) (G (*) B)(q) + y(q) (G (*) Cm)(q)),  (*) the full correlation. */
int vfi_ssim_loss_backward(const float *x, long long x_bstride, const float *y, long long y_bstride, const float *upstream,
                           float *grad_x, long long gx_bstride, int N, int C, int H, int W, int kernel_size, float sigma,
                           float c1, float c2, vfi_stream_t stream);

/* Adjoint of vfi_avg_pool: grad (planes, H/f, W/f) -> grad_x (planes, H, W), dense; every pixel of a window gets grad / f^2,
 * the rows and columns the floor drops get exactly 0. */
int vfi_avg_pool_backward(const float *grad, float *grad_x, int planes, int H, int W, int f, vfi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Optimiser step (torch.optim.SGD / Adam / Adamax / RMSprop as the trainers configure them): one multi-tensor pass that
 * reads and writes every element once.  DESIGN.md section 29.  The arithmetic restates torch/optim's _single_tensor_*
 * functions operation by operation in fp32 (no contraction); every scalar is derived in double and rounded once.
 *   SGD      g += wd p;  buf = g on first_step, else momentum buf + (1 - dampening) g;  g = nesterov ? g + momentum buf : buf;
 *            p -= lr g.  momentum == 0: no buffer, state0 is not read.                       state0 = momentum_buffer
 *   ADAM     g += wd p;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *            p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)                                 state0 = exp_avg, state1 = exp_avg_sq
 *   ADAMAX   g += wd p;  m as ADAM;  u = max(beta2 u, |g| + eps);  p -= (lr / bc1) m / u      state0 = exp_avg, state1 = exp_inf
 *   RMSPROP  g += wd p;  s = alpha s + (1 - alpha) g^2;  p -= lr g / (sqrt(s) + eps)          state0 = square_avg
 * (g += wd p changes the local copy only: grad is never written.)  With has_clamp the new p is clamped to
 * [clamp_min, clamp_max] in the same pass, the bits of Tensor.clamp_ afterwards.
 * ---------------------------------------------------------------------------------- */
#define VFI_OPTIM_SGD 0
#define VFI_OPTIM_ADAM 1
#define VFI_OPTIM_ADAMAX 2
#define VFI_OPTIM_RMSPROP 3
#define VFI_OPTIM_CHUNK 4096               /* elements one workgroup takes */
#define VFI_OPTIM_TENSORS_PER_LAUNCH 40    /* both tables travel in the launch's 4 KiB of kernel arguments */
#define VFI_OPTIM_CHUNKS_PER_LAUNCH 2048
#define VFI_OPTIM_MAX_NUMEL (1LL << 40)    /* per tensor; element offsets are 64-bit */

typedef struct vfi_optim_tensor {
    float *param;       /* device, numel floats, 4-byte aligned; 16-byte accesses when all four pointers allow */
    const float *grad;  /* device, read only */
    float *state0;      /* see the table above; may be NULL where the kind does not use it */
    float *state1;
    long long numel;
} vfi_optim_tensor;

typedef struct vfi_optim_hyper {
    double lr, beta1, beta2, alpha, eps, weight_decay, momentum, dampening;
    double bias_correction1, bias_correction2; /* 1 - beta^step, from the step count in double (ADAM, ADAMAX) */
    double clamp_min, clamp_max;
    int nesterov, first_step, has_clamp;       /* first_step: SGD with momentum, the buffer is created (buf = g) */
} vfi_optim_hyper;

/* One update of `count` tensors that share `hyper` (HOST arrays, read before the call returns).  A workgroup takes one
 * chunk of one tensor; a launch carries at most VFI_OPTIM_TENSORS_PER_LAUNCH tensors and VFI_OPTIM_CHUNKS_PER_LAUNCH chunks
 * (a tensor may continue in the next launch), so the call is ceil(work / capacity) launches and nothing else: no device
 * allocation, no copy, no wait.  The tensors must not overlap.
 * Checked before anything touches a device: an unknown kind, count <= 0, null tensors or hyper, a record with a null param
 * or grad, a null state the kind uses, or numel <= 0, and hyper-parameters outside torch's own ranges are
 * VFI_ERR_INVALID_ARG; numel above VFI_OPTIM_MAX_NUMEL is VFI_ERR_UNSUPPORTED. */
int vfi_optim_step(int kind, const vfi_optim_tensor *tensors, int count, const vfi_optim_hyper *hyper, vfi_stream_t stream);

/* The limits above at run time (no device): elements per chunk, tensors and chunks per launch, the largest numel. */
int vfi_optim_limits(long long *chunk, int *tensors_per_launch, int *chunks_per_launch, long long *max_numel);

/* ------------------------------------------------------------------------------------
 * Clip I/O: the frames of a YUV4MPEG2 stream to and from the tensors of the fused frame.  DESIGN.md section 30.
 *   frame   DEVICE uint8, dense, any byte alignment, the stream's own layout: H * W luma bytes, then Cb, then Cr;
 *           each chroma plane (H / 2) * (W / 2) bytes in 4:2:0 (H and W even), H * W bytes in 4:4:4 (any H, W >= 1)
 *   format  HOST int[4] = (subsampling, horizontal chroma siting, matrix, range), the constants below; vertical siting is
 *           always centre, the siting field is not used in 4:4:4 (but must hold one of its two values)
 * With (Kr, Kb) = (0.2126, 0.0722) for BT.709 and (0.299, 0.114) for BT.601, Kg = 1 - Kr - Kb, and
 * (y_off, y_scale, c_scale) = (16, 219, 224) for limited range (Y 16...235, C 16...240), (0, 255, 255) for full range.
 * Both are single streaming launches: no workspace, no atomics, one writer per byte, the same bits on every call.
 * Checked before anything is enqueued, nothing written: null pointers, H or W <= 0 and a format field that is none of its
 * constants are VFI_ERR_INVALID_ARG; odd H or W in 4:2:0 is VFI_ERR_SHAPE; H * W >= 2^31 is VFI_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------- */
#define VFI_YUV_420 0
#define VFI_YUV_444 1
#define VFI_YUV_SITING_CENTRE 0 /* C420jpeg, C420paldv: chroma between luma columns 2i and 2i + 1 */
#define VFI_YUV_SITING_LEFT 1   /* C420mpeg2, C420: chroma on luma column 2i */
#define VFI_YUV_BT709 0
#define VFI_YUV_BT601 1
#define VFI_YUV_LIMITED 0
#define VFI_YUV_FULL 1

/* Decode.  rgb, lab_a, lab_b: (3, H, W) float32, 4-byte aligned (16-byte stores where a row segment allows), each may be
 * NULL but not all three (VFI_ERR_INVALID_ARG); lab_a and lab_b receive the same bits (a frame is the second frame of one
 * pair and the first of the next: it lands in two (6, H, W) Lab buffers from one read).  In float32:
 *   y = (Y - y_off) / y_scale, cb = (Cb - 128) / c_scale, cr = (Cr - 128) / c_scale
 *   R = y + 2 (1 - Kr) cr,  B = y + 2 (1 - Kb) cb,  G = (y - Kr R - Kb B) / Kg,  each then clamped to [0, 1]
 *   lab = vfi_rgb2lab's formulas on the clamped rgb (its accuracy, not its bits)
 * 4:2:0 chroma at luma pixel (r, x) is bilinear over the chroma bytes c, indices clamped to the plane: vertically, and
 * horizontally for centre siting, even r takes c[r/2 - 1] / 4 + 3 c[r/2] / 4 and odd r takes 3 c[(r-1)/2] / 4 + c[(r+1)/2] / 4;
 * for left siting even x takes c[x/2] and odd x takes (c[(x-1)/2] + c[(x+1)/2]) / 2. */
int vfi_yuv_to_rgb(const unsigned char *frame, int H, int W, const int *format, float *rgb, float *lab_a, float *lab_b,
                   vfi_stream_t stream);

/* Encode.  rgb (3, H, W) float32, 4-byte aligned, clamped to [0, 1] first (torchvision.save_image's clamp).  At full
 * resolution y = Kr R + Kg G + Kb B, cb = (B - y) / (2 (1 - Kb)), cr = (R - y) / (2 (1 - Kr)).  4:2:0 takes the mean of
 * rows 2j and 2j + 1, then for centre siting the mean of columns 2i and 2i + 1, for left siting
 * (c[2i - 1] + 2 c[2i] + c[2i + 1]) / 4 with the column index clamped.  Y = y_off + y_scale y, C = 128 + c_scale c, then
 * floor(v + 0.5), then the clamp to the range's limits.  A NaN in rgb gives the lower limit in every byte it reaches. */
int vfi_rgb_to_yuv(const float *rgb, int H, int W, const int *format, unsigned char *frame, vfi_stream_t stream);

/* Scene cuts, decided on the device: the statistic and the decision stay in device words, so the
 * thread that enqueues a clip never waits for either.  Both calls check before anything is enqueued, nothing written: a
 * null pointer (except where NULL is allowed below) or a size <= 0 is VFI_ERR_INVALID_ARG, a size >= 2^31 is
 * VFI_ERR_UNSUPPORTED.
 *
 * Sum of absolute differences: *sad = sum over i < n of |a[i] - b[i]|, exact.  a, b: DEVICE bytes of any alignment,
 * independent of each other (the clip loop passes two frames and n = H * W, the luma plane); sad: one DEVICE 64-bit word,
 * 8-byte aligned.  What *sad held before does not matter: the call zeroes it on `stream`, then each workgroup adds one
 * 64-bit integer to it, so every call gives the same bits. */
int vfi_luma_sad(const unsigned char *a, const unsigned char *b, long long n, unsigned long long *sad, vfi_stream_t stream);

/* With p = sad_prev ? *sad_prev : 0 and s = min(*sad, |*sad - p|) (the difference without unsigned wrap), the pair is a
 * cut when s >= min_sad; min_sad = 0 always is.  On a cut dst[0, nbytes) = src[0, nbytes); otherwise dst is not written.
 * cut (one DEVICE int, may be NULL) receives 1 or 0 either way.  dst, src: DEVICE bytes of any alignment, independent of
 * each other, not overlapping; sad, sad_prev: DEVICE 64-bit words as vfi_luma_sad writes them, sad_prev may be NULL.
 * This is the rule ffmpeg's scdet filter documents, in integers: with the mean absolute luma difference in percent
 * m = 100 sad / (255 n), the score is min(m, |m - m_prev|) (m_prev = 0 for the first pair) and a cut is score >= threshold;
 * the host passes min_sad = ceil(threshold * 255 * n / 100). */
int vfi_frame_pick(unsigned char *dst, const unsigned char *src, long long nbytes, const unsigned long long *sad,
                   const unsigned long long *sad_prev, unsigned long long min_sad, int *cut, vfi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_H */
