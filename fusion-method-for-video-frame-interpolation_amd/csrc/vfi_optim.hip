// Optimiser step on the device (gfx950): SGD, Adam, Adamax and RMSprop over a list of tensors in one multi-tensor pass.
// DESIGN.md section 29.
//
// A workgroup of 256 threads takes one chunk (kChunk = 4096 consecutive elements) of one tensor.  A launch carries its two
// tables in its kernel arguments (4 KiB, the limit that governs MultiRowsT in vfi_pyramid.hip):
//   t[kTensors]       the tensors of this launch: param, grad, state0, state1, numel, and `bias` = (the tensor's chunk that
//                     the launch's first workgroup on it takes) - (that workgroup's index)
//   owner[kChunks]    workgroup -> index into t; the workgroup's chunk of that tensor is blockIdx.x + bias
// so a step is ceil(work / table capacity) launches, with no device allocation, no copy of a table and no host wait.  A
// tensor larger than what is left of a launch continues in the next one.
//
// Every element is read once and written once: p, g and the state come in as 16-byte vectors where all pointers of the
// tensor are 16-byte aligned (chunks start at multiples of 4096 elements, so a chunk is aligned as its tensor is), else as
// single floats; a full chunk issues all its loads before the first store.  The last chunk's tail (numel % 4 elements behind
// the vectors) is done by the same workgroup.  Element offsets are 64-bit throughout.
//
// The arithmetic restates torch/optim's _single_tensor_* functions operation by operation: every product, sum, quotient and
// square root is rounded to fp32 on its own (contraction off; hipcc's fp32 divide and sqrt are correctly rounded), and
// every scalar is derived on the host in double and rounded once, as torch rounds a Python scalar handed to an fp32 op.
#include "vfi_common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;                                   // floats per 16-byte access
constexpr int kIters = 4;                                 // vectors per thread in a full chunk
constexpr int kChunk = kThreads * kVec * kIters;          // VFI_OPTIM_CHUNK
constexpr int kTensors = VFI_OPTIM_TENSORS_PER_LAUNCH;
constexpr int kChunks = VFI_OPTIM_CHUNKS_PER_LAUNCH;
static_assert(kChunk == VFI_OPTIM_CHUNK, "include/vfi_hip.h states the chunk");
static_assert(kTensors <= 256, "owner[] is a byte");

struct Tensor {
    float *p;
    const float *g;
    float *s0, *s1;
    long long numel;
    long long bias;
};

struct Scalars {
    float wd;                   // weight decay (0: none)
    float a, one_minus_a;       // SGD: momentum, 1 - dampening.  Adam/Adamax: 1 - beta1 and 1 - that.  RMSprop: alpha, 1 - alpha
    float b, one_minus_b;       // Adam/Adamax: beta2, 1 - beta2
    float eps;
    float neg_step;             // -lr (SGD, RMSprop), -lr / bias_correction1 (Adam, Adamax)
    float bc2_sqrt;             // Adam: sqrt(bias_correction2)
    float lo, hi;               // clamp interval
    int flags;
};
enum : int { kFirst = 1, kNesterov = 2, kClamp = 4, kMomentum = 8, kDecay = 16 };

struct Table {
    Tensor t[kTensors];
    unsigned char owner[kChunks];
    Scalars h;
};
static_assert(sizeof(Table) <= 4096, "kernel arguments are limited to 4 KiB");

// torch's lerp with a scalar weight (aten/src/ATen/native/Lerp.h): exact at weight 1, which betas = (0, 0.9) gives
__device__ __forceinline__ float lerp(float a, float b, float w, float one_minus_w) {
    const float d = b - a;
    return fabsf(w) < 0.5f ? a + w * d : b - d * one_minus_w;
}

template <int KIND>
struct Update;

template <>
struct Update<VFI_OPTIM_SGD> {
    static constexpr int kStates = 1;
    static __device__ __forceinline__ void apply(const Scalars &h, float &p, float g, float &buf, float &) {
        if (h.flags & kDecay) g = g + h.wd * p;
        if (h.flags & kMomentum) {
            buf = (h.flags & kFirst) ? g : buf * h.a + h.one_minus_a * g;
            g = (h.flags & kNesterov) ? g + h.a * buf : buf;
        }
        p = p + h.neg_step * g;
    }
};

template <>
struct Update<VFI_OPTIM_ADAM> {
    static constexpr int kStates = 2;
    static __device__ __forceinline__ void apply(const Scalars &h, float &p, float g, float &m, float &v) {
        if (h.flags & kDecay) g = g + h.wd * p;
        m = lerp(m, g, h.a, h.one_minus_a);
        v = v * h.b;
        v = v + h.one_minus_b * g * g;
        const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
        p = p + h.neg_step * (m / denom);
    }
};

template <>
struct Update<VFI_OPTIM_ADAMAX> {
    static constexpr int kStates = 2;
    static __device__ __forceinline__ void apply(const Scalars &h, float &p, float g, float &m, float &u) {
        if (h.flags & kDecay) g = g + h.wd * p;
        m = lerp(m, g, h.a, h.one_minus_a);
        const float x = u * h.b, y = fabsf(g) + h.eps;
        u = (x > y || x != x) ? x : y;          // torch.maximum: a NaN on either side stays
        p = p + h.neg_step * (m / u);
    }
};

template <>
struct Update<VFI_OPTIM_RMSPROP> {
    static constexpr int kStates = 1;
    static __device__ __forceinline__ void apply(const Scalars &h, float &p, float g, float &s, float &) {
        if (h.flags & kDecay) g = g + h.wd * p;
        s = s * h.a;
        s = s + h.one_minus_a * g * g;
        const float avg = sqrtf(s) + h.eps;
        p = p + h.neg_step * (g / avg);
    }
};

// Tensor.clamp_(lo, hi): a NaN stays a NaN
__device__ __forceinline__ float clamp(const Scalars &h, float p) {
    if (!(h.flags & kClamp)) return p;
    return p < h.lo ? h.lo : (p > h.hi ? h.hi : p);
}

template <int KIND, bool S0>
__device__ __forceinline__ void update_one(const Scalars &h, const Tensor &t, long long i) {
    float p = t.p[i], s0 = S0 ? t.s0[i] : 0.0f, s1 = Update<KIND>::kStates > 1 ? t.s1[i] : 0.0f;
    Update<KIND>::apply(h, p, t.g[i], s0, s1);
    t.p[i] = clamp(h, p);
    if (S0) t.s0[i] = s0;
    if (Update<KIND>::kStates > 1) t.s1[i] = s1;
}

template <int KIND, bool S0>
__device__ __forceinline__ void update_vec(const Scalars &h, float4 &p, const float4 &g, float4 &s0, float4 &s1) {
    Update<KIND>::apply(h, p.x, g.x, s0.x, s1.x);
    Update<KIND>::apply(h, p.y, g.y, s0.y, s1.y);
    Update<KIND>::apply(h, p.z, g.z, s0.z, s1.z);
    Update<KIND>::apply(h, p.w, g.w, s0.w, s1.w);
    p.x = clamp(h, p.x); p.y = clamp(h, p.y); p.z = clamp(h, p.z); p.w = clamp(h, p.w);
}

// S0: the kind keeps a first state array (false: SGD without momentum, whose s0 is NULL)
template <int KIND, bool S0>
__global__ __launch_bounds__(kThreads) void optim_step_kernel(const Table tab) {
    constexpr bool S1 = Update<KIND>::kStates > 1;
    const Tensor &t = tab.t[tab.owner[blockIdx.x]];
    const Scalars &h = tab.h;
    const long long base = ((long long)blockIdx.x + t.bias) * kChunk;       // < numel by construction of the table
    const long long left = t.numel - base;
    const int n = left < kChunk ? (int)left : kChunk;
    const uintptr_t bits = (uintptr_t)t.p | (uintptr_t)t.g | (S0 ? (uintptr_t)t.s0 : 0) | (S1 ? (uintptr_t)t.s1 : 0);
    if (bits & 15) {                          // a view at an odd offset: 4-byte accesses for this tensor
        for (int i = threadIdx.x; i < n; i += kThreads) update_one<KIND, S0>(h, t, base + i);
        return;
    }
    float4 *pv = reinterpret_cast<float4 *>(t.p + base);
    const float4 *gv = reinterpret_cast<const float4 *>(t.g + base);
    float4 *av = S0 ? reinterpret_cast<float4 *>(t.s0 + base) : nullptr;
    float4 *bv = S1 ? reinterpret_cast<float4 *>(t.s1 + base) : nullptr;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (n == kChunk) {                        // every load of the chunk is in flight before the first store
        float4 p[kIters], g[kIters], a[kIters], b[kIters];
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const int i = k * kThreads + threadIdx.x;
            p[k] = pv[i];
            g[k] = gv[i];
            a[k] = S0 ? av[i] : zero;
            b[k] = S1 ? bv[i] : zero;
        }
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const int i = k * kThreads + threadIdx.x;
            update_vec<KIND, S0>(h, p[k], g[k], a[k], b[k]);
            pv[i] = p[k];
            if (S0) av[i] = a[k];
            if (S1) bv[i] = b[k];
        }
        return;
    }
    const int nv = n / kVec;
    for (int i = threadIdx.x; i < nv; i += kThreads) {
        float4 p = pv[i], a = S0 ? av[i] : zero, b = S1 ? bv[i] : zero;
        update_vec<KIND, S0>(h, p, gv[i], a, b);
        pv[i] = p;
        if (S0) av[i] = a;
        if (S1) bv[i] = b;
    }
    const int tail = nv * kVec + threadIdx.x;             // numel % 4 elements behind the vectors
    if (tail < n) update_one<KIND, S0>(h, t, base + tail);
}

template <int KIND, bool S0>
int launch(const Table &tab, int blocks, hipStream_t s) {
    hipLaunchKernelGGL((optim_step_kernel<KIND, S0>), dim3(blocks), dim3(kThreads), 0, s, tab);
    return vfi::check_launch("vfi_optim_step");
}

int launch_kind(int kind, bool s0, const Table &tab, int blocks, hipStream_t s) {
    switch (kind) {
    case VFI_OPTIM_SGD: return s0 ? launch<VFI_OPTIM_SGD, true>(tab, blocks, s) : launch<VFI_OPTIM_SGD, false>(tab, blocks, s);
    case VFI_OPTIM_ADAM: return launch<VFI_OPTIM_ADAM, true>(tab, blocks, s);
    case VFI_OPTIM_ADAMAX: return launch<VFI_OPTIM_ADAMAX, true>(tab, blocks, s);
    default: return launch<VFI_OPTIM_RMSPROP, true>(tab, blocks, s);
    }
}

bool finite_nonneg(double x) { return std::isfinite(x) && x >= 0.0; }

}  // namespace

extern "C" int vfi_optim_limits(long long *chunk, int *tensors_per_launch, int *chunks_per_launch, long long *max_numel) {
    VFI_REQUIRE(chunk && tensors_per_launch && chunks_per_launch && max_numel, VFI_ERR_INVALID_ARG, "vfi_optim_limits: null pointer");
    *chunk = kChunk;
    *tensors_per_launch = kTensors;
    *chunks_per_launch = kChunks;
    *max_numel = VFI_OPTIM_MAX_NUMEL;
    return VFI_OK;
}

extern "C" int vfi_optim_step(int kind, const vfi_optim_tensor *tensors, int count, const vfi_optim_hyper *hyper,
                              vfi_stream_t stream) {
    VFI_REQUIRE(kind >= VFI_OPTIM_SGD && kind <= VFI_OPTIM_RMSPROP, VFI_ERR_INVALID_ARG, "vfi_optim_step: unknown kind %d", kind);
    VFI_REQUIRE(tensors && hyper, VFI_ERR_INVALID_ARG, "vfi_optim_step: null tensors or hyper");
    VFI_REQUIRE(count > 0, VFI_ERR_INVALID_ARG, "vfi_optim_step: count %d", count);
    const vfi_optim_hyper &y = *hyper;
    VFI_REQUIRE(std::isfinite(y.lr) && finite_nonneg(y.weight_decay) && finite_nonneg(y.eps), VFI_ERR_INVALID_ARG,
                "vfi_optim_step: lr, weight_decay or eps out of range");
    const bool momentum = kind == VFI_OPTIM_SGD && y.momentum != 0.0;
    const bool need_s0 = kind != VFI_OPTIM_SGD || momentum, need_s1 = kind == VFI_OPTIM_ADAM || kind == VFI_OPTIM_ADAMAX;
    if (need_s1)
        VFI_REQUIRE(y.beta1 >= 0.0 && y.beta1 < 1.0 && y.beta2 >= 0.0 && y.beta2 < 1.0 && y.bias_correction1 > 0.0 &&
                        y.bias_correction1 <= 1.0 && y.bias_correction2 > 0.0 && y.bias_correction2 <= 1.0,
                    VFI_ERR_INVALID_ARG, "vfi_optim_step: betas outside [0, 1) or a bias correction outside (0, 1]");
    if (kind == VFI_OPTIM_RMSPROP) VFI_REQUIRE(finite_nonneg(y.alpha), VFI_ERR_INVALID_ARG, "vfi_optim_step: alpha %g", y.alpha);
    if (kind == VFI_OPTIM_SGD)
        VFI_REQUIRE(finite_nonneg(y.momentum) && std::isfinite(y.dampening) &&
                        (!y.nesterov || (y.momentum > 0.0 && y.dampening == 0.0)),
                    VFI_ERR_INVALID_ARG, "vfi_optim_step: nesterov needs a momentum and no dampening");
    if (y.has_clamp) VFI_REQUIRE(y.clamp_min <= y.clamp_max, VFI_ERR_INVALID_ARG, "vfi_optim_step: empty clamp interval");
    for (int i = 0; i < count; ++i) {
        const vfi_optim_tensor &r = tensors[i];
        VFI_REQUIRE(r.param && r.grad && r.numel > 0 && (!need_s0 || r.state0) && (!need_s1 || r.state1), VFI_ERR_INVALID_ARG,
                    "vfi_optim_step: record %d has a null param, grad or state, or numel %lld", i, r.numel);
        VFI_REQUIRE(r.numel <= VFI_OPTIM_MAX_NUMEL, VFI_ERR_UNSUPPORTED, "vfi_optim_step: record %d: numel %lld above %lld", i,
                    r.numel, (long long)VFI_OPTIM_MAX_NUMEL);
    }

    Table tab;
    Scalars &h = tab.h;
    h = Scalars{};
    h.wd = (float)y.weight_decay;
    h.eps = (float)y.eps;
    h.flags = (y.weight_decay != 0.0 ? kDecay : 0) | (y.has_clamp ? kClamp : 0);
    h.lo = (float)y.clamp_min;
    h.hi = (float)y.clamp_max;
    if (kind == VFI_OPTIM_SGD) {
        h.a = (float)y.momentum;
        h.one_minus_a = (float)(1.0 - y.dampening);
        h.neg_step = (float)-y.lr;
        h.flags |= (momentum ? kMomentum : 0) | (y.first_step ? kFirst : 0) | (y.nesterov ? kNesterov : 0);
    } else if (need_s1) {
        h.a = (float)(1.0 - y.beta1);
        h.one_minus_a = 1.0f - h.a;                 // Lerp.h subtracts in the tensor's precision
        h.b = (float)y.beta2;
        h.one_minus_b = (float)(1.0 - y.beta2);
        h.neg_step = (float)-(y.lr / y.bias_correction1);
        h.bc2_sqrt = (float)std::sqrt(y.bias_correction2);
    } else {
        h.a = (float)y.alpha;
        h.one_minus_a = (float)(1.0 - y.alpha);
        h.neg_step = (float)-y.lr;
    }

    // fill launches: a launch is closed when either table is full
    hipStream_t s = vfi::as_stream(stream);
    int nt = 0, nb = 0;
    for (int i = 0; i < count; ++i) {
        const vfi_optim_tensor &r = tensors[i];
        const long long chunks = (r.numel + kChunk - 1) / kChunk;
        long long done = 0;
        while (done < chunks) {
            if (nt == kTensors || nb == kChunks) {
                if (int e = launch_kind(kind, need_s0, tab, nb, s)) return e;
                nt = nb = 0;
            }
            const long long take = chunks - done < kChunks - nb ? chunks - done : kChunks - nb;
            Tensor &t = tab.t[nt];
            t.p = r.param;
            t.g = r.grad;
            t.s0 = need_s0 ? r.state0 : nullptr;
            t.s1 = need_s1 ? r.state1 : nullptr;
            t.numel = r.numel;
            t.bias = done - nb;
            for (long long k = 0; k < take; ++k) tab.owner[nb + k] = (unsigned char)nt;
            nb += (int)take;
            done += take;
            ++nt;
        }
    }
    return launch_kind(kind, need_s0, tab, nb, s);
}
