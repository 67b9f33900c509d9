// Gradient accumulation of a mixed-scale training step in one launch per backward.
//
// The reference's step (train.py:110-146) runs several (lr, hr) pairs of different sizes and scales, averages their losses and
// steps the optimizer once, so a parameter's gradient is the sum over the samples that used it.  Here every group of samples
// runs its own backward (accumulate.py) and its gradients are added into one persistent flat fp32 arena.  Left to torch that is
// one aten add_ per parameter and backward (~100 launches for a FastTransformer scale); this is one launch for all of them,
// table-driven like tup_adam_step (pack_plan.hip): a segment table carries the pointers, a chunk table maps workgroups to
// (segment, first element).
//   mode 0: dst = alpha * src         (a parameter's first gradient of the step: the arena is never zero-filled as a whole)
//   mode 1: dst = dst + alpha * src   (later gradients)
//   mode 2: dst = 0                   (segments this rank did not touch, before the per-step all-reduce)
// alpha * src is rounded before the add (no fused multiply-add), so with alpha == 1 mode 1 is torch's `grad += g` to the bit and
// mode 0 a copy.  Every element has exactly one writer: no atomics.
// Bound: HBM (mode 1: 8 B read + 4 B written per element).
#include "common.h"

struct AccSeg {
    float* dst; const float* src;
    long long n;
    float alpha; int mode;
};
static_assert(sizeof(AccSeg) == 32, "segment record = 32 bytes (the host packs it as 4 int64 words)");

namespace {
constexpr int ACC_CHUNK = 4096;

template <int MODE>
__device__ __forceinline__ float acc_one(float d, float s, float alpha)
{
#pragma clang fp contract(off)
    if constexpr (MODE == 0) return alpha * s;
    else if constexpr (MODE == 1) { const float t = alpha * s; return d + t; }
    else return 0.f;
}

template <int MODE>
__device__ __forceinline__ void acc_chunk(const AccSeg& s, long long first, long long end)
{
    float* __restrict__ dst = s.dst;
    const float* __restrict__ src = s.src;
    const float alpha = s.alpha;
    // `first` is a multiple of 4096, so the chunk start is 16-byte aligned when the segment bases are
    const bool vec = ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) && (MODE == 2 || (reinterpret_cast<uintptr_t>(src) & 15) == 0);
    long long i = first;
    if (vec) {
        const long long nvec = (end - first) >> 2;
        for (long long v = threadIdx.x; v < nvec; v += 256) {
            const long long e = first + 4 * v;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f), g = d;
            if constexpr (MODE != 2) g = *reinterpret_cast<const float4*>(src + e);
            if constexpr (MODE == 1) d = *reinterpret_cast<const float4*>(dst + e);
            d.x = acc_one<MODE>(d.x, g.x, alpha); d.y = acc_one<MODE>(d.y, g.y, alpha);
            d.z = acc_one<MODE>(d.z, g.z, alpha); d.w = acc_one<MODE>(d.w, g.w, alpha);
            *reinterpret_cast<float4*>(dst + e) = d;
        }
        i = first + 4 * nvec;          // scalar tail: at most 3 elements
    }
    for (i += threadIdx.x; i < end; i += 256) {
        float d = 0.f, g = 0.f;
        if constexpr (MODE != 2) g = src[i];
        if constexpr (MODE == 1) d = dst[i];
        dst[i] = acc_one<MODE>(d, g, alpha);
    }
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const AccSeg* __restrict__ segs, const int* __restrict__ chunks)
{
    const int seg = chunks[2 * blockIdx.x], first = chunks[2 * blockIdx.x + 1];
    const AccSeg s = segs[seg];
    if (first >= s.n) return;
    const long long end = min((long long)first + ACC_CHUNK, s.n);
    if (s.mode == 0) acc_chunk<0>(s, first, end);
    else if (s.mode == 1) acc_chunk<1>(s, first, end);
    else acc_chunk<2>(s, first, end);
}
}  // namespace

// segs: device array [nseg] of 32-byte records {float* dst; const float* src; long long n; float alpha; int mode}; chunks: device
// int [nchunks][2] = (segment index, first element), one workgroup per 4096 elements.  Segments must not overlap each other.
extern "C" int tup_grad_accumulate(const void* segs, const int* chunks, int nchunks, void* stream)
{
    if (nchunks <= 0) return 0;
    grad_accumulate_kernel<<<dim3((unsigned)nchunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>((const AccSeg*)segs, chunks);
    TUP_CHECK_LAUNCH();
    return 0;
}
