// The guarded optimizer step: global gradient norm, clip coefficient and apply / skip decision on the device, and an Adam / AdamW
// update that reads them -- no host synchronisation inside a step.
//
// The reference steps through GradScaler (train.py:136-139), which skips an optimizer step whose gradients hold an inf or a NaN;
// torch's clip_grad_norm_ scales all gradients by min(1, max_norm / (norm + 1e-6)).  Done with torch, both cost ~100 small
// launches per step and the skip a host synchronisation.  Here a step is at most three launches:
//   1. grad_sumsq_kernel   table-driven like tup_adam_step: one workgroup per 4096 gradient elements, every lane converts g to
//                          double and accumulates g * g in double, the workgroup writes ONE double partial;
//   2. guard_finish_kernel one workgroup sums the partials in a fixed order and writes the guard record (below);
//   3. adam_guarded_kernel tup_adam_step's update with weight decay, reading coef and apply from the guard record with a uniform
//                          load: apply == 0 returns before p, m or v are written, otherwise coef * g is the gradient.  The
//                          gradients themselves are not rewritten: p.grad keeps the unclipped values.
// There is no floating-point atomic on this path and every sum has one fixed order (per lane: ascending elements; per workgroup:
// a fixed LDS tree; over workgroups: ascending stripes, then the same tree), so the record is bitwise reproducible from run to
// run, with or without ops.deterministic.
// Bound: HBM.  The norm pass reads the gradients once (4 B per element); the step moves 4 reads + 3 writes as tup_adam_step.
//
// tup_adam_step_ema is the same step with an exponential moving average of the weights kept in the same launch (adam_ema_kernel):
// after the update, e = e + ema_w * (p_new - e) from the p held in registers, so the average costs one more read and one more write
// per element (5 reads + 4 writes of 4 B) instead of a second pass over all parameters, and it obeys the guard: a step skipped on
// the device leaves e where it was, which the host could not arrange without a synchronisation.  p, m and v come out bit-equal to
// the step the optimizer would have launched without the average, so the kernel carries both arithmetic forms (record field
// `form`): tup_adam_step's (csrc/pack_plan.hip) and adam_guarded_kernel's below.  A segment with g == NULL is a parameter that has
// an average but no gradient in this step (the other scales' upsamplers of a mixed-scale step): its average moves, nothing else.
#include "common.h"

struct NormSeg {
    const float* g;
    long long n;
};
static_assert(sizeof(NormSeg) == 16, "norm segment record = 16 bytes (the host packs it as 2 int64 words)");

struct GuardRec {
    double sumsq, norm;                     // sum of squares of all gradient elements and its square root
    float coef;                             // min(1, max_norm / (norm + 1e-6)) computed in double, then rounded; 1 without a max_norm
    int apply;                              // isfinite(sumsq) || !skip_nonfinite
    float norm_f32;                         // norm rounded to fp32 (what optimizer.grad_norm shows)
    int clipped;                            // this step: apply && coef < 1
    unsigned long long steps, n_applied, n_clipped, n_skipped;      // running counters since the record was zeroed
};
static_assert(sizeof(GuardRec) == 64, "guard record = 64 bytes (the host reads it as 8 int64 words)");

struct AdamWSeg {
    float* p; const float* g; float* m; float* v;
    long long n;
    float step_size, bc2_sqrt, beta2, omb1, omb2, eps;      // step_size = lr / bias_correction1, bc2_sqrt = sqrt(bias_correction2)
    float wd_l2;                            // torch.optim.Adam's weight decay: g += wd_l2 * p (0: none)
    float decay;                            // torch.optim.AdamW's: p *= decay, decay = 1 - lr * weight_decay rounded from double (1: none)
};
static_assert(sizeof(AdamWSeg) == 72, "guarded segment record = 72 bytes (the host packs it as 9 int64 words)");

struct AdamEmaSeg {
    float* p; const float* g; float* m; float* v;          // g == NULL: no gradient in this step, the average alone moves
    long long n;
    float step_size, bc2, beta2, omb1, omb2, eps;           // bc2: form 0: 1 / sqrt(bias_correction2) (AdamSeg), form 1: its sqrt (AdamWSeg)
    float wd_l2, decay;                                     // form 1 only, as in AdamWSeg
    float* e;                                               // the average, updated in place
    float ema_w;                                            // 1 - decay of this update, rounded from double on the host
    int form;                                               // 0: tup_adam_step's arithmetic, 1: tup_adam_step_guarded's
};
static_assert(sizeof(AdamEmaSeg) == 88, "EMA segment record = 88 bytes (the host packs it as 11 int64 words)");

namespace {
constexpr int GUARD_CHUNK = 4096;

// sum of the 256 lanes' values in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double block_sum_256(double x, double* lds)
{
    lds[threadIdx.x] = x;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    return lds[0];
}

__device__ __forceinline__ double sq(float g) { const double d = (double)g; return d * d; }

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const NormSeg* __restrict__ segs, const int* __restrict__ chunks,
                                                         double* __restrict__ partials)
{
    __shared__ double lds[256];
    const int seg = chunks[2 * blockIdx.x], first = chunks[2 * blockIdx.x + 1];
    const NormSeg s = segs[seg];
    const float* __restrict__ g = s.g;
    const long long end = min((long long)first + GUARD_CHUNK, s.n);          // first >= n: an empty chunk, partial 0
    double acc = 0.0;
    long long i = first;
    // `first` is a multiple of 4096, so the chunk start is 16-byte aligned when the segment base is
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && end > first) {
        const long long nvec = (end - first) >> 2;
        for (long long v = threadIdx.x; v < nvec; v += 256) {
            const float4 x = *reinterpret_cast<const float4*>(g + first + 4 * v);
            acc += sq(x.x); acc += sq(x.y); acc += sq(x.z); acc += sq(x.w);
        }
        i = first + 4 * nvec;          // scalar tail: at most 3 elements
    }
    for (i += threadIdx.x; i < end; i += 256) acc += sq(g[i]);
    const double total = block_sum_256(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void guard_finish_kernel(const double* __restrict__ partials, int npartials, double max_norm,
                                                           int skip_nonfinite, GuardRec* __restrict__ rec)
{
    __shared__ double lds[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartials; i += 256) acc += partials[i];
    const double sumsq = block_sum_256(acc, lds);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sumsq);
    double coef = 1.0;
    if (max_norm >= 0.0) {                  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1); a NaN stays
        coef = max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    const bool finite = (sumsq - sumsq) == 0.0;          // false for inf and NaN
    const int apply = (finite || !skip_nonfinite) ? 1 : 0;
    const float coef32 = (float)coef;
    const int clipped = (apply && coef32 < 1.f) ? 1 : 0;
    rec->sumsq = sumsq; rec->norm = norm;
    rec->coef = coef32; rec->apply = apply; rec->norm_f32 = (float)norm; rec->clipped = clipped;
    rec->steps += 1ull; rec->n_applied += (unsigned long long)apply; rec->n_clipped += (unsigned long long)clipped;
    rec->n_skipped += (unsigned long long)(1 - apply);
}

// The update in the operation order of torch's multi-tensor step (torch/optim/adam.py _multi_tensor_adam), whose every line is one
// launch: one rounding where each of torch's launches ends (contraction is off in the loop), and a fused multiply-add, written
// out, where one of its functors feeds a product into an add.
//   g  = g + wd * p                                 (_foreach_add(grads, params, alpha = weight_decay), Adam)
//   p  = p * (1 - lr * wd)                          (_foreach_mul_(params, 1 - lr * weight_decay), AdamW)
//   m  = m + (1 - beta1) * (g - m)                  (_foreach_lerp_)
//   v  = v * beta2;  v = v + (1 - beta2) * (g * g)  (_foreach_mul_, _foreach_addcmul_)
//   d  = sqrt(v);  d = d / sqrt(bias_correction2);  d = d + eps
//   p  = p + (-step_size) * (m / d)                 (_foreach_addcdiv_)
template <bool GUARDED>
__global__ __launch_bounds__(256) void adam_guarded_kernel(const AdamWSeg* __restrict__ segs, const int* __restrict__ chunks,
                                                           const GuardRec* __restrict__ guard)
{
    float coef = 1.f;
    if constexpr (GUARDED) {
        if (guard->apply == 0) return;      // uniform: the whole grid leaves p, m and v as they are
        coef = guard->coef;
    }
    const int seg = chunks[2 * blockIdx.x], first = chunks[2 * blockIdx.x + 1];
    const AdamWSeg s = segs[seg];
    const long long end = min((long long)first + GUARD_CHUNK, s.n);
    const float omb1 = s.omb1, omb2 = s.omb2, beta2 = s.beta2, wd = s.wd_l2, decay = s.decay, neg_step = -s.step_size;
    const bool l2 = wd != 0.f, scale = coef != 1.f;
    for (long long i = first + threadIdx.x; i < end; i += 256) {
#pragma clang fp contract(off)
        float g = s.g[i], p = s.p[i];
        float m = s.m[i], v = s.v[i];
        if (scale) g = g * coef;
        if (l2) g = fmaf(wd, p, g);
        p = p * decay;
        m = fmaf(omb1, g - m, m);
        v = v * beta2;
        v = fmaf(omb2, g * g, v);
        float d = sqrtf(v);
        d = d / s.bc2_sqrt;
        d = d + s.eps;
        s.m[i] = m; s.v[i] = v;
        s.p[i] = fmaf(neg_step, m / d, p);
    }
}

// e = e + w * (p - e) in three separately rounded operations, so that sub / mul / add in torch reproduce it bit for bit
__device__ __forceinline__ float ema_update(float e, float p, float w)
{
#pragma clang fp contract(off)
    float d = p - e;
    d = d * w;
    return e + d;
}

// adam_step_kernel (form 0) or adam_guarded_kernel (form 1) followed by the average's update on the new p.  Form 0 spells out what
// the compiler makes of adam_step_kernel's expressions (checked in its ISA): m and the denominator and p are fused multiply-adds, v
// is two rounded products and their sum.
template <bool GUARDED>
__global__ __launch_bounds__(256) void adam_ema_kernel(const AdamEmaSeg* __restrict__ segs, const int* __restrict__ chunks,
                                                       const GuardRec* __restrict__ guard)
{
    float coef = 1.f;
    if constexpr (GUARDED) {
        if (guard->apply == 0) return;      // uniform: the whole grid leaves p, m, v and e as they are
        coef = guard->coef;
    }
    const int seg = chunks[2 * blockIdx.x], first = chunks[2 * blockIdx.x + 1];
    const AdamEmaSeg s = segs[seg];
    const long long end = min((long long)first + GUARD_CHUNK, s.n);
    const float w = s.ema_w;
    if (s.g == nullptr) {                   // uniform per workgroup: p is read, never written; m and v are not touched
        for (long long i = first + threadIdx.x; i < end; i += 256) s.e[i] = ema_update(s.e[i], s.p[i], w);
        return;
    }
    const float omb1 = s.omb1, omb2 = s.omb2, beta2 = s.beta2, neg_step = -s.step_size;
    if (s.form == 0) {
        for (long long i = first + threadIdx.x; i < end; i += 256) {
#pragma clang fp contract(off)
            const float g = s.g[i];
            float m = s.m[i], v = s.v[i];
            m = fmaf(g - m, omb1, m);
            const float gg = g * g * omb2;
            v = v * beta2 + gg;
            const float denom = fmaf(sqrtf(v), s.bc2, s.eps);
            s.m[i] = m; s.v[i] = v;
            const float p = fmaf(neg_step, m / denom, s.p[i]);
            s.p[i] = p;
            s.e[i] = ema_update(s.e[i], p, w);
        }
        return;
    }
    const float wd = s.wd_l2, decay = s.decay;
    const bool l2 = wd != 0.f, scale = coef != 1.f;
    for (long long i = first + threadIdx.x; i < end; i += 256) {
#pragma clang fp contract(off)
        float g = s.g[i], p = s.p[i];
        float m = s.m[i], v = s.v[i];
        if (scale) g = g * coef;
        if (l2) g = fmaf(wd, p, g);
        p = p * decay;
        m = fmaf(omb1, g - m, m);
        v = v * beta2;
        v = fmaf(omb2, g * g, v);
        float d = sqrtf(v);
        d = d / s.bc2;
        d = d + s.eps;
        s.m[i] = m; s.v[i] = v;
        p = fmaf(neg_step, m / d, p);
        s.p[i] = p;
        s.e[i] = ema_update(s.e[i], p, w);
    }
}
}  // namespace

// segs: device array [nseg] of 16-byte records {const float* g; long long n}; chunks: device int [nchunks][2] = (segment index, first
// element), one workgroup per 4096 elements; partials: device double [nchunks], written (one per workgroup).
extern "C" int tup_grad_sumsq_partial(const void* segs, const int* chunks, int nchunks, double* partials, void* stream)
{
    if (nchunks <= 0) return 0;
    grad_sumsq_kernel<<<dim3((unsigned)nchunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>((const NormSeg*)segs, chunks, partials);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Sums partials[0 .. npartials) in a fixed order (npartials == 0: sum 0) and writes the 64-byte guard record; max_norm < 0: no
// clipping (coef = 1).  The record's four running counters are read, incremented and written back: zero the record once.
extern "C" int tup_grad_guard_finish(const double* partials, int npartials, double max_norm, int skip_nonfinite, void* guard, void* stream)
{
    if (npartials < 0 || guard == nullptr) return (int)hipErrorInvalidValue;
    guard_finish_kernel<<<dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(partials, npartials, max_norm, skip_nonfinite,
                                                                                         (GuardRec*)guard);
    TUP_CHECK_LAUNCH();
    return 0;
}

// segs: device array [nseg] of 72-byte records (AdamWSeg above); chunks as for tup_adam_step; guard: the record
// tup_grad_guard_finish wrote on the same stream, or NULL (always apply, coef = 1: weight decay without a guard).
extern "C" int tup_adam_step_guarded(const void* segs, const int* chunks, int nchunks, const void* guard, void* stream)
{
    if (nchunks <= 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (guard != nullptr)
        adam_guarded_kernel<true><<<dim3((unsigned)nchunks), dim3(256), 0, s>>>((const AdamWSeg*)segs, chunks, (const GuardRec*)guard);
    else
        adam_guarded_kernel<false><<<dim3((unsigned)nchunks), dim3(256), 0, s>>>((const AdamWSeg*)segs, chunks, nullptr);
    TUP_CHECK_LAUNCH();
    return 0;
}

// segs: device array [nseg] of 88-byte records (AdamEmaSeg above); chunks as for tup_adam_step; guard: the record
// tup_grad_guard_finish wrote on the same stream, or NULL (always apply, coef = 1).  Segments with g == NULL update e alone.
extern "C" int tup_adam_step_ema(const void* segs, const int* chunks, int nchunks, const void* guard, void* stream)
{
    if (nchunks <= 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (guard != nullptr)
        adam_ema_kernel<true><<<dim3((unsigned)nchunks), dim3(256), 0, s>>>((const AdamEmaSeg*)segs, chunks, (const GuardRec*)guard);
    else
        adam_ema_kernel<false><<<dim3((unsigned)nchunks), dim3(256), 0, s>>>((const AdamEmaSeg*)segs, chunks, nullptr);
    TUP_CHECK_LAUNCH();
    return 0;
}
