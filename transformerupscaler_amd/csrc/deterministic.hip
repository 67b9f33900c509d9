// Ordered slab reduce of the deterministic weight-gradient forms (gfx950).
//
// The weight-gradient kernels sum over workgroups with float atomics, whose result depends on the order the adds arrive in.
// Their deterministic forms (the *_det entries) instead give every static work item (an M slice, a persistent workgroup) its
// own slice of a caller-provided fp32 slab, written with plain stores, and this kernel adds the slices up in a fixed order:
//     group y = slab[y][i] + slab[y + 4][i] + slab[y + 8][i] + ...   (left to right, y = 0..3)
//     out[i] (= or, accumulating, out[i] +) ((group 0 + group 2) + (group 1 + group 3))
// The grouping depends on nslab only, so the result is the same bits on every run.
#include "common.h"

namespace {

// 64 columns (VEC floats each) x 4 slice groups per workgroup; group y adds slices y, y + 4, ... in order, then the four group
// sums are combined through LDS in a fixed tree (the form of dbias_sum_kernel)
template <int VEC>
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab, long long ld, int nslab,
                                                          float* __restrict__ out, long long n, int accumulate)
{
    typedef __attribute__((ext_vector_type(VEC))) float fv;
    __shared__ fv red[4][64];
    const long long col = (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    const int grp = threadIdx.x >> 6;
    const bool ok = col * VEC < n;
    fv acc = {};
    if (ok) {
        const float* base = slab + col * VEC;
        int s = grp;
        // four slices in flight per step, added in slice order
        for (; s + 12 < nslab; s += 16) {
            fv v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const fv*>(base + (size_t)(s + 4 * u) * ld);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += v[u];
        }
        for (; s < nslab; s += 4) acc += *reinterpret_cast<const fv*>(base + (size_t)s * ld);
    }
    red[grp][threadIdx.x & 63] = acc;
    __syncthreads();
    if (grp == 0 && ok) {
        const int t = threadIdx.x;
        fv r = (red[0][t] + red[2][t]) + (red[1][t] + red[3][t]);
        fv* o = reinterpret_cast<fv*>(out + col * VEC);
        if (accumulate) r = *o + r;
        *o = r;
    }
}

}  // namespace

// out[i] (accumulate ? += : =) the sum over s < nslab of slab[s * ld + i], i < n, in a fixed order that depends on nslab only.
extern "C" int tup_slab_reduce(const float* slab, long long ld, int nslab, float* out, long long n, int accumulate, void* stream)
{
    if (n <= 0) return 0;
    if (nslab <= 0 || ld < n || slab == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool vec = n % 4 == 0 && ld % 4 == 0 && ((uintptr_t)slab & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const long long cols = vec ? n / 4 : n;
    const long long blocks = (cols + 63) / 64;
    if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    if (vec) slab_reduce_kernel<4><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(slab, ld, nslab, out, n, accumulate);
    else slab_reduce_kernel<1><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(slab, ld, nslab, out, n, accumulate);
    TUP_CHECK_LAUNCH();
    return 0;
}
