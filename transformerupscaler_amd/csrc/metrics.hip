// Image-quality metrics for evaluating an upscaler's output against its target (reference inference.py:128-145 and
// ab_test.py:96-124): skimage's structural_similarity with its defaults (7 x 7 uniform window, sample covariance,
// K1 = 0.01, K2 = 0.03, mean over the interior [3:H-3, 3:W-3], channel_axis=-1) and the sum of squared errors behind MSE /
// PSNR, from one pass over an image pair.
//
//   tup_quality_f32_partial     fp32 planar [B][3][H][W] (model outputs, ToTensor targets)
//   tup_quality_u8hwc_partial   uint8 interleaved [B][H][W][3] (decoded frames), integer window moments
//   tup_quality_reduce          per-workgroup partials -> mse / psnr / ssim / per-channel ssim, fp64, fixed order
//
// Geometry: a workgroup owns a strip of SO = 250 columns and SEG = 96 rows of one image.  Its 256 threads hold one input column
// each (the strip plus the window's 3-column halo on either side) and walk down SEG + 6 input rows: every input byte is read
// 256/250 * 102/96 = 1.09 times.  Per row the loaded values go to LDS, each output column sums its 7 neighbours there (the
// horizontal window sums), and the last 7 rows of those sums stay in registers; the vertical sum is recomputed from the 7 rows
// each time (no running sum that adds and subtracts, which drifts).  Measured: 0.46 ms for four 4K fp32 pairs, 1.7 TB/s
// -- not at the HBM roof; neither PF rows of loads in flight, nor a barrier without the vmcnt wait, nor v_rcp moved it.
//
// Determinism: no atomics.  Each workgroup writes its sums to its own slot of the caller's workspace, and the reduce launch adds
// the slots of an image in a fixed order in fp64, so an image's result is bit-identical across runs and independent of the batch.
#include "common.h"

namespace {

constexpr int SW = 256;          // input columns per strip = threads per workgroup
constexpr int SO = SW - 6;       // columns a strip owns: output centres and squared-error pixels
constexpr int SEG = 96;          // rows a workgroup owns
constexpr int PF = 4;            // rows of loads in flight per thread

// Barrier for the per-row LDS hand-off: the LDS writes need lgkmcnt(0) only (__syncthreads() also waits vmcnt(0), for the PF rows
// of loads in flight).
TUP_DEVICE void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// sum K doubles over the workgroup in a fixed order; the result is valid in thread 0
template <int K>
TUP_DEVICE void block_sum(double (&v)[K], double (*red)[K])
{
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// One workgroup = (strip, segment, plane).  Window moments are taken of shifted data x - kx, y - ky with one constant per
// workgroup (its first pixel): E[x^2] - E[x]^2 of unshifted fp32 data loses the variance of flat bright regions to cancellation.
__global__ __launch_bounds__(256) void quality_f32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          double* __restrict__ partial, int H, int W, float c1, float c2)
{
    __shared__ float lx[2][SW], ly[2][SW];
    __shared__ double red[4][2];
    const int t = threadIdx.x;
    const int c0 = blockIdx.x * SO, r0 = blockIdx.y * SEG;
    const bool last_strip = blockIdx.x == gridDim.x - 1, last_seg = blockIdx.y == gridDim.y - 1;
    const size_t plane = blockIdx.z;
    const float* pa = a + plane * H * W + c0;
    const float* pb = b + plane * H * W + c0;
    const int col = c0 + t;
    const bool in = col < W;
    const bool out_col = t >= 3 && t < SW - 3 && col < W - 3;           // an output centre (col >= 3 since t >= 3)
    const bool own_col = in && (t < SO || last_strip);                  // squared errors: every pixel counted by one workgroup
    const int r1 = min(r0 + SEG + 6, H);                                // input rows [r0, r1)
    const int own_r1 = last_seg ? H : r0 + SEG;
    const float kx = pa[(size_t)r0 * W], ky = pb[(size_t)r0 * W];

    float ring[7][5];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int q = 0; q < 5; ++q) ring[k][q] = 0.f;
    double ssim_sum = 0.0, se_sum = 0.0;
    float xq[PF], yq[PF];                                                // rows r .. r + PF - 1
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        const bool ok = in && r0 + p < r1;
        xq[p] = ok ? pa[(size_t)(r0 + p) * W + t] : 0.f;
        yq[p] = ok ? pb[(size_t)(r0 + p) * W + t] : 0.f;
    }

    for (int base = r0; base < r1; base += 7) {
        float ssim_row = 0.f, se_row = 0.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int r = base + k;
            if (r >= r1) break;                                          // uniform over the workgroup
            const int buf = (r - r0) & 1;
            lx[buf][t] = xq[0] - kx;
            ly[buf][t] = yq[0] - ky;
            if (own_col && r < own_r1) {
                const float d = xq[0] - yq[0];
                se_row = fmaf(d, d, se_row);
            }
#pragma unroll
            for (int p = 0; p < PF - 1; ++p) { xq[p] = xq[p + 1]; yq[p] = yq[p + 1]; }
            if (in && r + PF < r1) {                                     // later rows' loads fly while this row is summed
                xq[PF - 1] = pa[(size_t)(r + PF) * W + t];
                yq[PF - 1] = pb[(size_t)(r + PF) * W + t];
            }
            lds_barrier();                                               // two LDS buffers: one barrier per row suffices
            if (out_col) {
                float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const float x = lx[buf][t - 3 + j], y = ly[buf][t - 3 + j];
                    sx += x;
                    sy += y;
                    sxx = fmaf(x, x, sxx);
                    syy = fmaf(y, y, syy);
                    sxy = fmaf(x, y, sxy);
                }
                ring[k][0] = sx; ring[k][1] = sy; ring[k][2] = sxx; ring[k][3] = syy; ring[k][4] = sxy;
                if (r - r0 >= 6) {                                       // window rows r-6 .. r: centre row r-3
                    float s[5];
#pragma unroll
                    for (int q = 0; q < 5; ++q)
                        s[q] = ((ring[0][q] + ring[1][q]) + (ring[2][q] + ring[3][q])) + ((ring[4][q] + ring[5][q]) + ring[6][q]);
                    const float mx = s[0] * (1.f / 49.f), my = s[1] * (1.f / 49.f);      // shifted means
                    const float vx = (s[2] - s[0] * mx) * (1.f / 48.f);                  // sample (co)variances: cov_norm = 49/48
                    const float vy = (s[3] - s[1] * my) * (1.f / 48.f);
                    const float vxy = (s[4] - s[0] * my) * (1.f / 48.f);
                    const float ux = mx + kx, uy = my + ky;
                    const float num = (2.f * ux * uy + c1) * (2.f * vxy + c2);
                    const float den = (ux * ux + uy * uy + c1) * (vx + vy + c2);
                    ssim_row += num * __builtin_amdgcn_rcpf(den);        // v_rcp_f32 (1 ulp) instead of the 10-instruction IEEE divide
                }
            }
        }
        ssim_sum += (double)ssim_row;                                    // <= 7 rows in fp32, then fp64
        se_sum += (double)se_row;
    }
    double v[2] = {ssim_sum, se_sum};
    block_sum<2>(v, red);
    if (t == 0) {
        double* p = partial + (plane * gridDim.y * gridDim.x + blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = v[0];
        p[1] = v[1];
    }
}

// One workgroup = (strip, segment, image), all three channels.  The strip's bytes are loaded coalesced (thread t: bytes t,
// t + 256, t + 512 of the row) and land in LDS de-interleaved as x | y << 16 per pixel and channel, so a 7-wide sum of those words
// is Sum x | Sum y << 16 (49 * 255 < 2^16: no carry).  Sum x^2, y^2, xy are int32, 49 Sum xx - (Sum x)^2 is exact; only the
// final formula is floating point (fp32 from the exact integers: ~3e-7 relative per window, unbiased; an fp64 formula with its
// divide made the kernel VALU-bound).
__global__ __launch_bounds__(256) void quality_u8hwc_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                            double* __restrict__ partial, int H, int W, float c1n, float c2n)
{
    __shared__ uint32_t lv[2][3][SW];
    __shared__ double red[4][6];
    const int t = threadIdx.x;
    const int c0 = blockIdx.x * SO, r0 = blockIdx.y * SEG;
    const bool last_strip = blockIdx.x == gridDim.x - 1, last_seg = blockIdx.y == gridDim.y - 1;
    const size_t img = blockIdx.z;
    const size_t pitch = (size_t)W * 3;
    const uint8_t* pa = a + img * H * pitch + (size_t)c0 * 3;
    const uint8_t* pb = b + img * H * pitch + (size_t)c0 * 3;
    const int col = c0 + t;
    const int nbytes = (min(c0 + SW, W) - c0) * 3;
    const bool out_col = t >= 3 && t < SW - 3 && col < W - 3;
    const bool own_col = col < W && (t < SO || last_strip);
    const int r1 = min(r0 + SEG + 6, H);
    const int own_r1 = last_seg ? H : r0 + SEG;

    uint32_t ring[7][3][4];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) ring[k][c][q] = 0u;
    double ssim_sum[3] = {0.0, 0.0, 0.0};
    uint32_t se[3] = {0u, 0u, 0u};                                       // <= (SEG + 6) * 255^2 per thread and channel
    uint32_t xq[PF][3], yq[PF][3];                                       // rows r .. r + PF - 1
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int j = t + q * SW;
            const bool ok = j < nbytes && r0 + p < r1;
            xq[p][q] = ok ? pa[(size_t)(r0 + p) * pitch + j] : 0u;
            yq[p][q] = ok ? pb[(size_t)(r0 + p) * pitch + j] : 0u;
        }

    for (int base = r0; base < r1; base += 7) {
        float ssim_row[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int r = base + k;
            if (r >= r1) break;
            const int buf = (r - r0) & 1;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int j = t + q * SW;
                if (j < nbytes) lv[buf][j % 3][j / 3] = xq[0][q] | (yq[0][q] << 16);
            }
#pragma unroll
            for (int p = 0; p < PF - 1; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) { xq[p][q] = xq[p + 1][q]; yq[p][q] = yq[p + 1][q]; }
            if (r + PF < r1) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int j = t + q * SW;
                    if (j < nbytes) {
                        xq[PF - 1][q] = pa[(size_t)(r + PF) * pitch + j];
                        yq[PF - 1][q] = pb[(size_t)(r + PF) * pitch + j];
                    }
                }
            }
            lds_barrier();
            if (own_col && r < own_r1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t w = lv[buf][c][t];
                    const int d = (int)(w & 0xffu) - (int)(w >> 16);
                    se[c] += (uint32_t)(d * d);
                }
            }
            if (out_col) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    uint32_t s = 0u, sxx = 0u, syy = 0u, sxy = 0u;
#pragma unroll
                    for (int j = 0; j < 7; ++j) {
                        const uint32_t w = lv[buf][c][t - 3 + j];
                        const uint32_t x = w & 0xffu, y = w >> 16;
                        s += w;
                        sxx += x * x;
                        syy += y * y;
                        sxy += x * y;
                    }
                    ring[k][c][0] = s; ring[k][c][1] = sxx; ring[k][c][2] = syy; ring[k][c][3] = sxy;
                }
                if (r - r0 >= 6) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        uint32_t s[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            s[q] = ring[0][c][q] + ring[1][c][q] + ring[2][c][q] + ring[3][c][q] + ring[4][c][q] + ring[5][c][q] + ring[6][c][q];
                        const int sx = (int)(s[0] & 0xffffu), sy = (int)(s[0] >> 16);
                        const int pxy = sx * sy;                                          // <= 12495^2 < 2^31
                        const int dxx = 49 * (int)s[1] - sx * sx, dyy = 49 * (int)s[2] - sy * sy, dxy = 49 * (int)s[3] - pxy;
                        // S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) with the 1/49^2 and 1/(49*48) factors
                        // cancelled: c1n = C1 * 49^2, c2n = C2 * 49 * 48
                        const float num = (2.f * (float)pxy + c1n) * (2.f * (float)dxy + c2n);
                        const float den = ((float)(sx * sx + sy * sy) + c1n) * ((float)(dxx + dyy) + c2n);
                        ssim_row[c] += num * __builtin_amdgcn_rcpf(den);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) ssim_sum[c] += (double)ssim_row[c];
    }
    double v[6] = {ssim_sum[0], (double)se[0], ssim_sum[1], (double)se[1], ssim_sum[2], (double)se[2]};
    block_sum<6>(v, red);
    if (t == 0) {
        const size_t nparts = (size_t)gridDim.y * gridDim.x, part = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double* p = partial + ((img * 3 + c) * nparts + part) * 2;
            p[0] = v[2 * c];
            p[1] = v[2 * c + 1];
        }
    }
}

// One workgroup per image: wave 2c + k adds slot k of channel c over the partials (lane l: partials l, l + 64, ... in order, then a
// fixed shuffle tree).  A single thread per slot walking ~400 dependent loads took 40 us.
__global__ __launch_bounds__(384) void quality_reduce_kernel(const double* __restrict__ partial, double* __restrict__ out, int B,
                                                             int nparts, double n_interior, double n_pixels, double range2)
{
    __shared__ double s[6];
    const int t = threadIdx.x, img = blockIdx.x, wave = t >> 6, lane = t & 63;
    const double* p = partial + ((size_t)img * 3 + (wave >> 1)) * nparts * 2 + (wave & 1);
    double acc = 0.0;
    for (int i = lane; i < nparts; i += 64) acc += p[(size_t)i * 2];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) s[wave] = acc;
    __syncthreads();
    if (t == 0) {
        const double mse = ((s[1] + s[3]) + s[5]) / n_pixels;
        const double c0 = s[0] / n_interior, c1 = s[2] / n_interior, c2 = s[4] / n_interior;
        out[img] = mse;
        out[B + img] = mse == 0.0 ? __builtin_inf() : 10.0 * log10(range2 / mse);
        out[2 * B + img] = (c0 + c1 + c2) / 3.0;
        out[3 * B + img] = c0;
        out[4 * B + img] = c1;
        out[5 * B + img] = c2;
    }
}

int check_geometry(int B, int H, int W, int nparts, int planes)
{
    if (B <= 0 || H < 7 || W < 7) return (int)hipErrorInvalidValue;
    const int nstrip = (W - 6 + SO - 1) / SO, nseg = (H - 6 + SEG - 1) / SEG;
    if (nparts != nstrip * nseg || planes > 65535 || nseg > 65535) return (int)hipErrorInvalidValue;
    return 0;
}

}  // namespace

extern "C" int tup_quality_f32_partial(const float* a, const float* b, double* partial, int B, int H, int W, int nparts,
                                       float data_range, void* stream)
{
    if (const int e = check_geometry(B, H, W, nparts, B * 3)) return e;
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    dim3 grid((W - 6 + SO - 1) / SO, (H - 6 + SEG - 1) / SEG, B * 3);
    quality_f32_kernel<<<grid, dim3(SW), 0, reinterpret_cast<hipStream_t>(stream)>>>(a, b, partial, H, W, c1, c2);
    TUP_CHECK_LAUNCH();
    return 0;
}

extern "C" int tup_quality_u8hwc_partial(const void* a, const void* b, double* partial, int B, int H, int W, int nparts,
                                         float data_range, void* stream)
{
    if (const int e = check_geometry(B, H, W, nparts, B)) return e;
    const double r = data_range;
    const float c1n = (float)((0.01 * r) * (0.01 * r) * 49.0 * 49.0), c2n = (float)((0.03 * r) * (0.03 * r) * 49.0 * 48.0);
    dim3 grid((W - 6 + SO - 1) / SO, (H - 6 + SEG - 1) / SEG, B);
    quality_u8hwc_kernel<<<grid, dim3(SW), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), partial, H, W, c1n, c2n);
    TUP_CHECK_LAUNCH();
    return 0;
}

extern "C" int tup_quality_reduce(const double* partial, double* out, int B, int H, int W, int nparts, float data_range,
                                  void* stream)
{
    if (const int e = check_geometry(B, H, W, nparts, 0)) return e;
    const double r = data_range;
    quality_reduce_kernel<<<dim3(B), dim3(384), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        partial, out, B, nparts, (double)(H - 6) * (W - 6), 3.0 * H * W, r * r);
    TUP_CHECK_LAUNCH();
    return 0;
}
