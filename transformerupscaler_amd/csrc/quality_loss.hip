// Training loss on the quantities csrc/metrics.hip scores (transformerupscaler_amd/losses.py):
//
//   loss = w_l1 * mean|x - y| + w_mse * mean (x - y)^2 + w_ssim * (1 - mean_b SSIM(x[b], y[b]))
//
// with nn.L1Loss, nn.MSELoss and skimage's default SSIM (7 x 7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, interior
// mean, mean over the 3 channels) of fp32 planar [B][3][H][W] pairs.
//
//   tup_quality_loss_reduce     the partials of tup_quality_f32_partial (+ those of tup_l1_loss_partial) -> the scalar loss
//   tup_quality_loss_f32_bwd    grad = g * d loss / d x, one streaming pass
//
// Forward: the SSIM and squared-error sums are the scorer's own kernel (one definition for the metric and the loss); the reduce adds
// each image's slots exactly as tup_quality_reduce does, then the images in index order, in fp64.
//
// Backward, SSIM term.  With n = 49, k = 49/48, window moments ux, uy, vx, vy, vxy and
//   A1 = 2 ux uy + C1, A2 = 2 vxy + C2, B1 = ux^2 + uy^2 + C1, B2 = vx + vy + C2, D = B1 B2, S = A1 A2 / D
// a window w gives every pixel p it covers
//   dS_w / dx_p = (2/n) [ T_w + k (A1/D) (y_p - uy) - k (S/B2) (x_p - ux) ],   T_w = uy A2/D - ux S/B1
//                                                                                  = A2 (uy - ux) (uy (ux + uy) + C1) / (D B1)
// (the factored T_w has no cancellation left but uy - ux itself).  Every moment is taken of data shifted by one constant per
// workgroup (kx, ky: its first pixel), as the forward does, and the affine form is evaluated around the same shift:
//   dS_w / dx_p = a_w + b_w (x_p - kx) + c_w (y_p - ky),  c_w = (2k/n) A1/D,  b_w = -(2k/n) S/B2,
//   a_w = (2/n) T_w - c_w (uy - ky) - b_w (ux - kx)
// so a pixel's gradient is  -(w_ssim / (3 B Nwin)) * [ Sum a + (x_p - kx) Sum b + (y_p - ky) Sum c ]  over the <= 49 interior windows
// that cover it: a 7 x 7 box sum of the moments followed by a 7 x 7 box sum of three coefficient maps that are zero outside
// [0, H-6) x [0, W-6).
//
// Geometry: both box sums in ONE streaming kernel (no coefficient planes through HBM, which would be +6 plane passes).  A workgroup
// owns SO = 244 columns and SEG = 96 rows of one plane's gradient; its 256 threads hold one input column each (the strip plus a
// 6-column halo on either side: 3 for the window, 3 more for the windows that cover a pixel) and walk down SEG + 12 input rows, so
// x and y are read 256/244 * 108/96 = 1.18 times and grad is written once.  Thread t is input column c0 - 6 + t, the window whose
// LEFT column that is, and the gradient pixel of that column.  Per row: values -> LDS, 7-wide moment sums, the last 7 rows of them
// in registers; once 7 rows are in, the coefficients of the window row that just completed -> LDS, 7-wide sums of those, the last 7
// rows of them in registers; the gradient row that just completed is written.  The vertical sums are recomputed from their 7 rows
// each time (no running add-and-subtract).
//
// Determinism: no atomics, no cross-workgroup sums; a pixel's gradient depends on its own plane only.
#include "common.h"

namespace {

constexpr int SW = 256;          // input columns per strip = threads per workgroup
constexpr int HALO = 6;
constexpr int SO = SW - 2 * HALO;        // gradient columns a strip owns
constexpr int SEG = 96;          // gradient rows a workgroup owns
constexpr int PF = 4;            // rows of loads in flight per thread

// Barrier for the per-row LDS hand-offs: they need lgkmcnt(0) only (__syncthreads() also waits vmcnt(0), for the PF rows of loads in
// flight and the gradient stores).
TUP_DEVICE void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

TUP_DEVICE float sum7(const float (&r)[7][5], int q) { return ((r[0][q] + r[1][q]) + (r[2][q] + r[3][q])) + ((r[4][q] + r[5][q]) + r[6][q]); }
TUP_DEVICE float sum7c(const float (&r)[7][3], int q) { return ((r[0][q] + r[1][q]) + (r[2][q] + r[3][q])) + ((r[4][q] + r[5][q]) + r[6][q]); }

// s_l1 = w_l1 / N, s_mse = 2 w_mse / N, s_ssim = -w_ssim / (3 B Nwin); all multiplied by the upstream scalar g[0] here.
// Held to 4 waves per SIMD (124 VGPRs, no scratch): left alone the compiler takes 132 VGPRs and 3 waves, measured 6 % slower
// (200 -> 188 us at 4 x 3 x 1080 x 1920, same bits).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
void quality_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                             float* __restrict__ grad, int H, int W, float c1, float c2, float s_l1, float s_mse, float s_ssim)
{
    __shared__ float lx[SW], ly[SW];
    __shared__ float lc[3][SW];
    const int t = threadIdx.x;
    const int c0 = blockIdx.x * SO, r0 = blockIdx.y * SEG;
    const size_t plane = blockIdx.z;
    const float* px = x + plane * H * W;
    const float* py = y + plane * H * W;
    float* pg = grad + plane * H * W;
    const int col = c0 - HALO + t;
    const bool in = col >= 0 && col < W;
    const bool win_col = t < SW - 6 && col >= 0 && col < W - 6;          // window columns [col, col + 6] = threads t .. t + 6
    const bool out_col = t >= HALO && t < HALO + SO && col < W;          // (col >= 0 since t >= HALO)
    const size_t k0 = (size_t)max(r0 - 2 * HALO, 0) * W + max(c0 - HALO, 0);
    const float kx = px[k0], ky = py[k0], dk = ky - kx;
    const float gs = g[0];
    const float g_l1 = gs * s_l1, g_mse = gs * s_mse, g_ssim = gs * s_ssim;
    const int rows = min(SEG, H - r0);                                   // gradient rows [r0, r0 + rows)
    const int steps = rows + 2 * HALO;                                   // step i: input row r0 - 6 + i, window / gradient row r0 - 12 + i
    const int rin0 = r0 - HALO;

    float ring[7][5], cring[7][3], xr[7], yr[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int q = 0; q < 5; ++q) ring[k][q] = 0.f;
#pragma unroll
        for (int q = 0; q < 3; ++q) cring[k][q] = 0.f;
        xr[k] = 0.f;
        yr[k] = 0.f;
    }
    float xq[PF], yq[PF];                                                // input rows of steps i .. i + PF - 1
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        const int r = rin0 + p;
        const bool ok = in && r >= 0 && r < H;
        xq[p] = ok ? px[(size_t)r * W + col] : 0.f;
        yq[p] = ok ? py[(size_t)r * W + col] : 0.f;
    }

    for (int base = 0; base < steps; base += 7) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int i = base + k;
            if (i >= steps) break;                                       // uniform over the workgroup
            const int r = rin0 + i, q = r - HALO;                        // input row; top row of the window it completes = gradient row
            xr[k] = xq[0];
            yr[k] = yq[0];
            lx[t] = xq[0] - kx;
            ly[t] = yq[0] - ky;
#pragma unroll
            for (int p = 0; p < PF - 1; ++p) { xq[p] = xq[p + 1]; yq[p] = yq[p + 1]; }
            {
                const int rn = r + PF;
                const bool ok = in && rn >= 0 && rn < H;
                xq[PF - 1] = ok ? px[(size_t)rn * W + col] : 0.f;        // later rows' loads fly while this row is summed
                yq[PF - 1] = ok ? py[(size_t)rn * W + col] : 0.f;
            }
            lds_barrier();
            float ca = 0.f, cb = 0.f, cc = 0.f;
            if (win_col) {
                float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const float xv = lx[t + j], yv = ly[t + j];
                    sx += xv;
                    sy += yv;
                    sxx = fmaf(xv, xv, sxx);
                    syy = fmaf(yv, yv, syy);
                    sxy = fmaf(xv, yv, sxy);
                }
                ring[k][0] = sx; ring[k][1] = sy; ring[k][2] = sxx; ring[k][3] = syy; ring[k][4] = sxy;
                if (i >= 6 && q >= 0 && r < H) {                         // window rows q .. q + 6 = r, all walked and inside the image
                    const float s0 = sum7(ring, 0), s1 = sum7(ring, 1), s2 = sum7(ring, 2), s3 = sum7(ring, 3), s4 = sum7(ring, 4);
                    const float mx = s0 * (1.f / 49.f), my = s1 * (1.f / 49.f);          // shifted means
                    const float vx = (s2 - s0 * mx) * (1.f / 48.f);                      // sample (co)variances: cov_norm = 49/48
                    const float vy = (s3 - s1 * my) * (1.f / 48.f);
                    const float vxy = (s4 - s0 * my) * (1.f / 48.f);
                    const float ux = mx + kx, uy = my + ky;
                    const float a1 = 2.f * ux * uy + c1, a2 = 2.f * vxy + c2;
                    const float b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
                    const float rb1 = __builtin_amdgcn_rcpf(b1), rb2 = __builtin_amdgcn_rcpf(b2);
                    const float rd = rb1 * rb2;
                    const float a1d = a1 * rd;                                           // A1 / D
                    const float tw = a2 * ((my - mx) + dk) * fmaf(uy, ux + uy, c1) * (rd * rb1);
                    cc = (2.f / 48.f) * a1d;                                             // (2 k / n) A1 / D
                    cb = -(2.f / 48.f) * (a1d * a2) * rb2;                               // -(2 k / n) S / B2
                    ca = fmaf(2.f / 49.f, tw, -fmaf(cc, my, cb * mx));
                }
            }
            lc[0][t] = ca;
            lc[1][t] = cb;
            lc[2][t] = cc;
            lds_barrier();
            if (out_col) {
                float ha = 0.f, hb = 0.f, hc = 0.f;
#pragma unroll
                for (int j = 0; j < 7; ++j) {                            // the windows whose left column is col - 6 .. col
                    ha += lc[0][t - 6 + j];
                    hb += lc[1][t - 6 + j];
                    hc += lc[2][t - 6 + j];
                }
                cring[k][0] = ha; cring[k][1] = hb; cring[k][2] = hc;
                if (i >= 2 * HALO) {                                     // gradient row q in [r0, r0 + rows): window rows q - 6 .. q
                    const float xp = xr[(k + 1) % 7], yp = yr[(k + 1) % 7];              // row q: loaded 6 steps ago
                    const float sa = sum7c(cring, 0), sb = sum7c(cring, 1), sc = sum7c(cring, 2);
                    const float ds = fmaf(sc, yp - ky, fmaf(sb, xp - kx, sa));
                    const float d = xp - yp;
                    const float sg = d > 0.f ? g_l1 : (d < 0.f ? -g_l1 : 0.f);
                    pg[(size_t)q * W + col] = fmaf(g_ssim, ds, fmaf(g_mse, d, sg));
                }
            }
        }
    }
}

// The loss without its SSIM term: one pass, nothing shared between pixels.
__global__ __launch_bounds__(256) void pointwise_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const float* __restrict__ g, float* __restrict__ grad, size_t n4,
                                                                 size_t n, float s_l1, float s_mse)
{
    const float g_l1 = g[0] * s_l1, g_mse = g[0] * s_mse;
    if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) {                                                                   // n % 4 tail
        const float d = x[n4 * 4 + threadIdx.x] - y[n4 * 4 + threadIdx.x];
        grad[n4 * 4 + threadIdx.x] = fmaf(g_mse, d, d > 0.f ? g_l1 : (d < 0.f ? -g_l1 : 0.f));
    }
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 a = reinterpret_cast<const f32x4*>(x)[i], b = reinterpret_cast<const f32x4*>(y)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = a[e] - b[e];
            o[e] = fmaf(g_mse, d, d > 0.f ? g_l1 : (d < 0.f ? -g_l1 : 0.f));
        }
        reinterpret_cast<f32x4*>(grad)[i] = o;
    }
}

// One workgroup.  Per image, wave 2c + k adds slot k of channel c over the partials exactly as quality_reduce_kernel does (lane l:
// partials l, l + 64, ... in order, then a fixed shuffle tree), so the per-image SSIM and MSE are the scorer's bits; thread 0 adds
// the images in index order.  The L1 partials (fp32 per workgroup of tup_l1_loss_partial) are added in fp64: thread t takes
// t, t + 384, ..., then waves and lanes in a fixed order.
__global__ __launch_bounds__(384) void quality_loss_reduce_kernel(const double* __restrict__ qpartial, const float* __restrict__ l1partial,
                                                                  float* __restrict__ out, int B, int nparts, int nl1,
                                                                  double n_interior, double n_pixels, double w_l1, double w_mse,
                                                                  double w_ssim)
{
    __shared__ double s[6];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double mse_sum = 0.0, ssim_sum = 0.0, l1_sum = 0.0;
    if (qpartial != nullptr) {
        for (int img = 0; img < B; ++img) {
            const double* p = qpartial + ((size_t)img * 3 + (wave >> 1)) * nparts * 2 + (wave & 1);
            double acc = 0.0;
            for (int i = lane; i < nparts; i += 64) acc += p[(size_t)i * 2];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) s[wave] = acc;
            __syncthreads();
            if (t == 0) {
                mse_sum += ((s[1] + s[3]) + s[5]) / n_pixels;
                const double k0 = s[0] / n_interior, k1 = s[2] / n_interior, k2 = s[4] / n_interior;
                ssim_sum += (k0 + k1 + k2) / 3.0;
            }
            __syncthreads();
        }
    }
    if (l1partial != nullptr) {
        double acc = 0.0;
        for (int i = t; i < nl1; i += 384) acc += (double)l1partial[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) s[wave] = acc;
        __syncthreads();
        if (t == 0) l1_sum = ((s[0] + s[1]) + (s[2] + s[3])) + (s[4] + s[5]);
    }
    if (t == 0) {
        double loss = 0.0;
        if (w_l1 != 0.0) loss += w_l1 * (l1_sum / (n_pixels * B));
        if (w_mse != 0.0) loss += w_mse * (mse_sum / B);
        if (w_ssim != 0.0) loss += w_ssim * (1.0 - ssim_sum / B);
        out[0] = (float)loss;
    }
}

}  // namespace

extern "C" int tup_quality_loss_reduce(const double* qpartial, const float* l1partial, float* out, int B, int H, int W, int nparts,
                                       int nl1, float w_l1, float w_mse, float w_ssim, void* stream)
{
    if (B <= 0 || H < 7 || W < 7 || nparts < 0 || nl1 < 0) return (int)hipErrorInvalidValue;
    if ((w_mse != 0.f || w_ssim != 0.f) && (qpartial == nullptr || nparts < 1)) return (int)hipErrorInvalidValue;
    if (w_l1 != 0.f && (l1partial == nullptr || nl1 < 1)) return (int)hipErrorInvalidValue;
    quality_loss_reduce_kernel<<<dim3(1), dim3(384), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (w_mse != 0.f || w_ssim != 0.f) ? qpartial : nullptr, w_l1 != 0.f ? l1partial : nullptr, out, B, nparts, nl1,
        (double)(H - 6) * (W - 6), 3.0 * H * W, (double)w_l1, (double)w_mse, (double)w_ssim);
    TUP_CHECK_LAUNCH();
    return 0;
}

extern "C" int tup_quality_loss_f32_bwd(const float* x, const float* y, const float* gscalar, float* grad, int B, int H, int W,
                                        float w_l1, float w_mse, float w_ssim, float data_range, void* stream)
{
    if (B <= 0 || H < 7 || W < 7) return (int)hipErrorInvalidValue;
    const double n = 3.0 * B * H * W;
    const float s_l1 = (float)((double)w_l1 / n), s_mse = (float)(2.0 * (double)w_mse / n);
    if (w_ssim == 0.f) {
        const size_t total = (size_t)B * 3 * H * W;
        size_t blocks = (total / 4 + 255) / 256;
        blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
        pointwise_loss_bwd_kernel<<<dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
            x, y, gscalar, grad, total / 4, total, s_l1, s_mse);
        TUP_CHECK_LAUNCH();
        return 0;
    }
    const int nstrip = (W + SO - 1) / SO, nseg = (H + SEG - 1) / SEG;
    if (B * 3 > 65535 || nseg > 65535) return (int)hipErrorInvalidValue;
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    const float s_ssim = (float)(-(double)w_ssim / (3.0 * B * (double)(H - 6) * (double)(W - 6)));
    quality_loss_bwd_kernel<<<dim3(nstrip, nseg, B * 3), dim3(SW), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        x, y, gscalar, grad, H, W, c1, c2, s_l1, s_mse, s_ssim);
    TUP_CHECK_LAUNCH();
    return 0;
}
