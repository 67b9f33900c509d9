// P010 video frames (YUV 4:2:0, 10 bit: what an HEVC Main10 / AV1 10-bit decoder hands over) <-> fp32 planar RGB: the NV12 pair
// of image_io.hip carried to 10 bits ("P010 frames").  A sample is a little-endian uint16 with its 10-bit code in the high
// bits: a reader takes sample >> 6 and ignores the low six bits, a writer stores code << 6.  Integer arithmetic on the codes
// throughout, so the result is a definition: chroma sited "left", upsampled by the [1 3] / [3 1] vertical and [2] / [1 1] horizontal
// taps without intermediate rounding, 16.16 matrix, clip10; the tensor is code / 1023 (the IEEE quotient, never through 8 bits).  The
// encode quantises with q_10 (round to nearest, below), then the integer matrix and the [1 2 1] x [1 1] chroma filter.
// A lane owns 4 luma columns x 2 luma rows = 2 chroma pairs, as for NV12.  ALIGNED (plane pointers, pitches and batch strides
// multiples of 4 bytes, W % 4 == 0, the fp32 side 16-byte aligned): dwords of two samples on the 16-bit side, 16-byte vectors per
// plane row on the fp32 side.  Otherwise samples and floats one by one, columns past W skipped.  Pitches and strides are in bytes.
#include "common.h"

namespace {

struct P010Dec { int yoff, cy, rv, bu, gu, gv; };
struct P010Enc { int yadd, ry, gy, by, ur, ug, ub, vr, vg, vb; };          // yadd = (yoff << 16) + 32768

TUP_DEVICE int sat10(int v) { return v < 0 ? 0 : (v > 1023 ? 1023 : v); }
// ... for codes that are shifted into a dword next: hidden from instruction selection like image_io.hip's sat8_packable, so that
// no clamp-shift-pack idiom can be matched to a saturating pack instruction
TUP_DEVICE uint32_t sat10_packable(int v) { int r = sat10(v); asm("" : "+v"(r)); return (uint32_t)r; }

// q_10: t = x * 1023; NaN -> 0 (fmaxf); clamp; (int)(t + 0.5f).  The clamp sits between the multiply and the add: no fma can form.
TUP_DEVICE int q10(float x) {
    const float t = fminf(fmaxf(x * 1023.0f, 0.0f), 1023.0f);
    return (int)(t + 0.5f);
}

TUP_DEVICE int lo_code(uint32_t w) { return (int)((w & 0xffffu) >> 6); }
TUP_DEVICE int hi_code(uint32_t w) { return (int)(w >> 22); }
TUP_DEVICE uint32_t two_samples(uint32_t a, uint32_t b) { return (a << 6) | (b << 22); }

template <bool ALIGNED>
__global__ __launch_bounds__(256) void p010_to_f32chw_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp,
                                                             long long ybs, int ypitch, long long uvbs, int uvpitch,
                                                             float* __restrict__ dst, int H, int W, P010Dec k)
{
    // code / 1023 as the IEEE quotient, once per workgroup (the NV12 decode's lesson: 24 divides a lane made it VALU-bound)
    __shared__ float unit[1024];
#pragma unroll
    for (int i = 0; i < 4; ++i) unit[threadIdx.x + 256 * i] = (float)(threadIdx.x + 256 * i) / 1023.0f;
    __syncthreads();
    // XCD x takes the x-th contiguous band of the frame, as in nv12_to_f32chw_kernel (a chroma row is read by three row pairs); a
    // bijection of [0, gridDim.x) for any placement
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7, per = nb >> 3, rem = nb & 7;
    const unsigned wg = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    const unsigned lin = wg * 256u + threadIdx.x, groups = (unsigned)(W + 3) >> 2;
    const int j = (int)(lin / groups), q = (int)(lin - (unsigned)j * groups), b = blockIdx.y;
    const int x = 4 * q, h2 = H >> 1, w2 = W >> 1;
    if (j >= h2) return;
    const uint8_t* ys = yp + (long long)b * ybs + (size_t)(2 * j) * ypitch + 2 * x;
    const uint8_t* uvb = uvp + (long long)b * uvbs;
    const uint8_t* c[3] = {uvb + (size_t)(j > 0 ? j - 1 : 0) * uvpitch, uvb + (size_t)j * uvpitch,
                           uvb + (size_t)(j + 1 < h2 ? j + 1 : h2 - 1) * uvpitch};
    const int i0 = 2 * q;
    int t[3][3][2];                                                         // [chroma row j-1, j, j+1][pair i0, i0+1, i0+2][Cb, Cr]
    if (ALIGNED) {                                                          // W % 4 == 0: pair i0 + 1 exists
        const int in = i0 + 2 < w2 ? i0 + 2 : w2 - 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint32_t a0 = *reinterpret_cast<const uint32_t*>(c[r] + 4 * i0);
            const uint32_t a1 = *reinterpret_cast<const uint32_t*>(c[r] + 4 * i0 + 4);
            const uint32_t n = *reinterpret_cast<const uint32_t*>(c[r] + 4 * in);
            t[r][0][0] = lo_code(a0); t[r][0][1] = hi_code(a0);
            t[r][1][0] = lo_code(a1); t[r][1][1] = hi_code(a1);
            t[r][2][0] = lo_code(n); t[r][2][1] = hi_code(n);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int ip = i0 + p < w2 ? i0 + p : w2 - 1;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const uint16_t* cr = reinterpret_cast<const uint16_t*>(c[r]);
                t[r][p][0] = cr[2 * ip] >> 6; t[r][p][1] = cr[2 * ip + 1] >> 6;
            }
        }
    }
    const size_t hw = (size_t)H * W;
    float* d = dst + (size_t)b * 3 * hw + (size_t)(2 * j) * W + x;
#pragma unroll
    for (int r = 0; r < 2; ++r) {                                           // luma rows 2j, 2j + 1
        int v[3][2];                                                        // 4 x chroma at the three pairs
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) v[p][ch] = 3 * t[1][p][ch] + (r ? t[2][p][ch] : t[0][p][ch]);
        int yv[4];
        if (ALIGNED) {
            const uint32_t w0 = *reinterpret_cast<const uint32_t*>(ys + (size_t)r * ypitch);
            const uint32_t w1 = *reinterpret_cast<const uint32_t*>(ys + (size_t)r * ypitch + 4);
            yv[0] = lo_code(w0); yv[1] = hi_code(w0); yv[2] = lo_code(w1); yv[3] = hi_code(w1);
        } else {
            const uint16_t* yr = reinterpret_cast<const uint16_t*>(ys + (size_t)r * ypitch);
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[i] = x + i < W ? yr[i] >> 6 : 0;
        }
        f32x4 o0, o1, o2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = i >> 1;
            const int cb = ((i & 1) ? v[p][0] + v[p + 1][0] : 2 * v[p][0]) - 4096;       // 8 x (Cb - 512)
            const int cr = ((i & 1) ? v[p][1] + v[p + 1][1] : 2 * v[p][1]) - 4096;
            const int base = __mul24(k.cy, yv[i] - k.yoff) + 32768;         // 24-bit factors, sums below 2^31 (largest 1.46e8)
            o0[i] = unit[sat10((base + __mul24(k.rv, cr)) >> 16)];
            o1[i] = unit[sat10((base + __mul24(k.gu, cb) + __mul24(k.gv, cr)) >> 16)];
            o2[i] = unit[sat10((base + __mul24(k.bu, cb)) >> 16)];
        }
        float* dr = d + (size_t)r * W;
        if (ALIGNED) {
            *reinterpret_cast<f32x4*>(dr) = o0;
            *reinterpret_cast<f32x4*>(dr + hw) = o1;
            *reinterpret_cast<f32x4*>(dr + 2 * hw) = o2;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) { dr[i] = o0[i]; dr[hw + i] = o1[i]; dr[2 * hw + i] = o2[i]; }
        }
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void f32chw_to_p010_kernel(const float* __restrict__ src, uint8_t* __restrict__ yp,
                                                             uint8_t* __restrict__ uvp, long long ybs, int ypitch, long long uvbs,
                                                             int uvpitch, int H, int W, P010Enc k)
{
    const unsigned lin = blockIdx.x * 256u + threadIdx.x, groups = (unsigned)(W + 3) >> 2;
    const int j = (int)(lin / groups), b = blockIdx.y;
    const int x = 4 * (int)(lin - (unsigned)j * groups), h2 = H >> 1;
    if (j >= h2) return;
    const size_t hw = (size_t)H * W;
    const float* s = src + (size_t)b * 3 * hw + (size_t)(2 * j) * W + x;
    const int left = x > 0 ? 1 : 0;                                         // column x - 1, clamped to the image
    int p[2][3][5];                                                         // codes of [row][channel][column x - 1 .. x + 3]
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* sr = s + (size_t)ch * hw + (size_t)r * W;
            p[r][ch][0] = q10(sr[-left]);
            if (ALIGNED) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(sr);
#pragma unroll
                for (int i = 0; i < 4; ++i) p[r][ch][1 + i] = q10(a[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[r][ch][1 + i] = x + i < W ? q10(sr[i]) : 0;
            }
        }
    uint8_t* yd = yp + (long long)b * ybs + (size_t)(2 * j) * ypitch + 2 * x;
    uint8_t* ud = uvp + (long long)b * uvbs + (size_t)j * uvpitch + 2 * x;  // pair i = x / 2 starts at sample x
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t yv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            yv[i] = sat10_packable((__mul24(k.ry, p[r][0][1 + i]) + __mul24(k.gy, p[r][1][1 + i]) + __mul24(k.by, p[r][2][1 + i]) + k.yadd) >> 16);
        if (ALIGNED) {
            *reinterpret_cast<uint32_t*>(yd + (size_t)r * ypitch) = two_samples(yv[0], yv[1]);
            *reinterpret_cast<uint32_t*>(yd + (size_t)r * ypitch + 4) = two_samples(yv[2], yv[3]);
        } else {
            uint16_t* yr = reinterpret_cast<uint16_t*>(yd + (size_t)r * ypitch);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) yr[i] = (uint16_t)(yv[i] << 6);
        }
    }
    uint32_t cv[4];                                                         // Cb, Cr of pair x / 2, Cb, Cr of pair x / 2 + 1
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        int f[3];                                                           // 8 x the [1 2 1] x [1 1] filtered channel at column x + 2 pr
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            f[ch] = p[0][ch][2 * pr] + 2 * p[0][ch][2 * pr + 1] + p[0][ch][2 * pr + 2]
                  + p[1][ch][2 * pr] + 2 * p[1][ch][2 * pr + 1] + p[1][ch][2 * pr + 2];
        const int half = (512 << 19) + (1 << 18);                           // sums below 2^31 (largest 5.4e8)
        cv[2 * pr] = sat10_packable((__mul24(k.ur, f[0]) + __mul24(k.ug, f[1]) + __mul24(k.ub, f[2]) + half) >> 19);
        cv[2 * pr + 1] = sat10_packable((__mul24(k.vr, f[0]) + __mul24(k.vg, f[1]) + __mul24(k.vb, f[2]) + half) >> 19);
    }
    if (ALIGNED) {
        *reinterpret_cast<uint32_t*>(ud) = two_samples(cv[0], cv[1]);
        *reinterpret_cast<uint32_t*>(ud + 4) = two_samples(cv[2], cv[3]);
    } else {
        uint16_t* ur = reinterpret_cast<uint16_t*>(ud);
        ur[0] = (uint16_t)(cv[0] << 6); ur[1] = (uint16_t)(cv[1] << 6);     // W is even: columns x, x + 1 exist
        if (x + 2 < W) { ur[2] = (uint16_t)(cv[2] << 6); ur[3] = (uint16_t)(cv[3] << 6); }
    }
}

// [bt601, bt709, bt2020][limited, full], from Kr, Kb as DESIGN 3 derives them (tests/test_p010_cpu.py pins both tables)
constexpr P010Dec P010_DEC[3][2] = {{{64, 76533, 13113, 16574, -3219, -6679}, {0, 65536, 11485, 14516, -2819, -5850}},
                                    {{64, 76533, 14729, 17356, -1752, -4378}, {0, 65536, 12901, 15201, -1535, -3835}},
                                    {{64, 76533, 13792, 17597, -1539, -5344}, {0, 65536, 12080, 15412, -1348, -4681}}};
constexpr int P010_ENC[3][2][9] = {{{16780, 32941, 6398, -9685, -19015, 28700, 28700, -24033, -4667},
                                    {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}},
                                   {{11931, 40136, 4052, -6576, -22124, 28700, 28700, -26068, -2632},
                                    {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}},
                                   {{14742, 38049, 3328, -8015, -20685, 28700, 28700, -26392, -2308},
                                    {17216, 44434, 3886, -9151, -23617, 32768, 32768, -30133, -2635}}};

// shared argument check of the two P010 entries: 0 = launch, -1 = nothing to do, else the error to return.  Pitches and batch
// strides are bytes and must be even (a sample is two bytes), a row is 2 W bytes; no pointer of a non-empty shape may be null.
int p010_check(const void* y, const void* uv, const void* f32, long long ybs, int y_pitch, long long uvbs, int uv_pitch, int B, int H,
               int W, int matrix, int full_range)
{
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    if (!y || !uv || !f32 || B > 65535 || (H & 1) || (W & 1) || W > 0x3fffffff || y_pitch < 2 * W || uv_pitch < 2 * W ||
        (((uintptr_t)y | (uintptr_t)uv | (uintptr_t)ybs | (uintptr_t)uvbs | (uintptr_t)y_pitch | (uintptr_t)uv_pitch) & 1) ||
        matrix < 0 || matrix > 2 || full_range < 0 || full_range > 1 || (long long)(H / 2) * ((W + 3) / 4) > 0x7fffff00ll)
        return (int)hipErrorInvalidValue;
    return 0;
}

// one lane per 4 columns x 2 rows, numbered along a row pair and on to the next: 256 consecutive ones per workgroup, frames in y
dim3 p010_grid(int B, int H, int W) { return dim3((unsigned)(((long long)(H / 2) * ((W + 3) / 4) + 255) / 256), B); }

bool p010_aligned(const void* y, const void* uv, long long ybs, int y_pitch, long long uvbs, int uv_pitch, const void* f32, int W)
{
    return ((uintptr_t)y | (uintptr_t)uv | (uintptr_t)ybs | (uintptr_t)uvbs | (uintptr_t)y_pitch | (uintptr_t)uv_pitch |
            (uintptr_t)W) % 4 == 0 && (uintptr_t)f32 % 16 == 0;
}

}  // namespace

// A P010 surface -> fp32 planar RGB in [0, 1], bit-exact with the integer definition of DESIGN 3 ("P010 frames").  y u16 [B][H][W]
// (row pitch y_pitch, batch stride y_batch_stride, both in bytes and even), uv u16 [B][H/2][W/2][2] = (Cb, Cr) (uv_pitch,
// uv_batch_stride); dst fp32 [B][3][H][W].  One launch, no allocation, no synchronisation: capturable.
extern "C" int tup_p010_to_f32chw(const void* y, const void* uv, long long y_batch_stride, int y_pitch, long long uv_batch_stride,
                                  int uv_pitch, float* dst, int B, int H, int W, int matrix, int full_range, void* stream)
{
    if (const int e = p010_check(y, uv, dst, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, B, H, W, matrix, full_range))
        return e < 0 ? 0 : e;
    const dim3 grid = p010_grid(B, H, W);
    const P010Dec k = P010_DEC[matrix][full_range];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (p010_aligned(y, uv, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, dst, W))
        p010_to_f32chw_kernel<true><<<grid, dim3(256), 0, st>>>((const uint8_t*)y, (const uint8_t*)uv, y_batch_stride, y_pitch,
                                                                uv_batch_stride, uv_pitch, dst, H, W, k);
    else
        p010_to_f32chw_kernel<false><<<grid, dim3(256), 0, st>>>((const uint8_t*)y, (const uint8_t*)uv, y_batch_stride, y_pitch,
                                                                 uv_batch_stride, uv_pitch, dst, H, W, k);
    TUP_CHECK_LAUNCH();
    return 0;
}

// fp32 planar RGB -> a P010 surface: codes q_10(x) (round to nearest, NaN -> 0), then the integer matrix and the [1 2 1] x [1 1]
// chroma filter of DESIGN 3; samples are code << 6.  Same layout arguments; samples between W and the pitch are not written.
extern "C" int tup_f32chw_to_p010(const float* src, void* y, void* uv, long long y_batch_stride, int y_pitch,
                                  long long uv_batch_stride, int uv_pitch, int B, int H, int W, int matrix, int full_range,
                                  void* stream)
{
    if (const int e = p010_check(y, uv, src, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, B, H, W, matrix, full_range))
        return e < 0 ? 0 : e;
    const dim3 grid = p010_grid(B, H, W);
    const int* c = P010_ENC[matrix][full_range];
    const P010Enc k = {((full_range ? 0 : 64) << 16) + 32768, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (p010_aligned(y, uv, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, src, W))
        f32chw_to_p010_kernel<true><<<grid, dim3(256), 0, st>>>(src, (uint8_t*)y, (uint8_t*)uv, y_batch_stride, y_pitch,
                                                                uv_batch_stride, uv_pitch, H, W, k);
    else
        f32chw_to_p010_kernel<false><<<grid, dim3(256), 0, st>>>(src, (uint8_t*)y, (uint8_t*)uv, y_batch_stride, y_pitch,
                                                                 uv_batch_stride, uv_pitch, H, W, k);
    TUP_CHECK_LAUNCH();
    return 0;
}
