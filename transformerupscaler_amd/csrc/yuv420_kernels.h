// The YUV 4:2:0 frame kernels (a Y plane and a half-resolution plane of (Cb, Cr) pairs, both pitched, <-> fp32 planar RGB) as templates
// on the sample format F, and their host side.  image_io.hip instantiates Nv12Fmt (8-bit bytes), p010.hip P010Fmt (10-bit codes in
// the high bits of a uint16); each owns its format's traits, coefficient tables and extern "C" entries.  DESIGN 3, "NV12 frames".
// Integer arithmetic on the codes throughout, so the result is a definition, not an approximation: chroma sited "left" (sample (j, i)
// at luma column 2i, between luma rows 2j and 2j + 1), upsampled by the [1 3] / [3 1] vertical and [2] / [1 1] horizontal taps
// without intermediate rounding, 16.16 matrix, clamp to the code range; the tensor is code / (2^BITS - 1), the IEEE quotient.  The
// encode quantises with F::quantise, then the integer matrix and the [1 2 1] x [1 1] chroma filter over rows 2j, 2j + 1.
// A lane owns 4 luma columns x 2 luma rows = 2 chroma pairs; consecutive lanes run along a row pair.  ALIGNED (plane pointers, pitches
// and batch strides multiples of 4 bytes, W % 4 == 0, the fp32 side 16-byte aligned): dwords on the sample side (F::load2, load4,
// store4), 16-byte vectors per plane row on the fp32 side; the chroma neighbours (rows j - 1, j + 1, pair i + 1; on the encode column
// x - 1) are plain loads of lines the neighbouring lanes and waves fetch anyway.  Otherwise samples and floats one by one, columns
// past W skipped.  Pitches and strides are in bytes.  The coefficient rows arrive by value: scalar operands.
//
// A format F says what differs and nothing else:
//   sample_t                  uint8_t or uint16_t; a reader takes sample >> SHIFT, a writer stores code << SHIFT
//   BITS, SHIFT               8, 0 or 10, 6.  From BITS follow the table of 2^BITS quotients, the divisor 2^BITS - 1, the chroma centre
//                             2^(BITS-1) and the limited-range Y offset 16 << (BITS - 8)
//   quantise(float) -> int    the code of a tensor value
//   load2(p, c)               ALIGNED: one (Cb, Cr) pair at p -> c[0..1]
//   load4(p, c), store4(p, c) ALIGNED: four consecutive samples at p <-> the codes c[0..3]
//   MATRICES, DEC, ENC        host: the number of matrices and the coefficient tables [matrix][limited, full]
#pragma once
#include "common.h"

namespace {

struct Yuv420Dec { int yoff, cy, rv, bu, gu, gv; };
struct Yuv420Enc { int yadd, ry, gy, by, ur, ug, ub, vr, vg, vb; };        // yadd = (yoff << 16) + 32768

template <class F> TUP_DEVICE int sat_code(int v) { return v < 0 ? 0 : (v > (1 << F::BITS) - 1 ? (1 << F::BITS) - 1 : v); }
// ... for codes that are shifted into a dword next.  The empty asm hides the clamp from instruction selection: left visible,
// clip(v >> n) pairs under an OR become gfx950's v_ashr_pk_u8_i32 followed by a v_or3_b32 of bytes 2 and 3.  Observed on the device
// with that code: bytes 2 and 3 of the packed word came out OR-ed with what the destination register of the v_ashr_pk held before
// (an address half in one row, a byte value, hence right, in the other), as if the instruction wrote its low half only.  Hidden for
// every format, so that no clamp-shift-pack idiom can be matched to a saturating pack instruction.
template <class F> TUP_DEVICE uint32_t sat_packable(int v) { int r = sat_code<F>(v); asm("" : "+v"(r)); return (uint32_t)r; }

template <class F, bool ALIGNED>
__global__ __launch_bounds__(256) void yuv420_to_f32chw_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp,
                                                               long long ybs, int ypitch, long long uvbs, int uvpitch,
                                                               float* __restrict__ dst, int H, int W, Yuv420Dec k)
{
    typedef typename F::sample_t sample_t;
    constexpr int BYTES = (int)sizeof(sample_t), CODES = 1 << F::BITS;
    // code / (2^BITS - 1) as the IEEE quotient, once per workgroup: the 24 results of a lane are then LDS reads instead of 24 divides
    // of ~10 instructions each, which made the kernel as much VALU- as HBM-bound
    __shared__ float unit[CODES];
#pragma unroll
    for (int i = 0; i < CODES / 256; ++i) unit[threadIdx.x + 256 * i] = (float)(threadIdx.x + 256 * i) / (float)(CODES - 1);
    __syncthreads();
    // Workgroups go to the 8 XCDs in turn, and a chroma row is read by three row pairs: numbered as launched, those sit on different
    // XCDs and every L2 fetches the row for itself (counters at 8 x 2160 x 3840, 8-bit: 158 MB fetched for 100 MB).  So XCD x takes the
    // x-th contiguous band of the frame instead (the first nb % 8 bands one workgroup longer).  This takes the part's 8 XCDs and a
    // round-robin that starts at workgroup 0 of the launch for granted: with frames in blockIdx.y and gridDim.x % 8 != 0 the phase
    // shifts by gridDim.x % 8 per frame, so for b > 0 a band may be spread over XCDs again (the counter run above has 8 frames and
    // gridDim.x % 8 == 2 and still fetched the algorithmic 100 MB, so the loss, if any, is small there).  The numbering is a bijection
    // of [0, gridDim.x) for any placement: a wrong guess costs re-fetches, never results.
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7, per = nb >> 3, rem = nb & 7;
    const unsigned wg = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    const unsigned lin = wg * 256u + threadIdx.x, groups = (unsigned)(W + 3) >> 2;              // lanes run along a row pair, then on
    const int j = (int)(lin / groups), q = (int)(lin - (unsigned)j * groups), b = blockIdx.y;
    const int x = 4 * q, h2 = H >> 1, w2 = W >> 1;
    if (j >= h2) return;
    const uint8_t* ys = yp + (long long)b * ybs + (size_t)(2 * j) * ypitch + BYTES * x;
    const uint8_t* uvb = uvp + (long long)b * uvbs;
    const uint8_t* c[3] = {uvb + (size_t)(j > 0 ? j - 1 : 0) * uvpitch, uvb + (size_t)j * uvpitch,
                           uvb + (size_t)(j + 1 < h2 ? j + 1 : h2 - 1) * uvpitch};
    const int i0 = 2 * q;
    int t[3][3][2];                                                         // [chroma row j-1, j, j+1][pair i0, i0+1, i0+2][Cb, Cr]
    if (ALIGNED) {                                                          // W % 4 == 0: pair i0 + 1 exists
        const int in = i0 + 2 < w2 ? i0 + 2 : w2 - 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            F::load4(c[r] + 2 * BYTES * i0, &t[r][0][0]);
            F::load2(c[r] + 2 * BYTES * in, &t[r][2][0]);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int ip = i0 + p < w2 ? i0 + p : w2 - 1;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const sample_t* cr = reinterpret_cast<const sample_t*>(c[r]);
                t[r][p][0] = cr[2 * ip] >> F::SHIFT; t[r][p][1] = cr[2 * ip + 1] >> F::SHIFT;
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
            F::load4(ys + (size_t)r * ypitch, yv);
        } else {
            const sample_t* yr = reinterpret_cast<const sample_t*>(ys + (size_t)r * ypitch);
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[i] = x + i < W ? yr[i] >> F::SHIFT : 0;
        }
        f32x4 o0, o1, o2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = i >> 1;
            const int cb = ((i & 1) ? v[p][0] + v[p + 1][0] : 2 * v[p][0]) - 4 * CODES;  // 8 x (Cb - 2^(BITS-1))
            const int cr = ((i & 1) ? v[p][1] + v[p + 1][1] : 2 * v[p][1]) - 4 * CODES;
            // 24-bit factors, sums below 2^31 (largest 1.46e8 at 10 bits): full-rate multiplies
            const int base = __mul24(k.cy, yv[i] - k.yoff) + 32768;
            o0[i] = unit[sat_code<F>((base + __mul24(k.rv, cr)) >> 16)];
            o1[i] = unit[sat_code<F>((base + __mul24(k.gu, cb) + __mul24(k.gv, cr)) >> 16)];
            o2[i] = unit[sat_code<F>((base + __mul24(k.bu, cb)) >> 16)];
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

template <class F, bool ALIGNED>
__global__ __launch_bounds__(256) void f32chw_to_yuv420_kernel(const float* __restrict__ src, uint8_t* __restrict__ yp,
                                                               uint8_t* __restrict__ uvp, long long ybs, int ypitch, long long uvbs,
                                                               int uvpitch, int H, int W, Yuv420Enc k)
{
    typedef typename F::sample_t sample_t;
    constexpr int BYTES = (int)sizeof(sample_t);
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
            p[r][ch][0] = F::quantise(sr[-left]);
            if (ALIGNED) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(sr);
#pragma unroll
                for (int i = 0; i < 4; ++i) p[r][ch][1 + i] = F::quantise(a[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[r][ch][1 + i] = x + i < W ? F::quantise(sr[i]) : 0;
            }
        }
    uint8_t* yd = yp + (long long)b * ybs + (size_t)(2 * j) * ypitch + BYTES * x;
    uint8_t* ud = uvp + (long long)b * uvbs + (size_t)j * uvpitch + BYTES * x;                  // pair i = x / 2 starts at sample x
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t yv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            yv[i] = sat_packable<F>((__mul24(k.ry, p[r][0][1 + i]) + __mul24(k.gy, p[r][1][1 + i]) + __mul24(k.by, p[r][2][1 + i]) + k.yadd) >> 16);
        if (ALIGNED) {
            F::store4(yd + (size_t)r * ypitch, yv);
        } else {
            sample_t* yr = reinterpret_cast<sample_t*>(yd + (size_t)r * ypitch);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) yr[i] = (sample_t)(yv[i] << F::SHIFT);
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
        const int half = ((1 << (F::BITS - 1)) << 19) + (1 << 18);          // sums below 2^31 (largest 5.4e8 at 10 bits)
        cv[2 * pr] = sat_packable<F>((__mul24(k.ur, f[0]) + __mul24(k.ug, f[1]) + __mul24(k.ub, f[2]) + half) >> 19);
        cv[2 * pr + 1] = sat_packable<F>((__mul24(k.vr, f[0]) + __mul24(k.vg, f[1]) + __mul24(k.vb, f[2]) + half) >> 19);
    }
    if (ALIGNED) {
        F::store4(ud, cv);
    } else {
        sample_t* ur = reinterpret_cast<sample_t*>(ud);
        ur[0] = (sample_t)(cv[0] << F::SHIFT); ur[1] = (sample_t)(cv[1] << F::SHIFT);           // W is even: columns x, x + 1 exist
        if (x + 2 < W) { ur[2] = (sample_t)(cv[2] << F::SHIFT); ur[3] = (sample_t)(cv[3] << F::SHIFT); }
    }
}

// shared argument check of a format's two entries: 0 = launch, -1 = nothing to do, else the error to return.  Pitches and batch
// strides are bytes and, like the plane pointers, multiples of the sample size; a row is sizeof(sample_t) * W bytes; no pointer of a
// non-empty shape may be null.
template <class F>
int yuv420_check(const void* y, const void* uv, const void* f32, long long ybs, int y_pitch, long long uvbs, int uv_pitch, int B, int H,
                 int W, int matrix, int full_range)
{
    constexpr long long BYTES = sizeof(typename F::sample_t);
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    if (!y || !uv || !f32 || B > 65535 || (H & 1) || (W & 1) || y_pitch < BYTES * W || uv_pitch < BYTES * W ||
        (((uintptr_t)y | (uintptr_t)uv | (uintptr_t)ybs | (uintptr_t)uvbs | (uintptr_t)y_pitch | (uintptr_t)uv_pitch) & (BYTES - 1)) ||
        matrix < 0 || matrix >= F::MATRICES || full_range < 0 || full_range > 1 || (long long)(H / 2) * ((W + 3) / 4) > 0x7fffff00ll)
        return (int)hipErrorInvalidValue;
    return 0;
}

// one lane per 4 columns x 2 rows, numbered along a row pair and on to the next: 256 consecutive ones per workgroup, frames in y
dim3 yuv420_grid(int B, int H, int W) { return dim3((unsigned)(((long long)(H / 2) * ((W + 3) / 4) + 255) / 256), B); }

bool yuv420_aligned(const void* y, const void* uv, long long ybs, int y_pitch, long long uvbs, int uv_pitch, const void* f32, int W)
{
    return ((uintptr_t)y | (uintptr_t)uv | (uintptr_t)ybs | (uintptr_t)uvbs | (uintptr_t)y_pitch | (uintptr_t)uv_pitch |
            (uintptr_t)W) % 4 == 0 && (uintptr_t)f32 % 16 == 0;
}

// the body of a format's decode entry: one launch, no allocation, no synchronisation
template <class F>
int yuv420_decode(const void* y, const void* uv, long long ybs, int y_pitch, long long uvbs, int uv_pitch, float* dst, int B, int H, int W,
                  int matrix, int full_range, void* stream)
{
    if (const int e = yuv420_check<F>(y, uv, dst, ybs, y_pitch, uvbs, uv_pitch, B, H, W, matrix, full_range)) return e < 0 ? 0 : e;
    const dim3 grid = yuv420_grid(B, H, W);
    const Yuv420Dec k = F::DEC[matrix][full_range];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (yuv420_aligned(y, uv, ybs, y_pitch, uvbs, uv_pitch, dst, W))
        yuv420_to_f32chw_kernel<F, true><<<grid, dim3(256), 0, st>>>((const uint8_t*)y, (const uint8_t*)uv, ybs, y_pitch, uvbs, uv_pitch,
                                                                     dst, H, W, k);
    else
        yuv420_to_f32chw_kernel<F, false><<<grid, dim3(256), 0, st>>>((const uint8_t*)y, (const uint8_t*)uv, ybs, y_pitch, uvbs, uv_pitch,
                                                                      dst, H, W, k);
    TUP_CHECK_LAUNCH();
    return 0;
}

// ... and of its encode entry; samples between W and the pitch are not written
template <class F>
int yuv420_encode(const float* src, void* y, void* uv, long long ybs, int y_pitch, long long uvbs, int uv_pitch, int B, int H, int W,
                  int matrix, int full_range, void* stream)
{
    if (const int e = yuv420_check<F>(y, uv, src, ybs, y_pitch, uvbs, uv_pitch, B, H, W, matrix, full_range)) return e < 0 ? 0 : e;
    const dim3 grid = yuv420_grid(B, H, W);
    const int* c = F::ENC[matrix][full_range];
    const Yuv420Enc k = {((full_range ? 0 : 16 << (F::BITS - 8)) << 16) + 32768, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (yuv420_aligned(y, uv, ybs, y_pitch, uvbs, uv_pitch, src, W))
        f32chw_to_yuv420_kernel<F, true><<<grid, dim3(256), 0, st>>>(src, (uint8_t*)y, (uint8_t*)uv, ybs, y_pitch, uvbs, uv_pitch, H, W, k);
    else
        f32chw_to_yuv420_kernel<F, false><<<grid, dim3(256), 0, st>>>(src, (uint8_t*)y, (uint8_t*)uv, ybs, y_pitch, uvbs, uv_pitch, H, W, k);
    TUP_CHECK_LAUNCH();
    return 0;
}

}  // namespace
