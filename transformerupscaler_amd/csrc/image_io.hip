// Frame pre/post-processing either side of the model, HBM-bound byte work:
//   u8 HWC (RGB or BGR) -> fp32 planar CHW / 255      torchvision ToTensor on a uint8 image
//                                                     (reference data_handling/data_class.py:61-71, inference.py:65-75)
//   fp32 planar CHW -> u8 HWC (RGB or BGR)            (x * 255).clamp(0, 255).to(uint8).permute(1, 2, 0)[..., [2, 1, 0]]
//                                                     (reference app_overlay.py:381-388; ToPILImage's mul(255).byte(),
//                                                     inference.py:123-124)
//   NV12 (Y plane + plane of Cb/Cr pairs, pitched) <-> fp32 planar CHW      what a video decoder hands over and an encoder
//                                                     takes; integer definition in DESIGN 3, no counterpart in the reference
// Each lane handles 4 consecutive pixels: three 4-byte words on the interleaved side, one 16-byte vector per plane
// on the planar side, so both sides move whole dwords.  Results are bit-exact with the torch expressions
// (IEEE fp32 divide / multiply, truncating float -> u8 conversion).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void u8hwc_to_f32chw_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                              long long hw, int swap_rb)
{
    const int b = blockIdx.y;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;          // group of 4 pixels
    const long long p0 = q * 4;
    if (p0 >= hw) return;
    const uint8_t* s = src + (size_t)b * hw * 3 + p0 * 3;
    float* d = dst + (size_t)b * hw * 3 + p0;
    const int c0 = swap_rb ? 2 : 0, c2 = swap_rb ? 0 : 2;
    if (p0 + 4 <= hw && ((size_t)b * hw * 3) % 4 == 0 && hw % 4 == 0) {
        const uint32_t w0 = *reinterpret_cast<const uint32_t*>(s), w1 = *reinterpret_cast<const uint32_t*>(s + 4),
                       w2 = *reinterpret_cast<const uint32_t*>(s + 8);
        uint8_t v[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = (w0 >> (8 * i)) & 0xff; v[4 + i] = (w1 >> (8 * i)) & 0xff; v[8 + i] = (w2 >> (8 * i)) & 0xff; }
        f32x4 o0, o1, o2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o0[i] = (float)v[3 * i + c0] / 255.0f;
            o1[i] = (float)v[3 * i + 1] / 255.0f;
            o2[i] = (float)v[3 * i + c2] / 255.0f;
        }
        *reinterpret_cast<f32x4*>(d) = o0;
        *reinterpret_cast<f32x4*>(d + hw) = o1;
        *reinterpret_cast<f32x4*>(d + 2 * hw) = o2;
    } else {
        for (int i = 0; i < 4 && p0 + i < hw; ++i) {
            d[i] = (float)s[3 * i + c0] / 255.0f;
            d[hw + i] = (float)s[3 * i + 1] / 255.0f;
            d[2 * hw + i] = (float)s[3 * i + c2] / 255.0f;
        }
    }
}

TUP_DEVICE uint32_t to_u8(float x) {
    const float v = fminf(fmaxf(x * 255.0f, 0.0f), 255.0f);                 // NaN -> 0 like clamp on a NaN-free model output
    return (uint32_t)v;                                                     // truncation, as tensor.to(torch.uint8)
}

__global__ __launch_bounds__(256) void f32chw_to_u8hwc_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                              long long hw, int swap_rb)
{
    const int b = blockIdx.y;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long p0 = q * 4;
    if (p0 >= hw) return;
    const float* s = src + (size_t)b * hw * 3 + p0;
    uint8_t* d = dst + (size_t)b * hw * 3 + p0 * 3;
    const int c0 = swap_rb ? 2 : 0, c2 = swap_rb ? 0 : 2;
    if (p0 + 4 <= hw && hw % 4 == 0) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(s + (size_t)c0 * hw), g = *reinterpret_cast<const f32x4*>(s + hw),
                    c = *reinterpret_cast<const f32x4*>(s + (size_t)c2 * hw);
        uint32_t v[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[3 * i] = to_u8(a[i]); v[3 * i + 1] = to_u8(g[i]); v[3 * i + 2] = to_u8(c[i]); }
        *reinterpret_cast<uint32_t*>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        *reinterpret_cast<uint32_t*>(d + 4) = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
        *reinterpret_cast<uint32_t*>(d + 8) = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
    } else {
        for (int i = 0; i < 4 && p0 + i < hw; ++i) {
            d[3 * i] = (uint8_t)to_u8(s[(size_t)c0 * hw + i]);
            d[3 * i + 1] = (uint8_t)to_u8(s[hw + i]);
            d[3 * i + 2] = (uint8_t)to_u8(s[(size_t)c2 * hw + i]);
        }
    }
}

// ---- transforms.Resize on a uint8 image = Pillow's two-pass 8-bit resampler (reference data_handling/data_class.py:61-71,
// inference.py:65-75).  Integer arithmetic, bit-exact with Pillow: out = clip8((2^21 + sum(pixel * k)) >> 22), k = the
// normalised triangle weights with 22 fractional bits (tables from resize_taps.pil_bilinear_coeffs). ----
constexpr int PIL_PRECISION_BITS = 32 - 8 - 2;
TUP_DEVICE uint32_t clip8(int v) { v >>= PIL_PRECISION_BITS; return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// horizontal pass: src u8 [B][H][W][3] -> dst u8 [B][H][Wo][3]; a thread owns one output pixel (its taps are 3*n contiguous bytes)
__global__ __launch_bounds__(256) void resize_u8_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             const int* __restrict__ xmin, const int* __restrict__ xsize,
                                                             const int* __restrict__ kk, int ksize, int H, int W, int Wo)
{
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (ox >= Wo || y >= H) return;
    const uint8_t* s = src + ((size_t)((size_t)b * H + y) * W + xmin[ox]) * 3;
    const int* k = kk + (size_t)ox * ksize;
    const int n = xsize[ox];
    int s0 = 1 << (PIL_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < n; ++i) {
        const int kv = k[i];
        s0 += (int)s[3 * i] * kv; s1 += (int)s[3 * i + 1] * kv; s2 += (int)s[3 * i + 2] * kv;
    }
    uint8_t* d = dst + ((size_t)((size_t)b * H + y) * Wo + ox) * 3;
    d[0] = (uint8_t)clip8(s0); d[1] = (uint8_t)clip8(s1); d[2] = (uint8_t)clip8(s2);
}

// vertical pass: src u8 [B][H][W][3] -> dst u8 [B][Ho][W][3] and / or fp32 planar [B][3][Ho][W] = value / 255 (ToTensor fused)
__global__ __launch_bounds__(256) void resize_u8_cols_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst_u8,
                                                             float* __restrict__ dst_f32, const int* __restrict__ ymin,
                                                             const int* __restrict__ ysize, const int* __restrict__ kk, int ksize,
                                                             int H, int W, int Ho, int swap_rb)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= W || oy >= Ho) return;
    const uint8_t* s = src + ((size_t)((size_t)b * H + ymin[oy]) * W + x) * 3;
    const int* k = kk + (size_t)oy * ksize;
    const int n = ysize[oy];
    int s0 = 1 << (PIL_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < n; ++i) {
        const int kv = k[i];
        const uint8_t* r = s + (size_t)i * W * 3;
        s0 += (int)r[0] * kv; s1 += (int)r[1] * kv; s2 += (int)r[2] * kv;
    }
    const uint32_t v0 = clip8(s0), v1 = clip8(s1), v2 = clip8(s2);
    if (dst_u8) {
        uint8_t* d = dst_u8 + ((size_t)((size_t)b * Ho + oy) * W + x) * 3;
        d[0] = (uint8_t)v0; d[1] = (uint8_t)v1; d[2] = (uint8_t)v2;
    }
    if (dst_f32) {
        const size_t hw = (size_t)Ho * W;
        float* d = dst_f32 + (size_t)b * 3 * hw + (size_t)oy * W + x;
        d[0] = (float)(swap_rb ? v2 : v0) / 255.0f; d[hw] = (float)v1 / 255.0f; d[2 * hw] = (float)(swap_rb ? v0 : v2) / 255.0f;
    }
}

// ---- NV12 (YUV 4:2:0: a Y plane and a half-resolution plane of (Cb, Cr) pairs, both pitched) <-> fp32 planar RGB.  Integer
// arithmetic on bytes throughout ("NV12 frames"), so the result is a definition, not an approximation: chroma sited
// "left" (sample (j, i) at luma column 2i, between luma rows 2j and 2j + 1), upsampled by the [1 3] / [3 1] vertical and
// [2] / [1 1] horizontal taps without intermediate rounding, 16.16 matrix; the encode filters with [1 2 1] over rows 2j, 2j + 1.
// A lane owns 4 luma columns x 2 luma rows = 2 chroma pairs; consecutive lanes run along a row pair.  ALIGNED (pointers, pitches and batch strides multiples of 4,
// W % 4 == 0): dwords on the byte side, 16-byte vectors per plane row on the fp32 side; the chroma neighbours (rows j - 1, j + 1,
// pair i + 1; on the encode column x - 1) are plain loads of lines the neighbouring lanes and waves fetch anyway.  Otherwise bytes
// and floats one by one, columns past W skipped.  The coefficient rows arrive by value: scalar operands. ----
struct Nv12Dec { int yoff, cy, rv, bu, gu, gv; };
struct Nv12Enc { int yadd, ry, gy, by, ur, ug, ub, vr, vg, vb; };          // yadd = (yoff << 16) + 32768

TUP_DEVICE int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// ... for bytes that are packed into a dword next.  The empty asm hides the clamp from instruction selection: left visible,
// clip(v >> n) pairs under an OR become gfx950's v_ashr_pk_u8_i32 followed by a v_or3_b32 of bytes 2 and 3.  Observed on the device
// with that code: bytes 2 and 3 of the packed word came out OR-ed with what the destination register of the v_ashr_pk held before
// (an address half in one row, a byte value, hence right, in the other), as if the instruction wrote its low half only.
TUP_DEVICE uint32_t sat8_packable(int v) { int r = sat8(v); asm("" : "+v"(r)); return (uint32_t)r; }

template <bool ALIGNED>
__global__ __launch_bounds__(256) void nv12_to_f32chw_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp,
                                                             long long ybs, int ypitch, long long uvbs, int uvpitch,
                                                             float* __restrict__ dst, int H, int W, Nv12Dec k)
{
    // byte / 255 as the IEEE quotient, once per workgroup: the 24 results of a lane are then LDS reads instead of 24 divides of
    // ~10 instructions each, which made the kernel as much VALU- as HBM-bound
    __shared__ float unit[256];
    unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    // Workgroups go to the 8 XCDs in turn, and a chroma row is read by three row pairs: numbered as launched, those sit on different
    // XCDs and every L2 fetches the row for itself (counters at 8 x 2160 x 3840: 158 MB fetched for 100 MB).  So XCD x takes the
    // x-th contiguous band of the frame instead (the first nb % 8 bands one workgroup longer).  This takes the part's 8 XCDs and a
    // round-robin that starts at workgroup 0 of the launch for granted: with frames in blockIdx.y and gridDim.x % 8 != 0 the phase
    // shifts by gridDim.x % 8 per frame, so for b > 0 a band may be spread over XCDs again (the counter run above has 8 frames and gridDim.x % 8 == 2
    // and still fetched the algorithmic 100 MB, so the loss, if any, is small there).  The numbering is a bijection of [0, gridDim.x)
    // for any placement: a wrong guess costs re-fetches, never results.
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7, per = nb >> 3, rem = nb & 7;
    const unsigned wg = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    const unsigned lin = wg * 256u + threadIdx.x, groups = (unsigned)(W + 3) >> 2;              // lanes run along a row pair, then on
    const int j = (int)(lin / groups), q = (int)(lin - (unsigned)j * groups), b = blockIdx.y;
    const int x = 4 * q, h2 = H >> 1, w2 = W >> 1;
    if (j >= h2) return;
    const uint8_t* ys = yp + (long long)b * ybs + (size_t)(2 * j) * ypitch + x;
    const uint8_t* uvb = uvp + (long long)b * uvbs;
    const uint8_t* c[3] = {uvb + (size_t)(j > 0 ? j - 1 : 0) * uvpitch, uvb + (size_t)j * uvpitch,
                           uvb + (size_t)(j + 1 < h2 ? j + 1 : h2 - 1) * uvpitch};
    const int i0 = 2 * q;
    int t[3][3][2];                                                         // [chroma row j-1, j, j+1][pair i0, i0+1, i0+2][Cb, Cr]
    if (ALIGNED) {
        const int in = i0 + 2 < w2 ? i0 + 2 : w2 - 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const uint32_t a = *reinterpret_cast<const uint32_t*>(c[r] + 2 * i0);
            const uint32_t n = *reinterpret_cast<const uint16_t*>(c[r] + 2 * in);
            t[r][0][0] = a & 0xff; t[r][0][1] = (a >> 8) & 0xff; t[r][1][0] = (a >> 16) & 0xff; t[r][1][1] = a >> 24;
            t[r][2][0] = n & 0xff; t[r][2][1] = n >> 8;
        }
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int ip = i0 + p < w2 ? i0 + p : w2 - 1;
#pragma unroll
            for (int r = 0; r < 3; ++r) { t[r][p][0] = c[r][2 * ip]; t[r][p][1] = c[r][2 * ip + 1]; }
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
            const uint32_t w = *reinterpret_cast<const uint32_t*>(ys + (size_t)r * ypitch);
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[i] = (w >> (8 * i)) & 0xff;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) yv[i] = x + i < W ? ys[(size_t)r * ypitch + i] : 0;
        }
        f32x4 o0, o1, o2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = i >> 1;
            const int cb = ((i & 1) ? v[p][0] + v[p + 1][0] : 2 * v[p][0]) - 1024;       // 8 x (Cb - 128)
            const int cr = ((i & 1) ? v[p][1] + v[p + 1][1] : 2 * v[p][1]) - 1024;
            const int base = __mul24(k.cy, yv[i] - k.yoff) + 32768;         // 24-bit factors, products below 2^31: full-rate multiplies
            o0[i] = unit[sat8((base + __mul24(k.rv, cr)) >> 16)];
            o1[i] = unit[sat8((base + __mul24(k.gu, cb) + __mul24(k.gv, cr)) >> 16)];
            o2[i] = unit[sat8((base + __mul24(k.bu, cb)) >> 16)];
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
__global__ __launch_bounds__(256) void f32chw_to_nv12_kernel(const float* __restrict__ src, uint8_t* __restrict__ yp,
                                                             uint8_t* __restrict__ uvp, long long ybs, int ypitch, long long uvbs,
                                                             int uvpitch, int H, int W, Nv12Enc k)
{
    const unsigned lin = blockIdx.x * 256u + threadIdx.x, groups = (unsigned)(W + 3) >> 2;
    const int j = (int)(lin / groups), b = blockIdx.y;
    const int x = 4 * (int)(lin - (unsigned)j * groups), h2 = H >> 1;
    if (j >= h2) return;
    const size_t hw = (size_t)H * W;
    const float* s = src + (size_t)b * 3 * hw + (size_t)(2 * j) * W + x;
    const int left = x > 0 ? 1 : 0;                                         // column x - 1, clamped to the image
    int p[2][3][5];                                                         // bytes of [row][channel][column x - 1 .. x + 3]
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* sr = s + (size_t)ch * hw + (size_t)r * W;
            p[r][ch][0] = (int)to_u8(sr[-left]);
            if (ALIGNED) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(sr);
#pragma unroll
                for (int i = 0; i < 4; ++i) p[r][ch][1 + i] = (int)to_u8(a[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) p[r][ch][1 + i] = x + i < W ? (int)to_u8(sr[i]) : 0;
            }
        }
    uint8_t* yd = yp + (long long)b * ybs + (size_t)(2 * j) * ypitch + x;
    uint8_t* ud = uvp + (long long)b * uvbs + (size_t)j * uvpitch + x;      // pair i = x / 2 starts at byte x
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t yv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            yv[i] = sat8_packable((__mul24(k.ry, p[r][0][1 + i]) + __mul24(k.gy, p[r][1][1 + i]) + __mul24(k.by, p[r][2][1 + i]) + k.yadd) >> 16);
        if (ALIGNED) {
            *reinterpret_cast<uint32_t*>(yd + (size_t)r * ypitch) = yv[0] | (yv[1] << 8) | (yv[2] << 16) | (yv[3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) yd[(size_t)r * ypitch + i] = (uint8_t)yv[i];
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
        const int half = (128 << 19) + (1 << 18);
        cv[2 * pr] = sat8_packable((__mul24(k.ur, f[0]) + __mul24(k.ug, f[1]) + __mul24(k.ub, f[2]) + half) >> 19);
        cv[2 * pr + 1] = sat8_packable((__mul24(k.vr, f[0]) + __mul24(k.vg, f[1]) + __mul24(k.vb, f[2]) + half) >> 19);
    }
    if (ALIGNED) {
        *reinterpret_cast<uint32_t*>(ud) = cv[0] | (cv[1] << 8) | (cv[2] << 16) | (cv[3] << 24);
    } else {
        ud[0] = (uint8_t)cv[0]; ud[1] = (uint8_t)cv[1];                     // W is even: columns x, x + 1 exist
        if (x + 2 < W) { ud[2] = (uint8_t)cv[2]; ud[3] = (uint8_t)cv[3]; }
    }
}

// limited / full range x bt601 / bt709, from Kr, Kb as DESIGN 3 derives them (tests/test_yuv_cpu.py recomputes both tables)
constexpr Nv12Dec NV12_DEC[2][2] = {{{16, 76309, 13075, 16525, -3209, -6660}, {0, 65536, 11485, 14516, -2819, -5850}},
                                    {{16, 76309, 14686, 17305, -1747, -4366}, {0, 65536, 12901, 15201, -1535, -3835}}};
constexpr int NV12_ENC[2][2][9] = {{{16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681},
                                    {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}},
                                   {{11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639},
                                    {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}}};

// shared argument check of the two NV12 entries: 0 = launch, -1 = nothing to do, else the error to return
int nv12_check(int y_pitch, int uv_pitch, int B, int H, int W, int matrix, int full_range)
{
    if (B <= 0 || H <= 0 || W <= 0) return -1;
    if (B > 65535 || (H & 1) || (W & 1) || y_pitch < W || uv_pitch < W || matrix < 0 || matrix > 1 || full_range < 0 ||
        full_range > 1 || (long long)(H / 2) * ((W + 3) / 4) > 0x7fffff00ll)
        return (int)hipErrorInvalidValue;
    return 0;
}

// one lane per 4 columns x 2 rows, numbered along a row pair and on to the next: 256 consecutive ones per workgroup, frames in y
dim3 nv12_grid(int B, int H, int W) { return dim3((unsigned)(((long long)(H / 2) * ((W + 3) / 4) + 255) / 256), B); }

bool nv12_aligned(const void* y, const void* uv, long long ybs, int y_pitch, long long uvbs, int uv_pitch, const void* f32, int W)
{
    return ((uintptr_t)y | (uintptr_t)uv | (uintptr_t)ybs | (uintptr_t)uvbs | (uintptr_t)y_pitch | (uintptr_t)uv_pitch |
            (uintptr_t)W) % 4 == 0 && (uintptr_t)f32 % 16 == 0;
}

}  // namespace

// An NV12 surface -> fp32 planar RGB in [0, 1] = "convert to RGB24, then ToTensor", bit-exact with the integer definition of
// DESIGN 3.  y u8 [B][H][W] (row pitch y_pitch, batch stride y_batch_stride, both in bytes), uv u8 [B][H/2][W/2][2] = (Cb, Cr)
// (uv_pitch, uv_batch_stride); dst fp32 [B][3][H][W].  One launch, no allocation, no synchronisation: capturable.
extern "C" int tup_nv12_to_f32chw(const void* y, const void* uv, long long y_batch_stride, int y_pitch, long long uv_batch_stride,
                                  int uv_pitch, float* dst, int B, int H, int W, int matrix, int full_range, void* stream)
{
    if (const int e = nv12_check(y_pitch, uv_pitch, B, H, W, matrix, full_range)) return e < 0 ? 0 : e;
    const dim3 grid = nv12_grid(B, H, W);
    const Nv12Dec k = NV12_DEC[matrix][full_range];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nv12_aligned(y, uv, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, dst, W))
        nv12_to_f32chw_kernel<true><<<grid, dim3(256), 0, st>>>((const uint8_t*)y, (const uint8_t*)uv, y_batch_stride, y_pitch,
                                                                uv_batch_stride, uv_pitch, dst, H, W, k);
    else
        nv12_to_f32chw_kernel<false><<<grid, dim3(256), 0, st>>>((const uint8_t*)y, (const uint8_t*)uv, y_batch_stride, y_pitch,
                                                                 uv_batch_stride, uv_pitch, dst, H, W, k);
    TUP_CHECK_LAUNCH();
    return 0;
}

// fp32 planar RGB -> an NV12 surface: bytes as tup_f32chw_to_u8hwc makes them (trunc(clamp(x * 255, 0, 255)), NaN -> 0), then the
// integer matrix and the [1 2 1] x [1 1] chroma filter of DESIGN 3.  Same layout arguments; bytes between W and the pitch are
// not written.
extern "C" int tup_f32chw_to_nv12(const float* src, void* y, void* uv, long long y_batch_stride, int y_pitch,
                                  long long uv_batch_stride, int uv_pitch, int B, int H, int W, int matrix, int full_range,
                                  void* stream)
{
    if (const int e = nv12_check(y_pitch, uv_pitch, B, H, W, matrix, full_range)) return e < 0 ? 0 : e;
    const dim3 grid = nv12_grid(B, H, W);
    const int* c = NV12_ENC[matrix][full_range];
    const Nv12Enc k = {((full_range ? 0 : 16) << 16) + 32768, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nv12_aligned(y, uv, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, src, W))
        f32chw_to_nv12_kernel<true><<<grid, dim3(256), 0, st>>>(src, (uint8_t*)y, (uint8_t*)uv, y_batch_stride, y_pitch,
                                                                uv_batch_stride, uv_pitch, H, W, k);
    else
        f32chw_to_nv12_kernel<false><<<grid, dim3(256), 0, st>>>(src, (uint8_t*)y, (uint8_t*)uv, y_batch_stride, y_pitch,
                                                                 uv_batch_stride, uv_pitch, H, W, k);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Pillow's horizontal 8-bit resampling pass (Image.resize(..., BILINEAR) on an RGB image, the arithmetic behind
// transforms.Resize on a PIL image: reference data_handling/data_class.py:61-71, inference.py:65-75).
// src u8 [B][H][W][3] -> dst u8 [B][H][Wo][3]; xmin / xsize int32 [Wo], k int32 [Wo][ksize] (22 fractional bits).
extern "C" int tup_resize_u8_rows(const void* src, void* dst, const int* xmin, const int* xsize, const int* k, int ksize,
                                  int B, int H, int W, int Wo, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0 || Wo <= 0) return 0;
    if (B > 65535 || ksize < 1 || (H + 3) / 4 > 65535) return (int)hipErrorInvalidValue;
    resize_u8_rows_kernel<<<dim3((Wo + 63) / 64, (H + 3) / 4, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)src, (uint8_t*)dst, xmin, xsize, k, ksize, H, W, Wo);
    TUP_CHECK_LAUNCH();
    return 0;
}

// ... and its vertical pass, optionally fused with ToTensor: src u8 [B][H][W][3] -> dst_u8 u8 [B][Ho][W][3] (may be NULL) and /
// or dst_f32 fp32 [B][3][Ho][W] = value / 255 (may be NULL; swap_rb = 1 reads BGR into RGB planes).
extern "C" int tup_resize_u8_cols(const void* src, void* dst_u8, float* dst_f32, const int* ymin, const int* ysize, const int* k,
                                  int ksize, int B, int H, int W, int Ho, int swap_rb, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0) return 0;
    if (B > 65535 || ksize < 1 || (Ho + 3) / 4 > 65535 || (!dst_u8 && !dst_f32)) return (int)hipErrorInvalidValue;
    resize_u8_cols_kernel<<<dim3((W + 63) / 64, (Ho + 3) / 4, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)src, (uint8_t*)dst_u8, dst_f32, ymin, ysize, k, ksize, H, W, Ho, swap_rb);
    TUP_CHECK_LAUNCH();
    return 0;
}

// src u8 [B][H][W][3] -> dst fp32 [B][3][H][W] = src / 255; swap_rb = 1 reads BGR frames (screen grabs) into RGB planes.
extern "C" int tup_u8hwc_to_f32chw(const void* src, float* dst, int B, int H, int W, int swap_rb, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (B > 65535) return (int)hipErrorInvalidValue;
    const long long hw = (long long)H * W;
    const long long groups = (hw + 3) / 4;
    u8hwc_to_f32chw_kernel<<<dim3((unsigned)((groups + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)src, dst, hw, swap_rb);
    TUP_CHECK_LAUNCH();
    return 0;
}

// src fp32 [B][3][H][W] -> dst u8 [B][H][W][3] = trunc(clamp(src * 255, 0, 255)); swap_rb = 1 writes BGR.
extern "C" int tup_f32chw_to_u8hwc(const float* src, void* dst, int B, int H, int W, int swap_rb, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (B > 65535) return (int)hipErrorInvalidValue;
    const long long hw = (long long)H * W;
    const long long groups = (hw + 3) / 4;
    f32chw_to_u8hwc_kernel<<<dim3((unsigned)((groups + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        src, (uint8_t*)dst, hw, swap_rb);
    TUP_CHECK_LAUNCH();
    return 0;
}
