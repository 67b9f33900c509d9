// The front half of a baseline JPEG encoder as libjpeg computes it, shared by the training degradations (degrade.hip: a 4:4:4 round
// trip on bytes) and the encoder (jpeg_encode.hip): the 16-bit RGB -> YCbCr conversion, the "slow integer" forward DCT (jfdctint.c),
// the Annex K tables scaled to a quality, and the quantiser; and the inverse DCT (jidctint.c) that degrade.hip and the decoder
// (jpeg_decode.hip) share, and the workgroup scan of the two codecs.  All in 32-bit integers; stated in numpy in tests/_degrade_ref.py and pinned there to Pillow.
#pragma once
#include "common.h"

namespace {
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;
constexpr int dg_fix(double x) { return (int)(x * 65536 + .5); }

// Annex K, natural order [vertical frequency][horizontal frequency]
__constant__ uint8_t dg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

TUP_DEVICE int dg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// entry i (natural order) of table `tab` (0 luma, 1 chroma) at `quality` 1..100: jpeg_quality_scaling, then clamped to a baseline table
TUP_DEVICE int dg_quant_entry(int quality, int tab, int i)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    return min(max(((int)dg_base[tab][i] * s + 50) / 100, 1), 255);
}
// floor(2^32 / (8 t)) + 1 (for a power of two this is 2^32 / (8 t) itself: exact too); see dg_quant_div
TUP_DEVICE uint32_t dg_quant_rcp(int t) { return 0xffffffffu / (uint32_t)(8 * t) + 1u; }
// (|c| + 4 t) / (8 t), the magnitude of a quantised coefficient.  n = |c| + 4 t < 2^16 and 8 t < 2^11, so with m = floor(2^32 / (8 t)) + 1
// the high word of n m is the quotient: n m / 2^32 exceeds n / (8 t) by less than n / 2^32 < 1 / (8 t), too little to reach the next integer
TUP_DEVICE int dg_quant_div(int c, int t, uint32_t rcp) { return (int)__umulhi((uint32_t)abs(c) + (uint32_t)(4 * t), rcp); }

// libjpeg's jccolor.c: Y, Cb, Cr in 0..255 from bytes
TUP_DEVICE void dg_rgb_to_ycc(int R, int G, int B, int& Y, int& Cb, int& Cr)
{
    Y = (dg_fix(.299) * R + dg_fix(.587) * G + dg_fix(.114) * B + 32768) >> 16;
    Cb = (-dg_fix(.16874) * R - dg_fix(.33126) * G + dg_fix(.5) * B + (128 << 16) + 32767) >> 16;
    Cr = (dg_fix(.5) * R - dg_fix(.41869) * G - dg_fix(.08131) * B + (128 << 16) + 32767) >> 16;
}

// libjpeg's jfdctint.c, one pass over d[0..8): FIRST = the row pass (outputs scaled up by 4), else the column pass (scaled back)
template <bool FIRST>
TUP_DEVICE void dg_fdct8(int (&d)[8])
{
    constexpr int N = FIRST ? 11 : 15;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : dg_descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : dg_descale(t10 - t11, 2);
    int z1 = (t12 + t13) * F_0_541196100;
    d[2] = dg_descale(z1 + t13 * F_0_765366865, N);
    d[6] = dg_descale(z1 - t12 * F_1_847759065, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F_1_175875602;
    t4 *= F_0_298631336; t5 *= F_2_053119869; t6 *= F_3_072711026; t7 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5; z4 = z4 * -F_0_390180644 + z5;
    d[7] = dg_descale(t4 + z1 + z3, N); d[5] = dg_descale(t5 + z2 + z4, N);
    d[3] = dg_descale(t6 + z2 + z3, N); d[1] = dg_descale(t7 + z1 + z4, N);
}

TUP_DEVICE int dg_clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// libjpeg's jidctint.c, one pass: FIRST = the column pass (descale by 11), else the row pass (by 18)
template <bool FIRST>
TUP_DEVICE void dg_idct8(int (&d)[8])
{
    constexpr int N = FIRST ? 11 : 18;
    int z1 = (d[2] + d[6]) * F_0_541196100;
    int t2 = z1 - d[6] * F_1_847759065, t3 = z1 + d[2] * F_0_765366865;
    int t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7]; t1 = d[5]; t2 = d[3]; t3 = d[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * F_1_175875602;
    t0 *= F_0_298631336; t1 *= F_2_053119869; t2 *= F_3_072711026; t3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5; z4 = z4 * -F_0_390180644 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    d[0] = dg_descale(t10 + t3, N); d[7] = dg_descale(t10 - t3, N);
    d[1] = dg_descale(t11 + t2, N); d[6] = dg_descale(t11 - t2, N);
    d[2] = dg_descale(t12 + t1, N); d[5] = dg_descale(t12 - t1, N);
    d[3] = dg_descale(t13 + t0, N); d[4] = dg_descale(t13 - t0, N);
}

constexpr int DG_SCAN_THREADS = 256;
// exclusive sum over a workgroup of DG_SCAN_THREADS lanes (the encoder's and the decoder's); `total` = the sum of all.  Ends on a
// barrier, so the buffer may be used again at once.
TUP_DEVICE int dg_scan256(int v, int (&buf)[2][DG_SCAN_THREADS], int tid, int& total)
{
    buf[0][tid] = v;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int d = 1; d < DG_SCAN_THREADS; d <<= 1) {
        int x = buf[cur][tid];
        if (tid >= d) x += buf[cur][tid - d];
        buf[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    const int incl = buf[cur][tid];
    total = buf[cur][DG_SCAN_THREADS - 1];
    __syncthreads();
    return incl - v;
}
}  // namespace
