// P010 video frames (YUV 4:2:0, 10 bit: what an HEVC Main10 / AV1 10-bit decoder hands over) <-> fp32 planar RGB: the 10-bit format
// of the kernels in yuv420_kernels.h, which image_io.hip instantiates for NV12 ("P010 frames").  A sample is a little-endian
// uint16 with its 10-bit code in the high bits: a reader takes sample >> 6 and ignores the low six bits, a writer stores code << 6.
// The tensor is code / 1023 (the IEEE quotient, never through 8 bits); the encode quantises with q_10 (round to nearest, below).
// ALIGNED moves dwords of two samples on the 16-bit side.
#include "common.h"
#include "yuv420_kernels.h"

namespace {

TUP_DEVICE int lo_code(uint32_t w) { return (int)((w & 0xffffu) >> 6); }
TUP_DEVICE int hi_code(uint32_t w) { return (int)(w >> 22); }
TUP_DEVICE uint32_t two_samples(uint32_t a, uint32_t b) { return (a << 6) | (b << 22); }

struct P010Fmt {
    typedef uint16_t sample_t;
    static constexpr int BITS = 10, SHIFT = 6, MATRICES = 3;
    // q_10: t = x * 1023; NaN -> 0 (fmaxf); clamp; (int)(t + 0.5f).  The clamp sits between the multiply and the add: no fma can form.
    static TUP_DEVICE int quantise(float x)
    {
        const float t = fminf(fmaxf(x * 1023.0f, 0.0f), 1023.0f);
        return (int)(t + 0.5f);
    }
    static TUP_DEVICE void load2(const uint8_t* p, int* c)
    {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        c[0] = lo_code(w); c[1] = hi_code(w);
    }
    static TUP_DEVICE void load4(const uint8_t* p, int* c) { load2(p, c); load2(p + 4, c + 2); }
    static TUP_DEVICE void store4(uint8_t* p, const uint32_t* c)
    {
        *reinterpret_cast<uint32_t*>(p) = two_samples(c[0], c[1]);
        *reinterpret_cast<uint32_t*>(p + 4) = two_samples(c[2], c[3]);
    }
    // [bt601, bt709, bt2020][limited, full], from Kr, Kb as DESIGN 3 derives them (tests/test_p010_cpu.py pins both tables)
    static constexpr Yuv420Dec DEC[3][2] = {{{64, 76533, 13113, 16574, -3219, -6679}, {0, 65536, 11485, 14516, -2819, -5850}},
                                            {{64, 76533, 14729, 17356, -1752, -4378}, {0, 65536, 12901, 15201, -1535, -3835}},
                                            {{64, 76533, 13792, 17597, -1539, -5344}, {0, 65536, 12080, 15412, -1348, -4681}}};
    static constexpr int ENC[3][2][9] = {{{16780, 32941, 6398, -9685, -19015, 28700, 28700, -24033, -4667},
                                          {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}},
                                         {{11931, 40136, 4052, -6576, -22124, 28700, 28700, -26068, -2632},
                                          {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}},
                                         {{14742, 38049, 3328, -8015, -20685, 28700, 28700, -26392, -2308},
                                          {17216, 44434, 3886, -9151, -23617, 32768, 32768, -30133, -2635}}};
};

}  // namespace

// A P010 surface -> fp32 planar RGB in [0, 1], bit-exact with the integer definition of DESIGN 3 ("P010 frames").  y u16 [B][H][W]
// (row pitch y_pitch, batch stride y_batch_stride, both in bytes and even), uv u16 [B][H/2][W/2][2] = (Cb, Cr) (uv_pitch,
// uv_batch_stride); dst fp32 [B][3][H][W].  One launch, no allocation, no synchronisation: capturable.
extern "C" int tup_p010_to_f32chw(const void* y, const void* uv, long long y_batch_stride, int y_pitch, long long uv_batch_stride,
                                  int uv_pitch, float* dst, int B, int H, int W, int matrix, int full_range, void* stream)
{
    return yuv420_decode<P010Fmt>(y, uv, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, dst, B, H, W, matrix, full_range, stream);
}

// fp32 planar RGB -> a P010 surface: codes q_10(x) (round to nearest, NaN -> 0), then the integer matrix and the [1 2 1] x [1 1]
// chroma filter of DESIGN 3; samples are code << 6.  Same layout arguments; samples between W and the pitch are not written.
extern "C" int tup_f32chw_to_p010(const float* src, void* y, void* uv, long long y_batch_stride, int y_pitch,
                                  long long uv_batch_stride, int uv_pitch, int B, int H, int W, int matrix, int full_range,
                                  void* stream)
{
    return yuv420_encode<P010Fmt>(src, y, uv, y_batch_stride, y_pitch, uv_batch_stride, uv_pitch, B, H, W, matrix, full_range, stream);
}
