// 16-bit PNG files: the encoder of png_encode.hip instantiated for two-byte samples (png_kernels.h, BPS = 2).  IHDR depth 16, samples
// big-endian, bpp = 6, rows of 1 + 6 W filtered bytes; tests/_png16_ref.py states the file.  tup_png16_blocks and tup_png16_offsets, which
// read no pixel, sit beside the scan kernel in png_encode.hip.
#include "png_kernels.h"

// The same four launches for 16-bit files (IHDR depth 16, samples big-endian, rows of 1 + 6 W bytes; refused from H * (1 + 6 W) = 2^31):
// frames_u16 is uint16 [B][H][W][3] in the machine's byte order, frames_f32 fp32 [B][3][H][W] quantised by q_16 (round to nearest).
extern "C" int tup_png16_filters(const void* frames_u16, const float* frames_f32, int B, int H, int W, void* filters, void* stream)
{
    if ((uintptr_t)frames_u16 & 1) return (int)hipErrorInvalidValue;
    return pn_filters<2>(frames_u16, frames_f32, B, H, W, filters, stream);
}

extern "C" int tup_png16_sizes(const void* frames_u16, const float* frames_f32, int B, int H, int W, int filter, int block_bytes,
                               const void* filters, int* sizes, int* partials, void* stream)
{
    if ((uintptr_t)frames_u16 & 1) return (int)hipErrorInvalidValue;
    return pn_sizes<2>(frames_u16, frames_f32, B, H, W, filter, block_bytes, filters, sizes, partials, stream);
}

extern "C" int tup_png16_write(const void* frames_u16, const float* frames_f32, int B, int H, int W, int filter, int block_bytes,
                               const void* filters, const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity,
                               void* stream)
{
    if ((uintptr_t)frames_u16 & 1) return (int)hipErrorInvalidValue;
    return pn_write<2>(frames_u16, frames_f32, B, H, W, filter, block_bytes, filters, offsets, lengths, adlers, data, capacity, stream);
}
