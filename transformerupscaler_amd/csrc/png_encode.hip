// PNG files (8- or 16-bit RGB, no interlace) of a whole batch on the GPU: `ops.png_encode`, DESIGN 7m.  tests/_png_ref.py (8 bits) and
// tests/_png16_ref.py (16 bits) state the file in Python and the files here equal them byte for byte; png_deflate.h holds the serial
// parts, which the host tests under sanitizers.  The kernels are templates on BPS, the bytes of a sample: a pixel is bpp = 3 BPS bytes
// (16-bit samples big-endian, quantised from fp32 by q_16, which rounds to nearest), a row 1 + 3 BPS W bytes, the left neighbour of a
// byte is bpp bytes back; filters work on bytes, and everything after the filtered byte is the same code.  The text below says 3 W for
// the 8-bit form.
//
// What makes the coder parallel: the filtered stream, H * (1 + 3 W) bytes that depend on the pixels alone, is cut into ranges of
// `block_bytes` bytes (row boundaries are ignored, so no row has to fit LDS), and every range is ONE deflate block that starts and ends
// on a byte boundary: a block that is not stored is followed by an empty stored block (zlib's sync flush), and nothing refers back
// across a block.  Each block is its own IDAT chunk, so its workgroup also computes its own CRC-32.  Launches:
//   0. png_filter_kernel        a workgroup per (row, image): the five sums of |residual|, the smallest wins (adaptive only)
//                                                                                                       -> filters uint8 [B][H]
//   1. png_block_kernel<false>  a workgroup per (block, image): filtered bytes into LDS, runs, histogram, code lengths, the exact bits
//                               of the three block forms                          -> sizes int32 [B][N], Adler partials int32 [B][N]
//   2. png_scan_kernel          a workgroup per image: exclusive sum of the sizes after the 33 bytes of signature and IHDR, the
//                               Adler-32 from the partials, the file's length (-1 where it does not fit)
//   3. png_block_kernel<true>   the same work again, then the codes OR-ed into an LDS bit buffer, the chunk's CRC, and stores of whole
//                               dwords where the destination allows.  Block 0 adds signature and IHDR, the last block the IDAT with
//                               the Adler-32 and IEND.  Images of length -1 are skipped.
// Nothing is kept between launches 1 and 3 but the sizes: keeping tokens would be at least a byte per filtered byte written and read.
//
// Inside a block (n <= 32768 bytes, 256 lanes):
//   a. a lane per byte (strided) reads the pixel, its left, upper and upper-left neighbours straight from the frame (uint8 HWC, or fp32
//      CHW quantised by tensor_to_frames' rule) and stores the filtered byte in LDS; the Adler partial is summed on the way.
//   b. tokens: literals and matches at distance 1.  A maximal run of r equal bytes is a literal, (r - 1) / 258 matches of 258, then a
//      match of the rest when it is 3 or more, else literals.  A lane owns the runs that START in its piece of the block (a piece is an
//      odd number of words, so that the lanes' byte walks meet different banks); a suffix minimum over the lanes' first starts tells a
//      lane where a run that leaves its piece ends.  Lanes therefore emit tokens in stream order and a scan of their bit counts
//      places them.
//   c. histograms per wave (LDS atomics; four copies so that near-constant data does not serialise the whole workgroup on one word),
//      summed; ranks by (count, symbol) on a lane per symbol; Moffat-Katajainen and the length limit on one lane (png_deflate.h);
//      the header's run-length code and its 7-bit code on one lane; bit totals of both Huffman forms from the histogram.
//   d. <true> only: canonical codes on a lane per symbol, the header by lane 0, the tokens by all lanes (ds_or), the CRC by pieces
//      combined with multiplications modulo the CRC polynomial, then the copy out.
// All global writes are ordinary vector stores.
#include "common.h"
#include "jpeg_dct.h"
#include "png_deflate.h"
#include "png_kernels.h"

namespace {
// ---- launch 2 ----
// sizes int32 [B][N] -> offsets int32 [B][N] = 33 + the sizes before; lengths[b] = the file's length, or -1 beyond capacity;
// adlers[b] = the Adler-32 of the filtered stream from the blocks' partials
__global__ __launch_bounds__(PN_THREADS) void png_scan_kernel(const int* __restrict__ sizes, const int* __restrict__ partials, int N, int L, int bb,
                                                              long long capacity, int* __restrict__ offsets, int* __restrict__ lengths,
                                                              int* __restrict__ adlers)
{
    __shared__ int buf[2][PN_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    long long base = PN_HEAD;
    uint32_t A = 1, Bsum = 0;
    for (int k0 = 0; k0 < N; k0 += PN_THREADS) {
        const int k = k0 + tid;
        int total;
        const int v = k < N ? sizes[(size_t)b * N + k] : 0;
        const int before = dg_scan256(v, buf, tid, total);                         // a tile is at most 256 x (32768 + 47) bytes
        if (k < N) offsets[(size_t)b * N + k] = (int)min(base + before, 0x7fffffffLL);
        base = min(base + total, capacity + 1);
        // Adler: a block moves (A, B) to (A + a, B + n A + b)
        const uint32_t p = k < N ? (uint32_t)partials[(size_t)b * N + k] : 0u;
        const uint32_t n = k < N ? (uint32_t)min(bb, L - k * bb) : 0u;
        int a_total, t_total;
        const int a_before = dg_scan256((int)(p & 0xffffu), buf, tid, a_total);
        const uint32_t A_here = (A + (uint32_t)a_before) % PD_ADLER;
        const uint32_t term = k < N ? (n % PD_ADLER) * A_here % PD_ADLER + (p >> 16) : 0u;
        dg_scan256((int)term, buf, tid, t_total);
        A = (A + (uint32_t)a_total) % PD_ADLER;
        Bsum = (Bsum + (uint32_t)t_total) % PD_ADLER;
    }
    if (tid == 0) {
        lengths[b] = base <= capacity ? (int)base : -1;
        adlers[b] = (int)(Bsum << 16 | A);
    }
}

int pn_offsets(int bps, const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, int* offsets,
               int* lengths, int* adlers, void* stream)
{
    const int N = pn_blocks(H, W, block_bytes, bps);
    if (N < 1 || !sizes || !partials || !offsets || !lengths || !adlers || B < 1 || B > 65535 || capacity < 0 || capacity > 0x7fffffffLL)
        return (int)hipErrorInvalidValue;
    png_scan_kernel<<<dim3((unsigned)B), dim3(PN_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(sizes, partials, N, H * (1 + 3 * bps * W),
                                                                                                       block_bytes, capacity, offsets, lengths, adlers);
    TUP_CHECK_LAUNCH();
    return 0;
}
}  // namespace

// The number of deflate blocks N of an H x W image cut every block_bytes bytes (what sizes the [B][N] workspaces), or -1 for what the
// encoder refuses: a side below 1, H * (1 + 3 W) from 2^31, block_bytes outside 256..32768.
extern "C" int tup_png_blocks(int H, int W, int block_bytes) { return pn_blocks(H, W, block_bytes, 1); }

// Launch 0 (adaptive filtering only): filters uint8 [B][H] <- the filter of every row.  Exactly one of frames_u8 (uint8 [B][H][W][3],
// RGB) and frames_f32 (fp32 [B][3][H][W], quantised as tensor_to_frames does) is given, here and below.
extern "C" int tup_png_filters(const void* frames_u8, const float* frames_f32, int B, int H, int W, void* filters, void* stream)
{
    return pn_filters<1>(frames_u8, frames_f32, B, H, W, filters, stream);
}

// Launch 1: sizes int32 [B][N] <- the bytes every block adds to the file, partials int32 [B][N] <- its Adler partial.  filter: 0..4 one
// filter for every row, 5 adaptive (then `filters` is launch 0's).
extern "C" int tup_png_sizes(const void* frames_u8, const float* frames_f32, int B, int H, int W, int filter, int block_bytes,
                             const void* filters, int* sizes, int* partials, void* stream)
{
    return pn_sizes<1>(frames_u8, frames_f32, B, H, W, filter, block_bytes, filters, sizes, partials, stream);
}

// Launch 2: offsets int32 [B][N], lengths int32 [B] and adlers int32 [B] from sizes and partials; capacity = the bytes of an image's
// row in `data`.
extern "C" int tup_png_offsets(const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, int* offsets,
                               int* lengths, int* adlers, void* stream)
{
    return pn_offsets(1, sizes, partials, B, H, W, block_bytes, capacity, offsets, lengths, adlers, stream);
}

// Launch 3: data uint8 [B][capacity] <- the whole file of every image whose length is not -1.
extern "C" int tup_png_write(const void* frames_u8, const float* frames_f32, int B, int H, int W, int filter, int block_bytes,
                             const void* filters, const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity,
                             void* stream)
{
    return pn_write<1>(frames_u8, frames_f32, B, H, W, filter, block_bytes, filters, offsets, lengths, adlers, data, capacity, stream);
}

// The block count and the scan of 16-bit files (rows of 1 + 6 W bytes); their three pixel-reading launches are in png16_encode.hip.
extern "C" int tup_png16_blocks(int H, int W, int block_bytes) { return pn_blocks(H, W, block_bytes, 2); }

extern "C" int tup_png16_offsets(const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, int* offsets,
                                 int* lengths, int* adlers, void* stream)
{
    return pn_offsets(2, sizes, partials, B, H, W, block_bytes, capacity, offsets, lengths, adlers, stream);
}
