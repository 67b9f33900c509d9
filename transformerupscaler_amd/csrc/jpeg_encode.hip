// Baseline sequential JPEG (SOF0) of a whole batch on the GPU: `ops.jpeg_encode`, DESIGN 7k.  The file of image b is byte for byte what
// Pillow's save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=R) writes (libjpeg's default path: standard Huffman
// tables, no optimisation); tests/_jpeg_ref.py states it in numpy and tests/test_jpeg_cpu.py pins that to Pillow.
//
// The restart interval is what makes the coder parallel: a restart segment (R MCU rows) starts on a byte boundary with its DC
// predictors at zero, so it depends on nothing but its own pixels.  Three launches:
//   1. jpeg_segment_kernel<false>   a workgroup per (segment, image): colour, downsample, DCT, quantise, code; counts the segment's bytes,
//                                   stuffed zeros and its closing marker included                     -> sizes int32 [B][S]
//   2. jpeg_scan_kernel             a workgroup per image: exclusive sum of the sizes after the header -> offsets int32 [B][S], and
//                                   lengths int32 [B] (-1 where the file does not fit the row it was given)
//   3. jpeg_segment_kernel<true>    the same work again, every byte stored at its final place; segment 0 also copies the header,
//                                   which the host built from the parameters.  Images of length -1 are skipped.
// Recomputing costs less than keeping coefficients: 2 B a coefficient would be 3 B per pixel written and read back.  The only
// workspace is the two int32 [B][S] arrays.
//
// A segment of an 8K row is 480 MCUs and does not fit LDS at once, so its workgroup walks it in chunks of JP_BLOCKS = 96 blocks (16
// MCUs of 4:2:0, 32 of 4:4:4), carrying the bits of the last unfinished byte, the three DC predictors and the byte count.  Per chunk:
//   a. samples: a lane per 2 x 2 pixels (4:2:0) or per pixel (4:4:4) reads RGB (uint8 HWC, or fp32 CHW quantised by tensor_to_frames'
//      rule trunc(clamp(x * 255, 0, 255))), converts, and stores level-shifted samples block by block.  Coordinates are clamped to the
//      image, which is libjpeg's edge replication, with one exception it makes itself: below the last chroma row of a 4:2:0 image the
//      DOWNSAMPLED row is repeated, not the downsample of repeated rows (these differ when H is even).
//   b. forward DCT by rows, then by columns with the quantiser (jpeg_dct.h), in place; a block is 65 words apart from the next so that
//      the lanes of step d, one per block, meet in different banks.
//   c. 4:2:0: the luma blocks of an edge MCU that lie beyond the image's blocks are not made from pixels; libjpeg codes them as DC of
//      the block before, AC zero.
//   d. a lane per block walks the zigzag twice: first for the block's bit count, then, after a scan of the counts, to put its codes
//      into the chunk's bit buffer in LDS (ds_or: neighbouring blocks share a word).  The buffer is sized for the worst block, 22 + 63 x
//      26 bits, so no content can overrun it.
//   e. bytes: a lane per run of bytes counts its 0xFF, a scan gives every byte its place, and the run is stored with the zeros stuffed.
// After the last chunk the open byte is padded with ones and RSTm (m = segment mod 8) or, for the last segment, EOI follows.
// All global writes are ordinary vector stores.  Bound: the coder of step d, one lane per block with 96 of 256 lanes busy; DESIGN 7k
// has the times.
#include "common.h"
#include "jpeg_dct.h"

namespace {
constexpr int JP_THREADS = 256;
constexpr int JP_BLOCKS = 96;                               // blocks per chunk
constexpr int JP_PITCH = 65;                                // words from one block to the next
constexpr int JP_BLOCK_BITS = 22 + 63 * 26;                 // DC: 11-bit code + 11 bits; AC: 16-bit code + 10 bits
constexpr int JP_WORDS = (7 + JP_BLOCKS * JP_BLOCK_BITS + 31) / 32 + 2;

struct JpHuff { uint32_t v[256]; };                         // by symbol: length << 16 | code
struct JpSpec { uint8_t counts[16]; uint8_t symbols[162]; };
constexpr JpHuff jp_codes(const JpSpec& s)
{
    JpHuff h{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int c = 0; c < s.counts[len - 1]; ++c) h.v[s.symbols[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
    return h;
}
// Annex K.3 - K.6
constexpr JpSpec JP_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpSpec JP_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpSpec JP_AC_LUMA = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr JpSpec JP_AC_CHROMA = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
// [DC luma, DC chroma, AC luma, AC chroma]
__constant__ const JpHuff jp_huff[4] = {jp_codes(JP_DC_LUMA), jp_codes(JP_DC_CHROMA), jp_codes(JP_AC_LUMA), jp_codes(JP_AC_CHROMA)};
// natural index of the k-th coefficient in zigzag order
__constant__ const uint8_t jp_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpShared {
    int coef[JP_BLOCKS * JP_PITCH];                         // samples, then coefficients, by block
    uint32_t bits[JP_WORDS];                                // the chunk's bit stream, MSB first: bit p is bit 31 - p % 32 of word p / 32
    uint32_t ac[2][256];                                    // length << 16 | code
    uint32_t dc[2][12];
    int qt[2][64];
    uint32_t qr[2][64];
    int scan[2][JP_THREADS];
    int pred[3];                                            // the DC of the last block of each component before this chunk
    uint8_t zz[64];
};

TUP_DEVICE int jp_to_u8(float x) { return (int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }      // tensor_to_frames' rule (image_io.hip)

// one pixel as bytes; exactly one of u8 (HWC) and f32 (CHW) is set, both already at the image
TUP_DEVICE void jp_rgb(const uint8_t* u8, const float* f32, size_t plane, int W, int y, int x, int& R, int& G, int& B)
{
    const size_t i = (size_t)y * W + x;
    if (u8) {
        R = u8[i * 3]; G = u8[i * 3 + 1]; B = u8[i * 3 + 2];
    } else {
        R = jp_to_u8(f32[i]); G = jp_to_u8(f32[plane + i]); B = jp_to_u8(f32[2 * plane + i]);
    }
}

TUP_DEVICE int jp_nbits(int v) { return 32 - __clz(abs(v)); }                                   // __clz(0) = 32

// `len` <= 27 bits of `val` at bit `pos` of the stream
TUP_DEVICE void jp_put(uint32_t* bits, int& pos, uint32_t val, int len)
{
    const int w = pos >> 5, o = pos & 31;
    const uint64_t v = (uint64_t)val << (64 - o - len);
    atomicOr(&bits[w], (uint32_t)(v >> 32));
    if ((uint32_t)v) atomicOr(&bits[w + 1], (uint32_t)v);
    pos += len;
}

// WRITE = false: seg[b][s] <- the bytes of segment s.  WRITE = true: seg[b][s] is where segment s starts in its image's row.
template <bool WRITE>
__global__ __launch_bounds__(JP_THREADS) void jpeg_segment_kernel(const uint8_t* __restrict__ frames_u8, const float* __restrict__ frames_f32,
                                                                  int H, int W, int quality, int sub, int restart_rows, int S,
                                                                  const uint8_t* __restrict__ header, int header_len, int* __restrict__ seg,
                                                                  const int* __restrict__ lengths, uint8_t* __restrict__ data, long long capacity)
{
    __shared__ JpShared sh;
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    if (WRITE && lengths[b] < 0) return;                                          // the file does not fit its row: nothing of it is written

    const int msize = sub == 2 ? 16 : 8, bpm = sub == 2 ? 6 : 3, mpc = JP_BLOCKS / bpm;
    const int mw = (W + msize - 1) / msize, mh = (H + msize - 1) / msize;
    const int interval = restart_rows * mw;
    const int m_begin = s * interval, m_end = min(mw * mh, m_begin + interval);
    const int wb = (W + 7) >> 3, hb = (H + 7) >> 3;                                // luma blocks the image has
    const size_t plane = (size_t)H * W;
    const uint8_t* u8 = frames_u8 ? frames_u8 + (size_t)b * plane * 3 : nullptr;
    const float* f32 = frames_f32 ? frames_f32 + (size_t)b * plane * 3 : nullptr;
    uint8_t* row = WRITE ? data + (size_t)b * (size_t)capacity : nullptr;
    const long long seg_at = WRITE ? (long long)seg[(size_t)b * S + s] : 0;

    for (int i = tid; i < 512; i += JP_THREADS) sh.ac[i >> 8][i & 255] = jp_huff[2 + (i >> 8)].v[i & 255];
    if (tid < 24) sh.dc[tid / 12][tid % 12] = jp_huff[tid / 12].v[tid % 12];
    if (tid < 64) sh.zz[tid] = jp_zigzag[tid];
    if (tid < 128) {
        const int t = dg_quant_entry(quality, tid >> 6, tid & 63);
        sh.qt[tid >> 6][tid & 63] = t;
        sh.qr[tid >> 6][tid & 63] = dg_quant_rcp(t);
    }
    if (tid < 3) sh.pred[tid] = 0;
    if (WRITE && s == 0)
        for (int i = tid; i < header_len; i += JP_THREADS) row[i] = header[i];
    __syncthreads();

    uint32_t open_bits = 0;                                                        // the unfinished byte, its bits at the top
    int open_n = 0;                                                                // how many of them, 0..7
    long long done = 0;                                                            // bytes of this segment so far

    for (int c0 = m_begin; c0 < m_end; c0 += mpc) {
        const int n = min(mpc, m_end - c0), nblk = n * bpm;

        // ---- a. samples ----
        if (sub == 2) {
            const int hc = (H + 1) >> 1;                                           // chroma rows the image has
            for (int i = tid; i < n * 64; i += JP_THREADS) {
                const int mi = i >> 6, qy = (i >> 3) & 7, qx = i & 7;
                const int mcu = c0 + mi, my = mcu / mw, mx = mcu - my * mw;
                const int x0 = min(mx * 16 + 2 * qx, W - 1), x1 = min(mx * 16 + 2 * qx + 1, W - 1);
                const int ly0 = min(my * 16 + 2 * qy, H - 1), ly1 = min(my * 16 + 2 * qy + 1, H - 1);
                const int cy = min(my * 8 + qy, hc - 1), cy0 = 2 * cy, cy1 = min(2 * cy + 1, H - 1);
                int* yb = sh.coef + (mi * 6 + (qy >> 2) * 2 + (qx >> 2)) * JP_PITCH + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
                int R, G, B, Y, Cb, Cr, sb = 0, sr = 0;
                jp_rgb(u8, f32, plane, W, ly0, x0, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); yb[0] = Y - 128; sb += Cb; sr += Cr;
                jp_rgb(u8, f32, plane, W, ly0, x1, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); yb[1] = Y - 128; sb += Cb; sr += Cr;
                jp_rgb(u8, f32, plane, W, ly1, x0, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); yb[8] = Y - 128; sb += Cb; sr += Cr;
                jp_rgb(u8, f32, plane, W, ly1, x1, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); yb[9] = Y - 128; sb += Cb; sr += Cr;
                if (cy0 != ly0 || cy1 != ly1) {                                    // below the last chroma row: that row again
                    sb = sr = 0;
                    jp_rgb(u8, f32, plane, W, cy0, x0, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); sb += Cb; sr += Cr;
                    jp_rgb(u8, f32, plane, W, cy0, x1, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); sb += Cb; sr += Cr;
                    jp_rgb(u8, f32, plane, W, cy1, x0, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); sb += Cb; sr += Cr;
                    jp_rgb(u8, f32, plane, W, cy1, x1, R, G, B); dg_rgb_to_ycc(R, G, B, Y, Cb, Cr); sb += Cb; sr += Cr;
                }
                const int bias = 1 + (qx & 1);                                     // 1, 2, 1, 2 along a chroma row (a block starts on an even column)
                sh.coef[(mi * 6 + 4) * JP_PITCH + qy * 8 + qx] = ((sb + bias) >> 2) - 128;
                sh.coef[(mi * 6 + 5) * JP_PITCH + qy * 8 + qx] = ((sr + bias) >> 2) - 128;
            }
        } else {
            for (int i = tid; i < n * 64; i += JP_THREADS) {
                const int mi = i >> 6, r = (i >> 3) & 7, c = i & 7;
                const int mcu = c0 + mi, my = mcu / mw, mx = mcu - my * mw;
                int R, G, B, Y, Cb, Cr;
                jp_rgb(u8, f32, plane, W, min(my * 8 + r, H - 1), min(mx * 8 + c, W - 1), R, G, B);
                dg_rgb_to_ycc(R, G, B, Y, Cb, Cr);
                int* d = sh.coef + mi * 3 * JP_PITCH + r * 8 + c;
                d[0] = Y - 128; d[JP_PITCH] = Cb - 128; d[2 * JP_PITCH] = Cr - 128;
            }
        }
        __syncthreads();

        // ---- b. forward DCT: rows, then columns with the quantiser ----
        for (int i = tid; i < nblk * 8; i += JP_THREADS) {
            int* p = sh.coef + (i >> 3) * JP_PITCH + (i & 7) * 8;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k];
            dg_fdct8<true>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k] = d[k];
        }
        __syncthreads();
        for (int i = tid; i < nblk * 8; i += JP_THREADS) {
            const int blk = i >> 3, c = i & 7, j = blk % bpm, tab = sub == 2 ? (j >= 4) : (j > 0);
            int* p = sh.coef + blk * JP_PITCH + c;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k * 8];
            dg_fdct8<false>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = dg_quant_div(d[k], sh.qt[tab][k * 8 + c], sh.qr[tab][k * 8 + c]);
                p[k * 8] = d[k] < 0 ? -q : q;
            }
        }
        __syncthreads();

        // ---- c. 4:2:0: luma blocks of an edge MCU beyond the image's blocks ----
        if (sub == 2 && ((wb & 1) || (hb & 1))) {
            if (tid < n) {
                const int mcu = c0 + tid, my = mcu / mw, mx = mcu - my * mw;
                for (int j = 1; j < 4; ++j) {
                    if (2 * my + (j >> 1) < hb && 2 * mx + (j & 1) < wb) continue;
                    int* p = sh.coef + (tid * 6 + j) * JP_PITCH;
                    p[0] = p[-JP_PITCH];
                    for (int k = 1; k < 64; ++k) p[k] = 0;
                }
            }
            __syncthreads();
        }

        // ---- d. code lengths, their scan, then the codes ----
        const int j = tid % bpm, mi = tid / bpm;
        const int comp = sub == 2 ? (j < 4 ? 0 : j - 3) : j, tab = comp > 0;
        const int* blk = sh.coef + tid * JP_PITCH;
        int diff = 0, nbits = 0;
        if (tid < nblk) {
            int before;                                                            // the block before this one in its component
            if (sub == 2 && j > 0 && j < 4) before = tid - 1;
            else if (mi == 0) before = -1;
            else before = (sub == 2 && j == 0) ? tid - 3 : tid - bpm;
            diff = blk[0] - (before < 0 ? sh.pred[comp] : sh.coef[before * JP_PITCH]);
            const int ds = jp_nbits(diff);
            nbits = (int)(sh.dc[tab][ds] >> 16) + ds;
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                const int v = blk[sh.zz[k]];
                if (v == 0) { ++run; continue; }
                nbits += (run >> 4) * (int)(sh.ac[tab][0xF0] >> 16);
                const int sz = jp_nbits(v);
                nbits += (int)(sh.ac[tab][((run & 15) << 4) | sz] >> 16) + sz;
                run = 0;
            }
            if (run) nbits += (int)(sh.ac[tab][0] >> 16);
        }
        int chunk_bits;
        const int at = dg_scan256(nbits, sh.scan, tid, chunk_bits);
        const int total = open_n + chunk_bits;
        const bool last = c0 + mpc >= m_end;
        for (int i = tid; i < ((total + 7 + 31) >> 5) + 1; i += JP_THREADS) sh.bits[i] = i == 0 ? open_bits << 24 : 0u;
        __syncthreads();
        if (tid < nblk) {
            int pos = open_n + at;
            const int ds = jp_nbits(diff);
            const uint32_t dcode = sh.dc[tab][ds];
            // a negative value is sent as the low bits of value - 1
            jp_put(sh.bits, pos, ((dcode & 0xffffu) << ds) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << ds) - 1u)), (int)(dcode >> 16) + ds);
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                const int v = blk[sh.zz[k]];
                if (v == 0) { ++run; continue; }
                for (; run > 15; run -= 16) jp_put(sh.bits, pos, sh.ac[tab][0xF0] & 0xffffu, (int)(sh.ac[tab][0xF0] >> 16));      // ZRL
                const int sz = jp_nbits(v);
                const uint32_t code = sh.ac[tab][(run << 4) | sz];
                jp_put(sh.bits, pos, ((code & 0xffffu) << sz) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u)), (int)(code >> 16) + sz);
                run = 0;
            }
            if (run) jp_put(sh.bits, pos, sh.ac[tab][0] & 0xffffu, (int)(sh.ac[tab][0] >> 16));                                    // EOB
            // the last block of each component hands its DC to the next chunk (every lane has read sh.pred before the scan's barriers)
            if (mi == n - 1 && (sub == 2 ? j >= 3 : true)) sh.pred[comp] = blk[0];
        }
        __syncthreads();

        // ---- e. bytes ----
        int nbytes = total >> 3, rest = total & 7;
        if (last && rest) {                                                        // pad the open byte with ones
            if (tid == 0) sh.bits[nbytes >> 2] |= ((1u << (8 - rest)) - 1u) << (24 - 8 * (nbytes & 3));
            ++nbytes; rest = 0;
            __syncthreads();
        }
        const int per = (nbytes + JP_THREADS - 1) / JP_THREADS;
        const int i0 = min(tid * per, nbytes), i1 = min(i0 + per, nbytes);
        int ff = 0;
        for (int i = i0; i < i1; ++i) ff += ((sh.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
        int ff_total;
        const int ff_before = dg_scan256(ff, sh.scan, tid, ff_total);
        if (WRITE) {
            long long o = seg_at + done + i0 + ff_before;
            for (int i = i0; i < i1; ++i) {
                const uint32_t v = (sh.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
                if (o < capacity) row[o] = (uint8_t)v;
                ++o;
                if (v == 255u) {
                    if (o < capacity) row[o] = 0;
                    ++o;
                }
            }
        }
        done += nbytes + ff_total;
        open_n = rest;
        open_bits = rest ? ((sh.bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u) & (0xffu << (8 - rest)) : 0u;
        __syncthreads();
    }

    if (tid == 0) {
        if (WRITE) {
            const long long o = seg_at + done;
            if (o + 1 < capacity) { row[o] = 0xFF; row[o + 1] = (uint8_t)(s == S - 1 ? 0xD9 : 0xD0 + (s & 7)); }
        } else {
            seg[(size_t)b * S + s] = (int)min(done + 2, 0x7fffffffLL);
        }
    }
}

// sizes int32 [B][S] -> offsets int32 [B][S] = header_len + the sizes before; lengths[b] = the file's length, or -1 beyond capacity
__global__ __launch_bounds__(JP_THREADS) void jpeg_scan_kernel(const int* __restrict__ sizes, int S, int header_len, long long capacity,
                                                               int* __restrict__ offsets, int* __restrict__ lengths)
{
    __shared__ int buf[2][JP_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    long long base = header_len;
    for (int s0 = 0; s0 < S; s0 += JP_THREADS) {
        const int s = s0 + tid;
        int total;
        const int v = s < S ? sizes[(size_t)b * S + s] : 0;
        // a tile's sum stays below 2^31 unless the file is beyond any capacity: then the length is -1 and the offsets are not used
        const int before = dg_scan256(v, buf, tid, total);
        if (s < S) offsets[(size_t)b * S + s] = (int)min(max(base + before, 0LL), 0x7fffffffLL);
        base = total < 0 ? capacity + 1 : min(base + total, capacity + 1);
    }
    if (tid == 0) lengths[b] = base <= capacity ? (int)base : -1;
}

int jp_segments(int H, int W, int sub, int restart_rows)
{
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (sub != 0 && sub != 2) || restart_rows < 1) return -1;
    const int m = sub == 2 ? 16 : 8, mw = (W + m - 1) / m, mh = (H + m - 1) / m;
    if ((long long)restart_rows * mw > 65535) return -1;
    return (mh + restart_rows - 1) / restart_rows;
}
}  // namespace

// The number of restart segments S of an H x W image (what sizes the [B][S] workspaces), or -1 for parameters the encoder refuses:
// sizes outside 1..65535, a subsampling other than 0 (4:4:4) / 2 (4:2:0), restart_rows < 1 or a restart interval above 65535 MCUs.
extern "C" int tup_jpeg_segments(int H, int W, int subsampling, int restart_rows) { return jp_segments(H, W, subsampling, restart_rows); }

// Launch 1: sizes int32 [B][S] <- the bytes of every restart segment.  Exactly one of frames_u8 (uint8 [B][H][W][3], RGB) and frames_f32
// (fp32 [B][3][H][W], quantised as tensor_to_frames does) is given.
extern "C" int tup_jpeg_sizes(const void* frames_u8, const float* frames_f32, int B, int H, int W, int quality, int subsampling,
                              int restart_rows, int* sizes, void* stream)
{
    const int S = jp_segments(H, W, subsampling, restart_rows);
    if (S < 1 || !sizes || (!frames_u8) == (!frames_f32) || B < 1 || B > 65535 || quality < 1 || quality > 100) return (int)hipErrorInvalidValue;
    jpeg_segment_kernel<false><<<dim3((unsigned)S, (unsigned)B), dim3(JP_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)frames_u8, frames_f32, H, W, quality, subsampling, restart_rows, S, nullptr, 0, sizes, nullptr, nullptr, 0);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Launch 2: offsets int32 [B][S] and lengths int32 [B] from sizes; capacity = the bytes of an image's row in `data`.
extern "C" int tup_jpeg_offsets(const int* sizes, int B, int S, int header_len, long long capacity, int* offsets, int* lengths, void* stream)
{
    if (!sizes || !offsets || !lengths || B < 1 || B > 65535 || S < 1 || header_len < 0 || capacity < 0 || capacity > 0x7fffffffLL)
        return (int)hipErrorInvalidValue;
    jpeg_scan_kernel<<<dim3((unsigned)B), dim3(JP_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(sizes, S, header_len, capacity, offsets, lengths);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Launch 3: data uint8 [B][capacity] <- header, scan and EOI of every image whose length is not -1.  header: header_len bytes on the
// device, SOI .. SOS, built by the caller from the same parameters.
extern "C" int tup_jpeg_write(const void* frames_u8, const float* frames_f32, int B, int H, int W, int quality, int subsampling,
                              int restart_rows, const void* header, int header_len, const int* offsets, const int* lengths, void* data,
                              long long capacity, void* stream)
{
    const int S = jp_segments(H, W, subsampling, restart_rows);
    if (S < 1 || !offsets || !lengths || !header || header_len < 1 || (!frames_u8) == (!frames_f32) || B < 1 || B > 65535 || quality < 1 ||
        quality > 100 || capacity < 0 || capacity > 0x7fffffffLL || (!data && capacity > 0))
        return (int)hipErrorInvalidValue;
    if (capacity == 0) return 0;                                                   // nothing fits: every length is -1 already
    jpeg_segment_kernel<true><<<dim3((unsigned)S, (unsigned)B), dim3(JP_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)frames_u8, frames_f32, H, W, quality, subsampling, restart_rows, S, (const uint8_t*)header, header_len,
        const_cast<int*>(offsets), lengths, (uint8_t*)data, capacity);
    TUP_CHECK_LAUNCH();
    return 0;
}
