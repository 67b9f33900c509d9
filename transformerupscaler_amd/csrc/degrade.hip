// Training degradations of a whole batch in one launch: blur, noise and a JPEG round trip on bytes, between `tup_patch_pairs` and the
// model (data.PatchSampler(degrade=...); the reference trains on clean bilinear downscales only, data_handling/data_class.py:24-75).
// Everything is integer arithmetic on bytes, stated in numpy in tests/_degrade_ref.py and pinned there to Pillow's 4:4:4 JPEG round
// trip (DESIGN 7j has the definition in full).  The stages are functions of degrade_stages.h, which degrade420.hip (the launch that
// also knows the 4:2:0 round trip) runs too; the numbers below name them in the order the kernel calls them.
//
// Per sample, a 32-byte record {taps[4], noise_amp, noise_seed, quality, flags}; the input is quantised u = clip(floor(v * 255 + .5)):
//   blur   separable 7 taps {k3 k2 k1 k0 k1 k2 k3} in Pillow's 22-bit fixed point, horizontal then vertical, each pass rounded to a
//          byte, indices clamped to the image.  {1 << 22, 0, 0, 0} is the identity by arithmetic, not by a branch.
//   noise  n = the four bytes of drop_hash(noise_seed, e) summed, - 510; u = clip(u + ((n * noise_amp + 32768) >> 16)); e = (y W + x) 3 + c,
//          or y W + x for all three channels with flags & 1.  noise_amp = 0 is off.
//   JPEG   quality 1..100 (0 is off): baseline 4:4:4 with the Annex K tables, libjpeg's 16-bit colour conversion and its "slow integer"
//          DCT both ways; entropy coding is lossless and not performed.
//
// A workgroup owns one 32 x 32 tile of one sample: 16 JPEG blocks per channel, whose grid starts at the image's origin, so a tile
// never shares a block with its neighbour.  It
//   1. stages the tile plus the 3-pixel blur halo from the fp32 input into LDS as bytes (coordinates clamped to the image);
//   2. runs the horizontal pass into a second byte tile, and the vertical pass and the noise into the first, 4 bytes a lane;
//   3. converts to YCbCr into an int tile, replicating the last column / row into the blocks that leave the image;
//   4. row DCT (a lane per row of a block), then column DCT + quantise + dequantise + column IDCT in registers (a lane per column of a
//      block), then row IDCT, all in place;
//   5. converts back and writes fp32, 16 bytes per store where the width and the base allow it.
// The int tile's rows are 33 words apart: in the row passes a 32-lane half holds 8 rows x 4 blocks, whose k-th words sit at banks
// (row + 8 block + k) % 32, all different; at 32 words apart the 8 rows would share a bank.  In the column passes a half holds 32
// neighbouring columns of one row.  No intermediate reaches memory; every output has one writer: no atomics, no workspace.
// Bound: its own instruction stream.  A batch of 64 patches of side 96 is 576 workgroups, 2.25 per CU and all resident at once, and
// moves 14 MB: 19 us with every stage on, 12 us with every stage off, against 3 us for the bytes alone.
#include "degrade_stages.h"      // the stages themselves, shared with degrade420.hip
#include "jpeg_dct.h"            // colour conversion, both DCTs, tables and quantiser: shared with jpeg_encode.hip and jpeg_decode.hip

static_assert(sizeof(DegradeRec) == 32, "degrade record = 32 bytes (the host packs it as eight 32-bit words)");

namespace {
__global__ __launch_bounds__(DG_THREADS) void degrade_lr_kernel(const float* __restrict__ in, const DegradeRec* __restrict__ recs,
                                                               int H, int W, float* __restrict__ out)
{
    using G = DgWindow<DG_TILE>;
    __shared__ __attribute__((aligned(16))) uint8_t win[G::WIN_BYTES];            // [ch][38][40]: the window, then the bytes after blur and noise
    __shared__ __attribute__((aligned(16))) uint8_t hpass[G::HPASS_BYTES];        // [ch][38][32]: the horizontal pass
    __shared__ int pl[3 * DG_TILE * DG_PS];                                       // [ch][32][33]: YCbCr - 128, coefficients, and back
    __shared__ int qt[2][64];                                                     // the quantiser tables: luma, chroma
    __shared__ uint32_t qr[2][64];                                                // floor(2^32 / (8 t)) + 1

    const int b = blockIdx.y, tid = threadIdx.x;
    const DegradeRec rec = recs[b];
    const int ntx = (W + DG_TILE - 1) / DG_TILE;
    const int tx0 = (blockIdx.x % ntx) * DG_TILE, ty0 = (blockIdx.x / ntx) * DG_TILE;
    const int tw = min(DG_TILE, W - tx0), th = min(DG_TILE, H - ty0);
    const size_t plane = (size_t)H * W;
    const bool jpeg = rec.quality >= 1 && rec.quality <= 100;
    const DgBox box = {tx0, ty0, 0, th, 0, tw};

    if (jpeg) dg_load_tables(rec.quality, qt, qr, tid);
    dg_stage<DG_TILE>(in + (size_t)b * 3 * plane, plane, H, W, box, win, tid);
    __syncthreads();
    dg_blur_rows<DG_TILE>(rec.taps, box, win, hpass, tid);
    __syncthreads();
    dg_blur_cols_noise<DG_TILE>(rec, W, box, hpass, win, tid);
    __syncthreads();
    if (jpeg) dg_jpeg444(win, pl, qt, qr, tw, th, tid);
    dg_store<DG_TILE>(win, out + (size_t)b * 3 * plane, (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, plane, W, tx0, ty0, tw, th, tid);
}
}  // namespace

// in / out: fp32 [B][3][H][W], values in [0, 1]; recs: device array [B] of 32-byte records
// {int taps[4]; int noise_amp; uint32_t noise_seed; int quality; int flags}.  out must not overlap in (a tile reads its neighbours' halo).
extern "C" int tup_degrade_lr(const float* in, const void* recs, int B, int H, int W, float* out, void* stream)
{
    if (!in || !recs || !out || B <= 0 || H <= 0 || W <= 0 || B > 65535) return (int)hipErrorInvalidValue;
    const long long n = (long long)B * 3 * H * W;
    if (in < out + n && out < in + n) return (int)hipErrorInvalidValue;
    const long long tiles = (long long)((W + DG_TILE - 1) / DG_TILE) * ((H + DG_TILE - 1) / DG_TILE);
    if (tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    degrade_lr_kernel<<<dim3((unsigned)tiles, (unsigned)B), dim3(DG_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        in, (const DegradeRec*)recs, H, W, out);
    TUP_CHECK_LAUNCH();
    return 0;
}
