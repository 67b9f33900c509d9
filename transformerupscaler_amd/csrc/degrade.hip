// Training degradations of a whole batch in one launch: blur, noise and a JPEG round trip on bytes, between `tup_patch_pairs` and the
// model (data.PatchSampler(degrade=...); the reference trains on clean bilinear downscales only, data_handling/data_class.py:24-75).
// Everything is integer arithmetic on bytes, stated in numpy in tests/_degrade_ref.py and pinned there to Pillow's 4:4:4 JPEG round
// trip (DESIGN 7j has the definition in full).
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
#include "common.h"
#include "jpeg_dct.h"      // colour conversion, both DCTs, tables and quantiser: shared with jpeg_encode.hip and jpeg_decode.hip

struct DegradeRec {
    int taps[4];
    int noise_amp;
    uint32_t noise_seed;
    int quality, flags;
};
static_assert(sizeof(DegradeRec) == 32, "degrade record = 32 bytes (the host packs it as eight 32-bit words)");

namespace {
constexpr int DG_TILE = 32;                        // tile side: a multiple of the 8 x 8 JPEG block
constexpr int DG_HALO = 3;                         // blur radius
constexpr int DG_WIN = DG_TILE + 2 * DG_HALO;      // 38
constexpr int DG_WS = 40;                          // byte pitch of a window row
constexpr int DG_PS = DG_TILE + 1;                 // word pitch of an int tile row (see above)
constexpr int DG_PRECISION_BITS = 32 - 8 - 2;      // Pillow's PRECISION_BITS for 8-bit images
constexpr int DG_THREADS = 256;
constexpr int DG_QUADS = DG_TILE / 4;              // 4-byte groups of a tile row

// one output of a blur pass from its seven inputs, rounded to a byte as Pillow's resampler does
TUP_DEVICE int dg_blur7(const int (&k)[4], int a0, int a1, int a2, int a3, int a4, int a5, int a6)
{
    const int s = ((1 << (DG_PRECISION_BITS - 1)) + k[0] * a3 + k[1] * (a2 + a4) + k[2] * (a1 + a5) + k[3] * (a0 + a6)) >> DG_PRECISION_BITS;
    // The shift and the clip stay two instructions.  Left to itself hipcc (clang 22, ROCm 7.2) joins two neighbouring results into one
    // v_ashr_pk_u8_i32 and ORs the other two bytes of the dword on top of it as if the instruction had cleared bits 16-31 of its
    // destination; it leaves them as they were, and the stale bits came out in bytes 2 and 3 of every dword of the horizontal pass.
    return dg_clip255((int)opaque_copy((uint32_t)s));
}

__global__ __launch_bounds__(DG_THREADS) void degrade_lr_kernel(const float* __restrict__ in, const DegradeRec* __restrict__ recs,
                                                               int H, int W, float* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[3 * DG_WIN * DG_WS];      // [ch][38][40]: the window, then the bytes after blur and noise
    __shared__ __attribute__((aligned(16))) uint8_t hpass[3 * DG_WIN * DG_TILE];  // [ch][38][32]: the horizontal pass
    __shared__ int pl[3 * DG_TILE * DG_PS];                                       // [ch][32][33]: YCbCr - 128, coefficients, and back
    __shared__ int qt[2][64];                                                     // the quantiser tables: luma, chroma
    __shared__ uint32_t qr[2][64];                                                // floor(2^32 / (8 t)) + 1

    const int b = blockIdx.y, tid = threadIdx.x;
    const DegradeRec rec = recs[b];
    const int ntx = (W + DG_TILE - 1) / DG_TILE;
    const int tx0 = (blockIdx.x % ntx) * DG_TILE, ty0 = (blockIdx.x / ntx) * DG_TILE;
    const int tw = min(DG_TILE, W - tx0), th = min(DG_TILE, H - ty0);
    const size_t plane = (size_t)H * W;
    const float* src = in + (size_t)b * 3 * plane;
    const bool jpeg = rec.quality >= 1 && rec.quality <= 100;

    if (jpeg && tid < 128) {
        const int t = dg_quant_entry(rec.quality, tid >> 6, tid & 63);
        qt[tid >> 6][tid & 63] = t;
        qr[tid >> 6][tid & 63] = dg_quant_rcp(t);
    }

    // ---- 1. fp32 -> bytes, the tile and its halo; a coordinate outside the image reads the nearest pixel inside ----
    // Every loop below walks the full tile with constant divisors and skips what a partial tile lacks (no integer division by a
    // run-time size).  Here all of a lane's loads are issued before the first is used: one memory latency per tile, not 17.
    {
        const int nr = th + 2 * DG_HALO, nc = tw + 2 * DG_HALO;
        constexpr int ITERS = (3 * DG_WIN * DG_WIN + DG_THREADS - 1) / DG_THREADS;
        float v[ITERS];
#pragma unroll
        for (int k = 0; k < ITERS; ++k) {
            const int i = tid + k * DG_THREADS, c = i % DG_WIN, rc = i / DG_WIN, r = rc % DG_WIN, ch = rc / DG_WIN;
            const int gy = min(max(ty0 - DG_HALO + r, 0), H - 1), gx = min(max(tx0 - DG_HALO + c, 0), W - 1);
            v[k] = (ch < 3 && r < nr && c < nc) ? src[ch * plane + (size_t)gy * W + gx] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < ITERS; ++k) {
            const int i = tid + k * DG_THREADS, c = i % DG_WIN, rc = i / DG_WIN, r = rc % DG_WIN, ch = rc / DG_WIN;
            if (ch >= 3 || r >= nr || c >= nc) continue;
            const float q = floorf(__fadd_rn(__fmul_rn(v[k], 255.0f), 0.5f));      // two roundings, as the definition says: no fma
            win[(ch * DG_WIN + r) * DG_WS + c] = (uint8_t)(int)fminf(fmaxf(q, 0.0f), 255.0f);
        }
    }
    __syncthreads();

    // ---- 2a. the horizontal pass over every window row: a lane makes 4 neighbouring bytes from the 10 around them (3 dwords) ----
    {
        const int nr = th + 2 * DG_HALO;
        for (int i = tid; i < 3 * DG_WIN * DG_QUADS; i += DG_THREADS) {
            const int q = i % DG_QUADS, rc = i / DG_QUADS, r = rc % DG_WIN, ch = rc / DG_WIN;
            if (r >= nr || 4 * q >= tw) continue;
            // window columns 4 q .. 4 q + 11 (taps reach 4 q + 9); the row's pitch of 40 covers them for every q.  Past the image's
            // share of a partial tile the bytes are whatever LDS held: they only reach outputs at x >= tw, which nothing reads.
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(win + (ch * DG_WIN + r) * DG_WS + 4 * q);
            const uint32_t w[3] = {sp[0], sp[1], sp[2]};
            int bt[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) bt[j] = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
            uint32_t o = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) o |= (uint32_t)dg_blur7(rec.taps, bt[e], bt[e + 1], bt[e + 2], bt[e + 3], bt[e + 4], bt[e + 5], bt[e + 6]) << (8 * e);
            *reinterpret_cast<uint32_t*>(hpass + (ch * DG_WIN + r) * DG_TILE + 4 * q) = o;
        }
    }
    __syncthreads();

    // ---- 2b. the vertical pass, then the noise: bytes [ch][y][x] at the window's pitch; 4 neighbouring columns a lane ----
    for (int i = tid; i < 3 * DG_TILE * DG_QUADS; i += DG_THREADS) {
        const int q = i % DG_QUADS, rc = i / DG_QUADS, y = rc % DG_TILE, ch = rc / DG_TILE;
        if (y >= th || 4 * q >= tw) continue;
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(hpass + (ch * DG_WIN + y) * DG_TILE + 4 * q);      // rows y .. y + 6
        uint32_t w[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) w[j] = sp[j * (DG_TILE / 4)];
        uint32_t o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int sh = 8 * e;
            int u = dg_blur7(rec.taps, (int)((w[0] >> sh) & 255u), (int)((w[1] >> sh) & 255u), (int)((w[2] >> sh) & 255u), (int)((w[3] >> sh) & 255u),
                             (int)((w[4] >> sh) & 255u), (int)((w[5] >> sh) & 255u), (int)((w[6] >> sh) & 255u));
            if (rec.noise_amp != 0) {
                const uint32_t pix = (uint32_t)(ty0 + y) * (uint32_t)W + (uint32_t)(tx0 + 4 * q + e);
                const uint32_t h = drop_hash(rec.noise_seed, (rec.flags & 1) ? pix : pix * 3u + (uint32_t)ch);
                const int n = (int)(h & 255u) + (int)((h >> 8) & 255u) + (int)((h >> 16) & 255u) + (int)(h >> 24) - 510;
                u = dg_clip255(u + ((n * rec.noise_amp + (1 << 15)) >> 16));
            }
            o |= (uint32_t)u << sh;
        }
        *reinterpret_cast<uint32_t*>(win + (ch * DG_WIN + y) * DG_WS + 4 * q) = o;
    }
    __syncthreads();

    if (jpeg) {
        const int tw8 = (tw + 7) & ~7, th8 = (th + 7) & ~7;
        // ---- 3. RGB -> YCbCr - 128, the last column / row replicated into the blocks that leave the image ----
        for (int i = tid; i < DG_TILE * DG_TILE; i += DG_THREADS) {
            const int x = i % DG_TILE, y = i / DG_TILE;
            if (y >= th8 || x >= tw8) continue;
            const uint8_t* sp = win + min(y, th - 1) * DG_WS + min(x, tw - 1);
            const int R = sp[0], G = sp[DG_WIN * DG_WS], B = sp[2 * DG_WIN * DG_WS];
            int* d = pl + y * DG_PS + x;
            int Y, Cb, Cr;
            dg_rgb_to_ycc(R, G, B, Y, Cb, Cr);
            d[0] = Y - 128;
            d[DG_TILE * DG_PS] = Cb - 128;
            d[2 * DG_TILE * DG_PS] = Cr - 128;
        }
        __syncthreads();

        // ---- 4a. forward DCT, rows: a lane per (channel, row, block column) ----
        for (int i = tid; i < 3 * DG_TILE * 4; i += DG_THREADS) {
            const int bx = i & 3, r = (i >> 2) & 31, ch = i >> 7;
            if (r >= th8 || bx * 8 >= tw8) continue;
            int* p = pl + (ch * DG_TILE + r) * DG_PS + bx * 8;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k];
            dg_fdct8<true>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k] = d[k];
        }
        __syncthreads();

        // ---- 4b. forward DCT, columns; quantise, dequantise; inverse DCT, columns: a lane per (channel, block row, column) ----
        for (int i = tid; i < 3 * 4 * DG_TILE; i += DG_THREADS) {
            const int x = i & 31, by = (i >> 5) & 3, ch = i >> 7;
            if (x >= tw8 || by * 8 >= th8) continue;
            int* p = pl + (ch * DG_TILE + by * 8) * DG_PS + x;
            const int* t = qt[ch ? 1 : 0] + (x & 7);
            const uint32_t* rcp = qr[ch ? 1 : 0] + (x & 7);
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k * DG_PS];
            dg_fdct8<false>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                // sign(c) ((|c| + 4 t) / (8 t)) t
                const int tk = t[k * 8];
                const int q = dg_quant_div(d[k], tk, rcp[k * 8]) * tk;
                d[k] = d[k] < 0 ? -q : q;
            }
            dg_idct8<true>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k * DG_PS] = d[k];
        }
        __syncthreads();

        // ---- 4c. inverse DCT, rows; back to 0..255 ----
        for (int i = tid; i < 3 * DG_TILE * 4; i += DG_THREADS) {
            const int bx = i & 3, r = (i >> 2) & 31, ch = i >> 7;
            if (r >= th8 || bx * 8 >= tw8) continue;
            int* p = pl + (ch * DG_TILE + r) * DG_PS + bx * 8;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k];
            dg_idct8<false>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k] = dg_clip255(d[k] + 128);
        }
        __syncthreads();

        // ---- 5a. YCbCr -> RGB, into the byte tile (a pixel has one lane: in place) ----
        for (int i = tid; i < DG_TILE * DG_TILE; i += DG_THREADS) {
            const int x = i % DG_TILE, y = i / DG_TILE;
            if (y >= th || x >= tw) continue;
            const int* s = pl + y * DG_PS + x;
            const int Y = s[0], cb = s[DG_TILE * DG_PS] - 128, cr = s[2 * DG_TILE * DG_PS] - 128;
            uint8_t* d = win + y * DG_WS + x;
            d[0] = (uint8_t)dg_clip255(Y + ((dg_fix(1.402) * cr + 32768) >> 16));
            d[DG_WIN * DG_WS] = (uint8_t)dg_clip255(Y + ((-dg_fix(.34414) * cb + 32768 - dg_fix(.71414) * cr) >> 16));
            d[2 * DG_WIN * DG_WS] = (uint8_t)dg_clip255(Y + ((dg_fix(1.772) * cb + 32768) >> 16));
        }
        __syncthreads();
    }

    // ---- 5b. bytes -> fp32 ----
    float* dst = out + (size_t)b * 3 * plane;
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {               // tx0 and tw are multiples of 4 then
        for (int i = tid; i < 3 * DG_TILE * DG_QUADS; i += DG_THREADS) {
            const int q = i % DG_QUADS, rc = i / DG_QUADS, y = rc % DG_TILE, ch = rc / DG_TILE;
            if (y >= th || 4 * q >= tw) continue;
            const uint32_t w = *reinterpret_cast<const uint32_t*>(win + (ch * DG_WIN + y) * DG_WS + 4 * q);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (float)((w >> (8 * j)) & 255u) / 255.0f;
            *reinterpret_cast<f32x4*>(dst + ch * plane + (size_t)(ty0 + y) * W + tx0 + 4 * q) = o;
        }
    } else {
        for (int i = tid; i < 3 * DG_TILE * DG_TILE; i += DG_THREADS) {
            const int x = i % DG_TILE, rc = i / DG_TILE, y = rc % DG_TILE, ch = rc / DG_TILE;
            if (y >= th || x >= tw) continue;
            dst[ch * plane + (size_t)(ty0 + y) * W + tx0 + x] = (float)win[(ch * DG_WIN + y) * DG_WS + x] / 255.0f;
        }
    }
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
