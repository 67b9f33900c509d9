// The stages of the training degradations that degrade.hip (4:4:4) and degrade420.hip (4:2:0 beside 4:4:4) run on a workgroup's byte
// tiles in LDS: staging, the two blur passes with the noise, the 4:4:4 JPEG round trip of a 32 x 32 tile, and the store.
// A workgroup owns one 32 x 32 output tile; the bytes it stages, blurs and noises are a REG x REG pixel region around it plus the
// 3-pixel blur halo: REG = 32, the tile itself, for 4:4:4; REG = 64, the tile's 2 x 2 MCUs and one ring of MCUs, for 4:2:0.
#pragma once
#include "common.h"
#include "jpeg_dct.h"      // colour conversion, both DCTs, tables and quantiser: shared with jpeg_encode.hip and jpeg_decode.hip

struct DegradeRec {
    int taps[4];
    int noise_amp;
    uint32_t noise_seed;
    int quality, flags;
};

namespace {
constexpr int DG_TILE = 32;                        // tile side: a multiple of the 8 x 8 JPEG block
constexpr int DG_HALO = 3;                         // blur radius
constexpr int DG_PS = DG_TILE + 1;                 // word pitch of an int tile row (degrade.hip says why)
constexpr int DG_PRECISION_BITS = 32 - 8 - 2;      // Pillow's PRECISION_BITS for 8-bit images
constexpr int DG_THREADS = 256;

template <int REG>
struct DgWindow {
    static constexpr int WIN = REG + 2 * DG_HALO;  // 38 / 70: rows and columns of the window
    static constexpr int WS = WIN + 2;             // 40 / 72: byte pitch of a window row; the horizontal pass reads 12 bytes from column REG - 4
    static constexpr int QUADS = REG / 4;          // 4-byte groups of a region row
    static constexpr int WIN_BYTES = 3 * WIN * WS, HPASS_BYTES = 3 * WIN * REG;
    static_assert(WS % 4 == 0 && WS >= REG + 8 && REG % 16 == 0, "dword reads of a window row stay inside its pitch");
};

// Where a region lies in the image, and the part of it that is worked on: rows [r0, r1) and columns [c0, c1) of the region, all
// inside the image (c0 a multiple of 4).  The 4:4:4 tile has x0 = tx0, y0 = ty0, r0 = c0 = 0, r1 = th, c1 = tw.
struct DgBox {
    int x0, y0, r0, r1, c0, c1;
};

// one output of a blur pass from its seven inputs, rounded to a byte as Pillow's resampler does
TUP_DEVICE int dg_blur7(const int (&k)[4], int a0, int a1, int a2, int a3, int a4, int a5, int a6)
{
    const int s = ((1 << (DG_PRECISION_BITS - 1)) + k[0] * a3 + k[1] * (a2 + a4) + k[2] * (a1 + a5) + k[3] * (a0 + a6)) >> DG_PRECISION_BITS;
    // The shift and the clip stay two instructions.  Left to itself hipcc (clang 22, ROCm 7.2) joins two neighbouring results into one
    // v_ashr_pk_u8_i32 and ORs the other two bytes of the dword on top of it as if the instruction had cleared bits 16-31 of its
    // destination; it leaves them as they were, and the stale bits came out in bytes 2 and 3 of every dword of the horizontal pass.
    return dg_clip255((int)opaque_copy((uint32_t)s));
}

// ---- 1. fp32 -> bytes, the box and its halo into win [ch][WIN][WS]; a coordinate outside the image reads the nearest pixel inside ----
// Every loop below walks the full region with constant divisors and skips what the box lacks (no integer division by a run-time
// size).  Here a lane issues 17 loads before it uses the first: one memory latency per 17 elements, and per tile at REG = 32.
template <int REG>
TUP_DEVICE void dg_stage(const float* __restrict__ src, size_t plane, int H, int W, const DgBox& box, uint8_t* win, int tid)
{
    using G = DgWindow<REG>;
    constexpr int CHUNK = 17, ITERS = (3 * G::WIN * G::WIN + DG_THREADS - 1) / DG_THREADS;
    const int nr = box.r1 + 2 * DG_HALO, nc = box.c1 + 2 * DG_HALO;
    for (int k0 = 0; k0 < ITERS; k0 += CHUNK) {
        float v[CHUNK];
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            const int i = tid + (k0 + k) * DG_THREADS, c = i % G::WIN, rc = i / G::WIN, r = rc % G::WIN, ch = rc / G::WIN;
            const int gy = min(max(box.y0 - DG_HALO + r, 0), H - 1), gx = min(max(box.x0 - DG_HALO + c, 0), W - 1);
            v[k] = (ch < 3 && r >= box.r0 && r < nr && c >= box.c0 && c < nc) ? src[ch * plane + (size_t)gy * W + gx] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            const int i = tid + (k0 + k) * DG_THREADS, c = i % G::WIN, rc = i / G::WIN, r = rc % G::WIN, ch = rc / G::WIN;
            if (ch >= 3 || r < box.r0 || r >= nr || c < box.c0 || c >= nc) continue;
            const float q = floorf(__fadd_rn(__fmul_rn(v[k], 255.0f), 0.5f));      // two roundings, as the definition says: no fma
            win[(ch * G::WIN + r) * G::WS + c] = (uint8_t)(int)fminf(fmaxf(q, 0.0f), 255.0f);
        }
    }
}

// ---- 2a. the horizontal pass over every window row of the box: a lane makes 4 neighbouring bytes from the 10 around them (3 dwords) ----
template <int REG>
TUP_DEVICE void dg_blur_rows(const int (&taps)[4], const DgBox& box, const uint8_t* win, uint8_t* hpass, int tid)
{
    using G = DgWindow<REG>;
    const int nr = box.r1 + 2 * DG_HALO;
    for (int i = tid; i < 3 * G::WIN * G::QUADS; i += DG_THREADS) {
        const int q = i % G::QUADS, rc = i / G::QUADS, r = rc % G::WIN, ch = rc / G::WIN;
        if (r < box.r0 || r >= nr || 4 * q < box.c0 || 4 * q >= box.c1) continue;
        // window columns 4 q .. 4 q + 11 (taps reach 4 q + 9); the row's pitch covers them for every q.  Past the image's share of a
        // partial box the bytes are whatever LDS held: they only reach outputs at columns >= c1, which nothing reads.
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(win + (ch * G::WIN + r) * G::WS + 4 * q);
        const uint32_t w[3] = {sp[0], sp[1], sp[2]};
        int bt[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) bt[j] = (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
        uint32_t o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) o |= (uint32_t)dg_blur7(taps, bt[e], bt[e + 1], bt[e + 2], bt[e + 3], bt[e + 4], bt[e + 5], bt[e + 6]) << (8 * e);
        *reinterpret_cast<uint32_t*>(hpass + (ch * G::WIN + r) * REG + 4 * q) = o;
    }
}

// ---- 2b. the vertical pass, then the noise: bytes [ch][y][x] of the region at the window's pitch; 4 neighbouring columns a lane ----
// The noise index is the pixel's absolute index in the image.
template <int REG>
TUP_DEVICE void dg_blur_cols_noise(const DegradeRec& rec, int W, const DgBox& box, const uint8_t* hpass, uint8_t* win, int tid)
{
    using G = DgWindow<REG>;
    for (int i = tid; i < 3 * REG * G::QUADS; i += DG_THREADS) {
        const int q = i % G::QUADS, rc = i / G::QUADS, y = rc % REG, ch = rc / REG;
        if (y < box.r0 || y >= box.r1 || 4 * q < box.c0 || 4 * q >= box.c1) continue;
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(hpass + (ch * G::WIN + y) * REG + 4 * q);      // rows y .. y + 6
        uint32_t w[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) w[j] = sp[j * (REG / 4)];
        uint32_t o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int sh = 8 * e;
            int u = dg_blur7(rec.taps, (int)((w[0] >> sh) & 255u), (int)((w[1] >> sh) & 255u), (int)((w[2] >> sh) & 255u), (int)((w[3] >> sh) & 255u),
                             (int)((w[4] >> sh) & 255u), (int)((w[5] >> sh) & 255u), (int)((w[6] >> sh) & 255u));
            if (rec.noise_amp != 0) {
                const uint32_t pix = (uint32_t)(box.y0 + y) * (uint32_t)W + (uint32_t)(box.x0 + 4 * q + e);
                const uint32_t h = drop_hash(rec.noise_seed, (rec.flags & 1) ? pix : pix * 3u + (uint32_t)ch);
                const int n = (int)(h & 255u) + (int)((h >> 8) & 255u) + (int)((h >> 16) & 255u) + (int)(h >> 24) - 510;
                u = dg_clip255(u + ((n * rec.noise_amp + (1 << 15)) >> 16));
            }
            o |= (uint32_t)u << sh;
        }
        *reinterpret_cast<uint32_t*>(win + (ch * G::WIN + y) * G::WS + 4 * q) = o;
    }
}

// the quantiser tables of a quality into LDS: qt = luma, chroma; qr = floor(2^32 / (8 t)) + 1
TUP_DEVICE void dg_load_tables(int quality, int (&qt)[2][64], uint32_t (&qr)[2][64], int tid)
{
    if (tid < 128) {
        const int t = dg_quant_entry(quality, tid >> 6, tid & 63);
        qt[tid >> 6][tid & 63] = t;
        qr[tid >> 6][tid & 63] = dg_quant_rcp(t);
    }
}

// ---- 4. the DCT round trip of the blocks of pl [3][32][33] for which `live(ch, block row, block column)` holds, in place: row DCT (a
// lane per row of a block), then column DCT + quantise + dequantise + column IDCT in registers (a lane per column of a block), then
// row IDCT and back to 0..255.  Starts and ends on a barrier. ----
template <typename Live>
TUP_DEVICE void dg_dct_roundtrip(int* pl, const int (&qt)[2][64], const uint32_t (&qr)[2][64], int tid, Live live)
{
    __syncthreads();
    // 4a. forward DCT, rows: a lane per (channel, row, block column)
    for (int i = tid; i < 3 * DG_TILE * 4; i += DG_THREADS) {
        const int bx = i & 3, r = (i >> 2) & 31, ch = i >> 7;
        if (!live(ch, r >> 3, bx)) continue;
        int* p = pl + (ch * DG_TILE + r) * DG_PS + bx * 8;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        dg_fdct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = d[k];
    }
    __syncthreads();

    // 4b. forward DCT, columns; quantise, dequantise; inverse DCT, columns: a lane per (channel, block row, column)
    for (int i = tid; i < 3 * 4 * DG_TILE; i += DG_THREADS) {
        const int x = i & 31, by = (i >> 5) & 3, ch = i >> 7;
        if (!live(ch, by, x >> 3)) continue;
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

    // 4c. inverse DCT, rows; back to 0..255
    for (int i = tid; i < 3 * DG_TILE * 4; i += DG_THREADS) {
        const int bx = i & 3, r = (i >> 2) & 31, ch = i >> 7;
        if (!live(ch, r >> 3, bx)) continue;
        int* p = pl + (ch * DG_TILE + r) * DG_PS + bx * 8;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        dg_idct8<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = dg_clip255(d[k] + 128);
    }
    __syncthreads();
}

TUP_DEVICE void dg_ycc_to_rgb(int Y, int Cb, int Cr, uint8_t* d, int plane_bytes)
{
    const int cb = Cb - 128, cr = Cr - 128;
    d[0] = (uint8_t)dg_clip255(Y + ((dg_fix(1.402) * cr + 32768) >> 16));
    d[plane_bytes] = (uint8_t)dg_clip255(Y + ((-dg_fix(.34414) * cb + 32768 - dg_fix(.71414) * cr) >> 16));
    d[2 * plane_bytes] = (uint8_t)dg_clip255(Y + ((dg_fix(1.772) * cb + 32768) >> 16));
}

// ---- 3-5a. the 4:4:4 round trip of a tile of tw x th pixels: the bytes of win [ch][38][40] after blur and noise, and back into them.
// A tile never shares a block with its neighbour: the block grid starts at the image's origin.  Ends on a barrier. ----
TUP_DEVICE void dg_jpeg444(uint8_t* win, int* pl, const int (&qt)[2][64], const uint32_t (&qr)[2][64], int tw, int th, int tid)
{
    using G = DgWindow<DG_TILE>;
    const int tw8 = (tw + 7) & ~7, th8 = (th + 7) & ~7;
    // 3. RGB -> YCbCr - 128, the last column / row replicated into the blocks that leave the image
    for (int i = tid; i < DG_TILE * DG_TILE; i += DG_THREADS) {
        const int x = i % DG_TILE, y = i / DG_TILE;
        if (y >= th8 || x >= tw8) continue;
        const uint8_t* sp = win + min(y, th - 1) * G::WS + min(x, tw - 1);
        const int R = sp[0], G_ = sp[G::WIN * G::WS], B = sp[2 * G::WIN * G::WS];
        int* d = pl + y * DG_PS + x;
        int Y, Cb, Cr;
        dg_rgb_to_ycc(R, G_, B, Y, Cb, Cr);
        d[0] = Y - 128;
        d[DG_TILE * DG_PS] = Cb - 128;
        d[2 * DG_TILE * DG_PS] = Cr - 128;
    }
    dg_dct_roundtrip(pl, qt, qr, tid, [=](int, int by, int bx) { return by * 8 < th8 && bx * 8 < tw8; });
    // 5a. YCbCr -> RGB, into the byte tile (a pixel has one lane: in place)
    for (int i = tid; i < DG_TILE * DG_TILE; i += DG_THREADS) {
        const int x = i % DG_TILE, y = i / DG_TILE;
        if (y >= th || x >= tw) continue;
        const int* s = pl + y * DG_PS + x;
        dg_ycc_to_rgb(s[0], s[DG_TILE * DG_PS], s[2 * DG_TILE * DG_PS], win + y * G::WS + x, G::WIN * G::WS);
    }
    __syncthreads();
}

// ---- 5b. bytes -> fp32: the tile's bytes are rows 0 .. th and columns 0 .. tw of win [ch][WIN][WS]; 16 bytes per store where the
// width and the base allow it ----
template <int REG>
TUP_DEVICE void dg_store(const uint8_t* win, float* __restrict__ dst, bool wide, size_t plane, int W, int tx0, int ty0, int tw, int th, int tid)
{
    using G = DgWindow<REG>;
    constexpr int TQ = DG_TILE / 4;
    if (wide) {                                                                     // tx0 and tw are multiples of 4 then
        for (int i = tid; i < 3 * DG_TILE * TQ; i += DG_THREADS) {
            const int q = i % TQ, rc = i / TQ, y = rc % DG_TILE, ch = rc / DG_TILE;
            if (y >= th || 4 * q >= tw) continue;
            const uint32_t w = *reinterpret_cast<const uint32_t*>(win + (ch * G::WIN + y) * G::WS + 4 * q);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (float)((w >> (8 * j)) & 255u) / 255.0f;
            *reinterpret_cast<f32x4*>(dst + ch * plane + (size_t)(ty0 + y) * W + tx0 + 4 * q) = o;
        }
    } else {
        for (int i = tid; i < 3 * DG_TILE * DG_TILE; i += DG_THREADS) {
            const int x = i % DG_TILE, rc = i / DG_TILE, y = rc % DG_TILE, ch = rc / DG_TILE;
            if (y >= th || x >= tw) continue;
            dst[ch * plane + (size_t)(ty0 + y) * W + tx0 + x] = (float)win[(ch * G::WIN + y) * G::WS + x] / 255.0f;
        }
    }
}
}  // namespace
