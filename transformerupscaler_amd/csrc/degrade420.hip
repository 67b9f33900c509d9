// Training degradations whose JPEG round trip is 4:2:0 for the samples that ask for it (record flags & 4) and 4:4:4 for the rest, a
// whole batch in one launch (ops.degrade).  The stages are degrade.hip's (degrade_stages.h); what 4:2:0 adds per sample is
// jpeg_420.h, stated in numpy in tests/_degrade420_ref.py and pinned there to Pillow's subsampling=2 round trip.
//
// A workgroup owns one 32 x 32 output tile of one sample, so the sampling is uniform per workgroup.  Without the flag it runs exactly
// the stages of degrade_lr_kernel on the same tiles: those samples come out bit for bit as tup_degrade_lr writes them.  With it, an
// output pixel needs the chroma samples at (x >> 1) +- 1, (y >> 1) +- 1, each from the inverse DCT of an 8 x 8 chroma block that
// covers a 16 x 16 pixel MCU, which must be blurred, noised, converted, downsampled, transformed and quantised whole.  So the
// workgroup works on the 64 x 64 pixel region around its tile, the tile's 2 x 2 MCUs and one ring of MCUs (4 x 4 chroma blocks):
//   1-2. stages, blurs and noises the part of the region inside the image, with the 3-pixel halo: byte tiles [3][70][72] and [3][70][64]
//        (15 KB + 13 KB).  The noise index is the absolute pixel index, so a ring pixel gets the value its own tile gives it;
//   3.   plane 0 of the int tile [3][32][33] <- the luma of the inner tile, as at 4:4:4; planes 1 and 2 <- the downsampled Cb and Cr of
//        the region, 32 x 32 samples, padding by replication of the bytes after the noise (jpeg_420.h has the rules);
//   4.   the four DCT passes, unchanged, over the luma blocks the tile has and the chroma blocks whose MCU is inside the image;
//   5.   luma and the triangle-filtered chroma (rows and columns 8..23 of planes 1 and 2 and their +-1 neighbours, indices clamped to
//        the real samples; plain replication for images at most 4 pixels wide) -> RGB bytes -> fp32.
// Ring MCUs wholly outside the image are never touched.  No intermediate reaches memory; every output has one writer and the launch
// uses no workspace.  LDS: 42 KB a workgroup, three workgroups a CU.
#include "degrade_stages.h"
#include "jpeg_420.h"

namespace {
constexpr int D4_REG = 2 * DG_TILE;                // the region's side
constexpr int D4_RING = 16;                        // one MCU on every side of the tile
constexpr int D4_FLAG = 4;                         // record flags & 4: this sample's round trip is 4:2:0

__global__ __launch_bounds__(DG_THREADS) void degrade_sub_kernel(const float* __restrict__ in, const DegradeRec* __restrict__ recs,
                                                                int H, int W, float* __restrict__ out)
{
    using G1 = DgWindow<DG_TILE>;
    using G4 = DgWindow<D4_REG>;
    static_assert(G1::WIN_BYTES <= G4::WIN_BYTES && G1::HPASS_BYTES <= G4::HPASS_BYTES, "the 4:4:4 tiles fit in the 4:2:0 ones");
    __shared__ __attribute__((aligned(16))) uint8_t win[G4::WIN_BYTES];           // [ch][70][72], or [ch][38][40] without the flag
    __shared__ __attribute__((aligned(16))) uint8_t hpass[G4::HPASS_BYTES];       // [ch][70][64], or [ch][38][32]
    __shared__ int pl[3 * DG_TILE * DG_PS];                                       // [ch][32][33]
    __shared__ int qt[2][64];
    __shared__ uint32_t qr[2][64];

    const int b = blockIdx.y, tid = threadIdx.x;
    const DegradeRec rec = recs[b];
    const int ntx = (W + DG_TILE - 1) / DG_TILE;
    const int tx0 = (blockIdx.x % ntx) * DG_TILE, ty0 = (blockIdx.x / ntx) * DG_TILE;
    const int tw = min(DG_TILE, W - tx0), th = min(DG_TILE, H - ty0);
    const size_t plane = (size_t)H * W;
    const float* src = in + (size_t)b * 3 * plane;
    float* dst = out + (size_t)b * 3 * plane;
    const bool jpeg = rec.quality >= 1 && rec.quality <= 100;
    const bool wide = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;

    if (jpeg) dg_load_tables(rec.quality, qt, qr, tid);

    if (!(jpeg && (rec.flags & D4_FLAG))) {            // the same for every lane of the workgroup: degrade_lr_kernel's sequence
        const DgBox box = {tx0, ty0, 0, th, 0, tw};
        dg_stage<DG_TILE>(src, plane, H, W, box, win, tid);
        __syncthreads();
        dg_blur_rows<DG_TILE>(rec.taps, box, win, hpass, tid);
        __syncthreads();
        dg_blur_cols_noise<DG_TILE>(rec, W, box, hpass, win, tid);
        __syncthreads();
        if (jpeg) dg_jpeg444(win, pl, qt, qr, tw, th, tid);
        dg_store<DG_TILE>(win, dst, wide, plane, W, tx0, ty0, tw, th, tid);
        return;
    }

    // the region starts one MCU before the tile (outside the image for the first tile of a row or column: that ring is not worked on)
    const int rx0 = tx0 - D4_RING, ry0 = ty0 - D4_RING;
    const DgBox box = {rx0, ry0, ty0 ? 0 : D4_RING, min(D4_REG, H - ry0), tx0 ? 0 : D4_RING, min(D4_REG, W - rx0)};
    dg_stage<D4_REG>(src, plane, H, W, box, win, tid);
    __syncthreads();
    dg_blur_rows<D4_REG>(rec.taps, box, win, hpass, tid);
    __syncthreads();
    dg_blur_cols_noise<D4_REG>(rec, W, box, hpass, win, tid);
    __syncthreads();

    constexpr int WP = G4::WIN * G4::WS;               // bytes of a channel of win
    const int tw8 = (tw + 7) & ~7, th8 = (th + 7) & ~7;
    const int mcu_x0 = (tx0 >> 4) - 1, mcu_y0 = (ty0 >> 4) - 1, mw = (W + 15) >> 4, mh = (H + 15) >> 4;      // the region's first MCU; MCUs across / down
    const int ccx0 = 8 * mcu_x0, ccy0 = 8 * mcu_y0;                                                       // ... and its first chroma sample
    // luma: the blocks the tile has pixels in; chroma: the region's blocks whose MCU lies (partly) inside the image
    const auto live = [=](int ch, int by, int bx) {
        if (ch == 0) return by * 8 < th8 && bx * 8 < tw8;
        return mcu_y0 + by >= 0 && mcu_y0 + by < mh && mcu_x0 + bx >= 0 && mcu_x0 + bx < mw;
    };

    // ---- 3. luma - 128 of the tile, the last column / row replicated into the blocks that leave the image; Cb - 128 and Cr - 128 of
    // the region after the h2v2 downsample ----
    for (int i = tid; i < DG_TILE * DG_TILE; i += DG_THREADS) {
        const int x = i % DG_TILE, y = i / DG_TILE;
        if (y < th8 && x < tw8) {
            const uint8_t* sp = win + (D4_RING + min(y, th - 1)) * G4::WS + D4_RING + min(x, tw - 1);
            int Y, Cb, Cr;
            dg_rgb_to_ycc(sp[0], sp[WP], sp[2 * WP], Y, Cb, Cr);
            pl[y * DG_PS + x] = Y - 128;
        }
        if (live(1, y >> 3, x >> 3)) {                 // (y, x) is a chroma sample of the region here
            const J420Src s = j420_down_src(ccy0 + y, ccx0 + x, H, W);
            int cb[4], cr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* sp = win + (((k >> 1) ? s.y1 : s.y0) - ry0) * G4::WS + ((k & 1) ? s.x1 : s.x0) - rx0;
                int Y;
                dg_rgb_to_ycc(sp[0], sp[WP], sp[2 * WP], Y, cb[k], cr[k]);
            }
            pl[(DG_TILE + y) * DG_PS + x] = j420_down(cb[0], cb[1], cb[2], cb[3], ccx0 + x) - 128;
            pl[(2 * DG_TILE + y) * DG_PS + x] = j420_down(cr[0], cr[1], cr[2], cr[3], ccx0 + x) - 128;
        }
    }
    // ---- 4. the DCT round trip of the live blocks ----
    dg_dct_roundtrip(pl, qt, qr, tid, live);

    // ---- 5a. luma and upsampled chroma -> RGB, into the byte tile (rows and columns 0.. of win: nothing reads its old bytes any more) ----
    const bool narrow = j420_narrow(W);
    for (int i = tid; i < DG_TILE * DG_TILE; i += DG_THREADS) {
        const int x = i % DG_TILE, y = i / DG_TILE;
        if (y >= th || x >= tw) continue;
        const J420Taps t = j420_up_src(ty0 + y, tx0 + x, H, W);
        const int* c = pl + DG_TILE * DG_PS;           // Cb; Cr is a plane further
        const int oo = (t.cy - ccy0) * DG_PS + t.cx - ccx0, no = (t.ny - ccy0) * DG_PS + t.cx - ccx0;
        const int on = (t.cy - ccy0) * DG_PS + t.nx - ccx0, nn = (t.ny - ccy0) * DG_PS + t.nx - ccx0;
        constexpr int P = DG_TILE * DG_PS;
        const int Cb = narrow ? c[oo] : j420_up(c[oo], c[no], c[on], c[nn], tx0 + x);
        const int Cr = narrow ? c[P + oo] : j420_up(c[P + oo], c[P + no], c[P + on], c[P + nn], tx0 + x);
        dg_ycc_to_rgb(pl[y * DG_PS + x], Cb, Cr, win + y * G4::WS + x, WP);
    }
    __syncthreads();
    dg_store<D4_REG>(win, dst, wide, plane, W, tx0, ty0, tw, th, tid);
}
}  // namespace

// As tup_degrade_lr, for records that may carry flags & 4.
extern "C" int tup_degrade_lr_sub(const float* in, const void* recs, int B, int H, int W, float* out, void* stream)
{
    if (!in || !recs || !out || B <= 0 || H <= 0 || W <= 0 || B > 65535) return (int)hipErrorInvalidValue;
    const long long n = (long long)B * 3 * H * W;
    if (in < out + n && out < in + n) return (int)hipErrorInvalidValue;
    const long long tiles = (long long)((W + DG_TILE - 1) / DG_TILE) * ((H + DG_TILE - 1) / DG_TILE);
    if (tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    degrade_sub_kernel<<<dim3((unsigned)tiles, (unsigned)B), dim3(DG_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        in, (const DegradeRec*)recs, H, W, out);
    TUP_CHECK_LAUNCH();
    return 0;
}
