// What the index kernels of the JPEG decoder share (jpeg_decode.hip: jpeg_index_kernel; jpeg_sync.hip: jpeg_sync_index_kernel; DESIGN
// 7l): the image record the host uploads, the tables of an image in LDS, the segment record, and the serial walk of a scan without
// restart markers, which is launch 1 of such a file by itself and what the self-synchronising index falls back to on a damaged scan.
#pragma once
#include "common.h"
#include "jpeg_dct.h"
#include "jpeg_entropy.h"

// what the host uploads per image (ops._JPEG_DEC_REC packs it)
struct JdImage {
    int scan_off;                       // of the scan in the upload's scan area: a multiple of 16
    int scan_len;                       // bytes between SOS and EOI
    uint8_t td[4], ta[4];               // each component's DC / AC table (0 or 1); entry 3 is not used
    uint16_t qt[3][64];                 // each component's quantisation table, natural order
    uint8_t huff[4][JE_SPEC_BYTES];     // DC 0, DC 1, AC 0, AC 1 as DHT carries them; zeros where the file has none
};

namespace {
constexpr int JD_THREADS = DG_SCAN_THREADS;
constexpr int JD_WINDOW = 8192;                             // bytes of the scan staged at a time
constexpr int JD_SEG = 8;                                   // words of a segment record
static_assert(JD_WINDOW - 16 >= JE_MCU_BYTES, "a window holds at least one MCU, so every chunk moves on");

__constant__ const uint8_t jd_zigzag[64] = JE_ZIGZAG_INIT;

struct JdGeometry {
    int m, bpm, mw, mh, total, S, yw, yh, cw, ch;           // MCU side, blocks per MCU, MCUs across / down / in all, segments, plane sizes
    long long ws;                                           // workspace bytes per image
};
// false for what the decoder refuses: sizes outside 1..65535, a layout other than 0 / 2 / 4, an interval outside 0..65535
inline bool jd_geometry(int H, int W, int layout, int interval, JdGeometry& g)
{
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (layout != 0 && layout != 2 && layout != 4) || interval < 0 || interval > 65535) return false;
    g.m = layout == 2 ? 16 : 8;
    g.bpm = je_blocks_per_mcu(layout);
    g.mw = (W + g.m - 1) / g.m;
    g.mh = (H + g.m - 1) / g.m;
    g.total = g.mw * g.mh;
    g.S = interval ? (g.total + interval - 1) / interval : g.mh;
    g.yw = g.mw * g.m; g.yh = g.mh * g.m;
    g.cw = layout == 4 ? 0 : g.mw * 8; g.ch = layout == 4 ? 0 : g.mh * 8;
    g.ws = (long long)g.yw * g.yh + 2LL * g.cw * g.ch;
    return true;
}

struct JdWalk {                                             // the walker's state between chunks
    int pos, acc, n, hit, pred[3], count, err;
};

struct JdTables {
    JeTable tab[4];
    uint8_t td[4], ta[4];
    uint8_t zz[64];
    int ok[4];
};

// tables, selectors and zigzag of an image into LDS; ends on a barrier.  false (for every lane): a table is no prefix code.
TUP_DEVICE bool jd_load_tables(const JdImage* rec, JdTables& t, int tid)
{
    if (tid < 4) t.ok[tid] = je_build(rec->huff[tid], t.tab[tid]) ? 1 : 0;
    if (tid >= 64 && tid < 68) { t.td[tid - 64] = rec->td[tid - 64]; t.ta[tid - 64] = rec->ta[tid - 64]; }
    if (tid >= 128 && tid < 192) t.zz[tid - 128] = jd_zigzag[tid - 128];
    __syncthreads();
    return (t.ok[0] & t.ok[1] & t.ok[2] & t.ok[3]) != 0;
}

// does the record describe bytes inside the scan area?  (whole 16-byte groups are loaded, so the rounded length counts)
TUP_DEVICE bool jd_record_ok(int off, int len, long long scans_bytes)
{
    return off >= 0 && (off & 15) == 0 && len >= 0 && len <= 0x7fffffff - 15 && (long long)off + ((len + 15) & ~15) <= scans_bytes;
}

// bytes [w0, w0 + 16 * ceil(n / 16)) of the scan -> win; w0 is a multiple of 16
TUP_DEVICE void jd_stage(const uint8_t* __restrict__ scan, int w0, int n, u32x4* win, int tid)
{
    for (int i = tid; i * 16 < n; i += JD_THREADS) win[i] = *reinterpret_cast<const u32x4*>(scan + w0 + i * 16);
}

TUP_DEVICE void jd_store_seg(int* seg, int pos, int end, int acc, int n, int p0, int p1, int p2, int mcu0)
{
    seg[0] = pos; seg[1] = end; seg[2] = acc; seg[3] = n; seg[4] = p0; seg[5] = p1; seg[6] = p2; seg[7] = mcu0;
}

// An image the index does not walk (a table that is no prefix code, a record outside the upload): no segment is placed.
TUP_DEVICE void jd_refuse_image(int* seg, int S, int* status, bool tables_ok, int tid)
{
    for (int k = tid; k < S; k += JD_THREADS) jd_store_seg(seg + (size_t)k * JD_SEG, 0, 0, 0, -1, 0, 0, 0, 0);
    if (tid == 0) *status = tables_ok ? JE_BAD_RECORD : JE_BAD_TABLE;
}

// No restart interval: one walk through the codes by lane 0, the state at the start of every MCU row recorded.  Called by the whole
// workgroup; win: JD_WINDOW bytes of LDS, 16-byte aligned.
TUP_DEVICE void jd_serial_index(const uint8_t* __restrict__ scan, int len, int layout, int mw, int total, int S, int* __restrict__ seg,
                                int* __restrict__ status, const JdTables& tb, uint32_t* win, JdWalk& wk, int tid)
{
    if (tid == 0) { wk.pos = 0; wk.acc = 0; wk.n = 0; wk.hit = 0; wk.pred[0] = wk.pred[1] = wk.pred[2] = 0; wk.count = 0; wk.err = 0; }
    __syncthreads();
    for (int guard = 0; guard <= len / 16 + 1; ++guard) {                           // a window moves on by at least 16 bytes
        const int w0 = wk.pos & ~15, wlen = min(JD_WINDOW, len - w0);
        const bool final = w0 + wlen >= len;
        jd_stage(scan, w0, wlen, reinterpret_cast<u32x4*>(win), tid);
        __syncthreads();
        if (tid == 0) {
            JeBits bits{reinterpret_cast<const uint8_t*>(win), wk.pos - w0, wlen, (uint32_t)wk.acc, wk.n, wk.hit};
            int mcu = wk.count, err = 0;
            while (mcu < total && (final || bits.pos + JE_MCU_BYTES <= wlen)) {
                if (mcu % mw == 0)
                    jd_store_seg(seg + (size_t)(mcu / mw) * JD_SEG, w0 + bits.pos, len, (int)bits.acc, bits.n, wk.pred[0], wk.pred[1], wk.pred[2], mcu);
                err = je_mcu(bits, tb.tab, tb.td, tb.ta, layout, wk.pred, nullptr, 0, tb.zz);
                if (err) break;
                ++mcu;
            }
            if (!err && mcu == wk.count && mcu < total) err = JE_END;               // cannot happen: a window holds an MCU
            wk.pos = w0 + bits.pos; wk.acc = (int)bits.acc; wk.n = bits.n; wk.hit = bits.hit; wk.count = mcu; wk.err = err;
        }
        __syncthreads();
        if (wk.err || wk.count >= total) break;
    }
    const int rows = wk.err ? wk.count / mw + 1 : S;                                 // rows whose start was recorded
    for (int q = rows + tid; q < S; q += JD_THREADS) jd_store_seg(seg + (size_t)q * JD_SEG, 0, 0, 0, -1, 0, 0, 0, 0);
    if (tid == 0) *status = wk.err ? wk.err : (wk.count >= total ? JE_OK : JE_END);
}
}  // namespace
