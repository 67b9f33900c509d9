// TEST INFRASTRUCTURE ONLY -- the self-synchronising index of a JPEG scan without restart markers on the host: the lanes of
// jpeg_sync_index_kernel (transformerupscaler_amd/csrc/jpeg_sync.hip) one after another, each doing what csrc/jpeg_sync.h has a lane
// do, beside the serial walk of the same scan.  tests/test_jpeg_sync_cpu.py builds it with the address and undefined-behaviour
// sanitizers and feeds it good and damaged scans.  As in the kernel a span of 256 subsequences is walked in a copy of its own, exactly
// as long as the window the kernel stages, so a byte read past that window is an error the sanitizer sees.
//
// Input file: int32 H, W, layout, restart interval (0); the 1488-byte image record ops.jpeg_decode uploads (scan_off is not used); the
// scan.  Output, every row as "logical bit, first MCU, three predictors" (or "-" where the row was not placed), the logical bit being
// 8 x (payload bytes before pos) - n:
//   serial status <JE_* code> rows <S> : ...
//   sync status <JE_* code> rounds <sync rounds> subsequences <count> fallback <0 | 1> rows <S> : ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_sync.h"

struct Record {
    int scan_off, scan_len;
    uint8_t td[4], ta[4];
    uint16_t qt[3][64];
    uint8_t huff[4][JE_SPEC_BYTES];
};
static_assert(sizeof(Record) == 1488, "the record of jpeg_decode.hip");

struct Row {
    int pos, acc, n, pred[3], mcu0;                                     // n = -1: not placed
};

static const int LANES = 256;

static long long logical_bit(const uint8_t* scan, int pos, int n)
{
    long long payload = 0;
    for (int i = 0; i < pos; ++payload) i += scan[i] == 0xFF ? 2 : 1;
    return 8 * payload - n;
}

static void print_rows(const uint8_t* scan, const std::vector<Row>& rows)
{
    printf(" rows %d :", (int)rows.size());
    for (const Row& r : rows) {
        if (r.n < 0) printf(" -");
        else printf(" %lld,%d,%d,%d,%d", logical_bit(scan, r.pos, r.n), r.mcu0, r.pred[0], r.pred[1], r.pred[2]);
    }
    printf("\n");
}

// the serial index: jd_serial_index of csrc/jpeg_index.h without its windows
static int serial_index(const uint8_t* scan, int len, const JeTable* tables, const Record& rec, int layout, int mw, int total, std::vector<Row>& rows,
                        const uint8_t* zz)
{
    JeBits bits{scan, 0, len, 0u, 0, 0};
    int pred[3] = {0, 0, 0}, mcu = 0, err = 0;
    for (Row& r : rows) r = Row{0, 0, -1, {0, 0, 0}, 0};
    while (mcu < total) {
        if (mcu % mw == 0) rows[mcu / mw] = Row{bits.pos, (int)bits.acc, bits.n, {pred[0], pred[1], pred[2]}, mcu};
        err = je_mcu(bits, tables, rec.td, rec.ta, layout, pred, nullptr, 0, zz);
        if (err) break;
        ++mcu;
    }
    return err;
}

struct StoreRows {
    std::vector<Row>* rows;
    int w0, before, p0, p1, p2, bpm, mw, total;
    void operator()(const JeBits& b, const JsCount& c) const
    {
        const int mcu = (before + c.blocks) / bpm;
        if (mcu < total && mcu % mw == 0)
            (*rows)[mcu / mw] = Row{w0 + b.pos, (int)b.acc, b.n, {js_pred(p0 + c.d0), js_pred(p1 + c.d1), js_pred(p2 + c.d2)}, mcu};
    }
};

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t tmp[4096];
    for (size_t n; (n = fread(tmp, 1, sizeof tmp, f)) > 0;) file.insert(file.end(), tmp, tmp + n);
    fclose(f);
    if (file.size() < 16 + sizeof(Record)) return 2;
    int head[4];
    Record rec;
    memcpy(head, file.data(), 16);
    memcpy(&rec, file.data() + 16, sizeof rec);
    const int H = head[0], W = head[1], layout = head[2], interval = head[3];
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (layout != 0 && layout != 2 && layout != 4) || interval != 0) return 2;
    const size_t size = file.size() - 16 - sizeof(Record);
    if (rec.scan_len < 0 || (size_t)rec.scan_len != size) return 2;
    const int len = (int)size;
    uint8_t* scan = (uint8_t*)malloc(len ? len : 1);                    // exactly the scan
    memcpy(scan, file.data() + 16 + sizeof(Record), len);

    static const uint8_t zz[64] = JE_ZIGZAG_INIT;
    JeTable* tables = new JeTable[4];
    for (int t = 0; t < 4; ++t)
        if (!je_build(rec.huff[t], tables[t])) return 2;                // (the kernel refuses such an image before either walk)

    const int m = layout == 2 ? 16 : 8, mw = (W + m - 1) / m, mh = (H + m - 1) / m, total = mw * mh, bpm = je_blocks_per_mcu(layout);
    std::vector<Row> serial(mh), sync(mh, Row{0, 0, -1, {0, 0, 0}, 0});
    const int serial_status = serial_index(scan, len, tables, rec, layout, mw, total, serial, zz);
    printf("serial status %d", serial_status);
    print_rows(scan, serial);

    const int span = LANES * JS_BYTES, need = total * bpm;
    JsState first{0, 0};
    int before = 0, p0 = 0, p1 = 0, p2 = 0, turns = 0;
    for (int w0 = 0; w0 < len && first.p >= 0 && before < need; w0 += span) {
        const int wlen = span + JS_SLACK < len - w0 ? span + JS_SLACK : len - w0;
        const int lanes = LANES < (len - w0 + JS_BYTES - 1) / JS_BYTES ? LANES : (len - w0 + JS_BYTES - 1) / JS_BYTES;
        uint8_t* data = (uint8_t*)malloc(wlen);                         // the window, and not a byte more
        memcpy(data, scan + w0, wlen);
        std::vector<JsState> entry(lanes), exit(lanes);
        std::vector<JsCount> cnt(lanes);
        std::vector<int> stop(lanes);
        for (int i = 0; i < lanes; ++i) {
            stop[i] = (i + 1) * JS_BYTES < wlen ? (i + 1) * JS_BYTES : wlen;
            entry[i] = i == 0 ? first : js_assume(data, i * JS_BYTES);
            exit[i] = js_walk(data, wlen, stop[i], entry[i], tables, rec.td, rec.ta, layout, cnt[i], JsNoVisit{});
        }
        bool settled = false;
        for (int r = 0; r < lanes && !settled; ++r) {
            std::vector<JsState> from(entry);
            for (int i = 1; i < lanes; ++i) from[i] = exit[i - 1];     // every exit is read before one is written
            settled = true;
            for (int i = 1; i < lanes; ++i)
                if (!js_same(from[i], entry[i])) {
                    settled = false;
                    entry[i] = from[i];
                    exit[i] = js_walk(data, wlen, stop[i], entry[i], tables, rec.td, rec.ta, layout, cnt[i], JsNoVisit{});
                }
            if (!settled) ++turns;
        }
        if (!settled) { printf("the rounds did not settle\n"); return 3; }
        bool stopped = false;                                           // the confirmed chain met an error: what follows does not count
        for (int i = 0; i < lanes && !stopped; ++i) {
            stopped = cnt[i].err != 0;
            if (js_first_row_block(before, cnt[i].blocks, entry[i], stopped ? JsState{-1, 0} : exit[i], bpm * mw) >= 0) {
                JsCount again;
                js_walk(data, wlen, stop[i], entry[i], tables, rec.td, rec.ta, layout, again, StoreRows{&sync, w0, before, p0, p1, p2, bpm, mw, total});
            }
            before += cnt[i].blocks;
            p0 = (p0 + cnt[i].d0) & 0xFFFF; p1 = (p1 + cnt[i].d1) & 0xFFFF; p2 = (p2 + cnt[i].d2) & 0xFFFF;
        }
        first = stopped ? JsState{-1, 0} : exit[lanes - 1];
        if (first.p >= 0) first.p -= span;
        free(data);
    }
    int status = JE_OK;
    const bool fallback = before < need;
    if (fallback) status = serial_index(scan, len, tables, rec, layout, mw, total, sync, zz);
    printf("sync status %d rounds %d subsequences %d fallback %d", status, turns, (len + JS_BYTES - 1) / JS_BYTES, fallback ? 1 : 0);
    print_rows(scan, sync);
    delete[] tables;
    free(scan);
    return 0;
}
