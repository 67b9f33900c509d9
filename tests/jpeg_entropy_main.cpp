// TEST INFRASTRUCTURE ONLY -- walks one JPEG scan on the host with the bit reader, table builder and block walker the GPU decoder
// runs (transformerupscaler_amd/csrc/jpeg_entropy.h).  tests/test_jpeg_decode_cpu.py builds it with the address and undefined-
// behaviour sanitizers and feeds it good and damaged scans: whatever the bytes, it must end normally.
//
// Input file: int32 H, W, layout, restart interval; the 1488-byte image record ops.jpeg_decode uploads (scan_off is not used); the
// scan.  Output: "status <JE_* code> blocks <walked> checksum <of the coefficients in scan order>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"

struct Record {
    int scan_off, scan_len;
    uint8_t td[4], ta[4];
    uint16_t qt[3][64];
    uint8_t huff[4][JE_SPEC_BYTES];
};
static_assert(sizeof(Record) == 1488, "the record of jpeg_decode.hip");

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
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (layout != 0 && layout != 2 && layout != 4) || interval < 0 || interval > 65535) return 2;
    const size_t len = file.size() - 16 - sizeof(Record);
    if (rec.scan_len < 0 || (size_t)rec.scan_len != len) return 2;
    uint8_t* scan = (uint8_t*)malloc(len ? len : 1);                     // exactly the scan: a byte read past it is an error the sanitizer sees
    memcpy(scan, file.data() + 16 + sizeof(Record), len);

    static const uint8_t zz[64] = JE_ZIGZAG_INIT;
    JeTable* tables = new JeTable[4];
    int status = JE_OK;
    for (int t = 0; t < 4; ++t)
        if (!je_build(rec.huff[t], tables[t])) status = JE_BAD_TABLE;

    const int m = layout == 2 ? 16 : 8, mw = (W + m - 1) / m, mh = (H + m - 1) / m, total = mw * mh, bpm = je_blocks_per_mcu(layout);
    // the segments: [start, end) of the bytes between restart markers, or the whole scan
    std::vector<int> starts{0}, ends;
    if (interval > 0)
        for (size_t i = 1; i < len; ++i)
            if (scan[i - 1] == 0xFF && scan[i] >= 0xD0 && scan[i] <= 0xD7) { ends.push_back((int)i - 1); starts.push_back((int)i + 1); }
    ends.push_back((int)len);
    const int S = interval ? (total + interval - 1) / interval : 1;
    if (status == JE_OK && (int)starts.size() != S) status = JE_RESTARTS;

    uint32_t checksum = 0;
    long long blocks = 0;
    for (int s = 0; s < S && s < (int)starts.size() && status != JE_BAD_TABLE; ++s) {
        JeBits bits{scan, starts[s], ends[s], 0u, 0, 0};
        int pred[3] = {0, 0, 0};
        const int first = interval ? s * interval : 0, count = interval ? (interval < total - first ? interval : total - first) : total;
        for (int i = 0; i < count; ++i) {
            int coef[6 * 64] = {0};
            const int err = je_mcu(bits, tables, rec.td, rec.ta, layout, pred, coef, 64, zz);
            if (err) {
                if (status == JE_OK) status = err;
                break;
            }
            for (int k = 0; k < bpm * 64; ++k) checksum = checksum * 1000003u + ((uint32_t)coef[k] & 0xFFFFu);
            blocks += bpm;
        }
    }
    printf("status %d blocks %lld checksum %u\n", status, blocks, checksum);
    delete[] tables;
    free(scan);
    return 0;
}
