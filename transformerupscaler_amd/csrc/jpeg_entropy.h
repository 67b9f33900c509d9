// The entropy-coded half of a baseline JPEG decoder: bit reader, Huffman table builder and block walker.  One text for the
// kernels of jpeg_decode.hip and for the host (tests/jpeg_entropy_main.cpp walks damaged scans with it under the address and
// undefined-behaviour sanitizers), so what the sanitizers saw is what the GPU runs.  tests/_jpeg_decode_ref.py states it in numpy.
//
// Safety on any bytes: every loop here is bounded by the byte range it was given (JeBits::end), by 64 coefficients a block and by
// the caller's block count; nothing is read outside [data, data + end) and nothing is written outside the 64 words of a block.  A
// bad condition ends the walk with one of the JE_* codes below; the caller records it as the image's status.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TUP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define TUP_HOST_DEVICE inline
#endif

enum {
    JE_OK = 0,
    JE_BAD_CODE = 1,         // bits that are no code of the table
    JE_BAD_INDEX = 2,        // a run that puts a coefficient past index 63
    JE_BAD_SIZE = 3,         // a DC category above 11 or an AC size above 10
    JE_MARKER = 4,           // a marker inside the segment, where more bits were needed
    JE_END = 5,              // the data ended where more bits were needed
    JE_RESTARTS = 6,         // the scan holds another number of restart markers than its restart interval asks for
    JE_BAD_TABLE = 7,        // Huffman counts that are no prefix code
    JE_BAD_RECORD = 8        // an image record that does not describe bytes inside the upload
};

// natural index of the k-th coefficient in zigzag order
#define JE_ZIGZAG_INIT {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, \
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

constexpr int JE_SPEC_BYTES = 16 + 256;      // a table as DHT carries it: the number of codes of each length 1..16, then the symbols

// With p = the next 16 bits of the stream: a code of length l <= 8 is found through lut[p >> 8] = l << 8 | symbol (0: none that
// short); a longer one has the smallest l with p < limit[l], and its symbol is values[offset[l] + (p >> (16 - l))].
struct JeTable {
    int limit[17];           // (the first code of length l + the number of them) << (16 - l); never decreases with l
    int offset[17];          // index of the first symbol of length l - its code
    uint16_t lut[256];
    uint8_t values[256];
};

// spec: JE_SPEC_BYTES.  false: the counts are no prefix code (a length with more codes than are left, or more than 256 symbols);
// the table then matches nothing.
TUP_HOST_DEVICE bool je_build(const uint8_t* spec, JeTable& t)
{
    for (int i = 0; i < 256; ++i) { t.lut[i] = 0; t.values[i] = spec[16 + i]; }
    for (int l = 0; l <= 16; ++l) { t.limit[l] = 0; t.offset[l] = 0; }
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = spec[l - 1];
        if (code + n > (1 << l) || k + n > 256) {
            for (int i = 0; i <= 16; ++i) t.limit[i] = 0;
            for (int i = 0; i < 256; ++i) t.lut[i] = 0;
            return false;
        }
        t.offset[l] = k - code;
        if (l <= 8)
            for (int c = 0; c < n; ++c) {
                const int first = (code + c) << (8 - l);
                for (int f = 0; f < (1 << (8 - l)); ++f) t.lut[first + f] = (uint16_t)((l << 8) | t.values[k + c]);
            }
        code += n;
        k += n;
        t.limit[l] = code << (16 - l);
        code <<= 1;
    }
    return true;
}

// The bits of data[pos .. end), MSB first, with 0xFF 0x00 read as 0xFF.  acc holds the next n bits at its top and zeros below them;
// hit = JE_MARKER / JE_END once the bytes have run out, after which nothing more is read.
struct JeBits {
    const uint8_t* data;
    int pos, end;
    uint32_t acc;
    int n, hit;
};

TUP_HOST_DEVICE void je_fill(JeBits& b)
{
    while (b.n <= 24 && !b.hit) {                                       // at most four bytes
        if (b.pos >= b.end) { b.hit = JE_END; break; }
        const uint32_t v = b.data[b.pos];
        if (v == 0xFFu) {
            if (b.pos + 1 >= b.end) { b.hit = JE_END; break; }
            if (b.data[b.pos + 1] != 0) { b.hit = JE_MARKER; break; }
            b.pos += 2;
        } else {
            ++b.pos;
        }
        b.acc |= v << (24 - b.n);
        b.n += 8;
    }
}

TUP_HOST_DEVICE int je_symbol(JeBits& b, const JeTable& t, int& err)
{
    je_fill(b);
    const int p = (int)(b.acc >> 16);
    const int e = t.lut[p >> 8];
    int len, sym;
    if (e) {
        len = e >> 8;
        sym = e & 255;
    } else {
        len = 9;
        while (len <= 16 && p >= t.limit[len]) ++len;
        if (len > 16) { err = JE_BAD_CODE; return 0; }
        sym = t.values[(t.offset[len] + (p >> (16 - len))) & 255];
    }
    if (len > b.n) { err = b.hit ? b.hit : JE_END; return 0; }         // the code reaches into bits that are not there
    b.acc <<= len;
    b.n -= len;
    return sym;
}

// s bits, 1 <= s <= 16, extended to a signed value as F.2.2.1 says
TUP_HOST_DEVICE int je_receive(JeBits& b, int s, int& err)
{
    je_fill(b);
    if (s > b.n) { err = b.hit ? b.hit : JE_END; return 0; }
    const int v = (int)(b.acc >> (32 - s));
    b.acc <<= s;
    b.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block.  pred: the DC predictor of its component, updated.  coef: 64 words in natural order, zero on entry, or null for a walk
// that only moves through the bits.  zz: the zigzag table.  Returns JE_OK or the reason it stopped.
TUP_HOST_DEVICE int je_block(JeBits& b, const JeTable& dc, const JeTable& ac, int& pred, int* coef, const uint8_t* zz)
{
    int err = JE_OK;
    const int s = je_symbol(b, dc, err);
    if (err) return err;
    if (s > 11) return JE_BAD_SIZE;
    if (s) {
        const int diff = je_receive(b, s, err);
        if (err) return err;
        pred = (int)(int16_t)((uint32_t)pred + (uint32_t)diff);        // libjpeg keeps coefficients in 16 bits; no overflow on any bytes
    }
    if (coef) coef[0] = pred;
    for (int k = 1; k < 64;) {                                          // k grows every turn
        const int rs = je_symbol(b, ac, err);
        if (err) return err;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;                                         // EOB
            k += 16;                                                    // ZRL
            continue;
        }
        if (sz > 10) return JE_BAD_SIZE;
        k += r;
        if (k > 63) return JE_BAD_INDEX;
        const int v = je_receive(b, sz, err);
        if (err) return err;
        if (coef) coef[zz[k]] = v;
        ++k;
    }
    return JE_OK;
}

// component of block j of an MCU; layout: 0 = 4:4:4 (Y Cb Cr), 2 = 4:2:0 (Y Y Y Y Cb Cr), 4 = grey (Y)
TUP_HOST_DEVICE int je_blocks_per_mcu(int layout) { return layout == 2 ? 6 : (layout == 0 ? 3 : 1); }
TUP_HOST_DEVICE int je_component(int layout, int j) { return layout == 2 ? (j < 4 ? 0 : j - 3) : (layout == 0 ? j : 0); }

// One MCU.  tables: DC 0, DC 1, AC 0, AC 1; td / ta: each component's selectors (0 or 1); pred: the three predictors; coef: the
// MCU's blocks, `pitch` words apart, or null.
TUP_HOST_DEVICE int je_mcu(JeBits& b, const JeTable* tables, const uint8_t* td, const uint8_t* ta, int layout, int* pred, int* coef, int pitch,
                           const uint8_t* zz)
{
    const int nblk = je_blocks_per_mcu(layout);
    for (int j = 0; j < nblk; ++j) {
        const int c = je_component(layout, j);
        const int err = je_block(b, tables[td[c] & 1], tables[2 + (ta[c] & 1)], pred[c], coef ? coef + j * pitch : nullptr, zz);
        if (err) return err;
    }
    return JE_OK;
}

// the most bytes one MCU can take in the scan: six blocks of a 16 + 11 bit DC and 63 AC of 16 + 10 bits, every byte stuffed, and the
// four bytes the reader looks ahead
constexpr int JE_MCU_BYTES = 6 * 2 * ((27 + 63 * 26 + 7) / 8) + 8;
