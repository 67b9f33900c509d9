// The serial half of the PNG decoder (png_decode.hip): a bounded bit reader, decode tables built from code lengths under
// RFC 1951's validity rules, the one-token decoder, the walk through the blocks of a zlib stream, and PNG's unfilter arithmetic for
// one byte.  One text for the kernels and for the host (tests/png_inflate_main.cpp runs it under the address and undefined-behaviour
// sanitizers); tests/_png_decode_ref.py states the same rules in Python.  The canonical code assignment is png_deflate.h's (pd_code).
//
// A walker is pi_inflate<Src, Sink, Walk>.  Src hands out 64 stream bits from any bit position, zeros past the end (peek), Sink
// receives the output (lit / match / stored / advance / finish) and Walk decodes the tokens of one Huffman block.  Everything in
// here is written to be run by `nlanes` lanes that hold the same values (1 on the host, the 64 of a wave in the kernel): the loops
// that build a table are spread over the lanes, everything else is repeated by all of them.  PI_SYNC orders the table's memory
// between those loops.
#pragma once
#include "png_deflate.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PI_SYNC() __syncthreads()
#else
#define PI_SYNC() ((void)0)
#endif

// status of an image: 0, or the first thing that went wrong in stream order
enum PiStatus : int {
    PI_OK = 0,
    PI_BAD_BLOCK_TYPE = 1,       // block type 3
    PI_BAD_STORED_LEN = 2,       // a stored block whose LEN is not the complement of NLEN
    PI_BAD_CODE = 3,             // a code RFC 1951 forbids: over-subscribed, incomplete (but for a single one-bit code of the literal or
                                 // distance alphabet), more than 286 / 30 symbols, a repeat without a length before it or past the
                                 // end of the list, no end-of-block code
    PI_NO_SYMBOL = 4,            // bits that are no code of the table, or a code of symbol 286, 287 or distance 30, 31
    PI_BAD_DISTANCE = 5,         // a match that begins before the start of the stream
    PI_INPUT_EXHAUSTED = 6,      // the stream ends inside a header, a token, a stored block or the Adler-32
    PI_OUTPUT_LONG = 7,          // more than stream_bytes bytes
    PI_OUTPUT_SHORT = 8,         // the final block ends before stream_bytes bytes
    PI_BAD_FILTER = 9,           // a row whose filter byte is above 4
    PI_BAD_ADLER = 10,           // the Adler-32 of the inflated bytes is not the stream's
};

constexpr int PI_FAST_BITS = 10;                         // codes up to this length are one table read
constexpr int PI_FAST = 1 << PI_FAST_BITS;
constexpr int PI_MAX_SYM = 288;                          // the fixed literal / length code has 288 symbols (its distance code 32)
constexpr int PI_LENS = PI_MAX_SYM + 32;
constexpr int PI_LIT = 0, PI_DIST = 1, PI_CL = 2;        // kinds of code (the code-length code is built in table 0)
constexpr uint32_t PI_STORED_PIECE = 16384;              // a stored block reaches the sink in pieces of at most this

struct PiTables {
    uint16_t fast[2][PI_FAST];        // symbol << 4 | length of the code whose reversed bits are the index's low bits; 0: none that short
    uint16_t sorted[2][PI_MAX_SYM];   // the coded symbols in (length, symbol) order
    uint16_t count[2][16];            // codes of every length
    uint8_t lens[PI_LENS];            // the code lengths of a header: literal / length symbols, then distances
    uint8_t cl_lens[PD_CL + 1];
};

// one decoded token: kind 0 literal (value), 1 match (len, dist), 2 end of block; err 0, PI_NO_SYMBOL or PI_INPUT_EXHAUSTED; used: its bits
struct PiToken {
    int err, kind, used, value, len, dist;
};

// the place of symbol s among the coded symbols in (length, symbol) order
PD_HOST_DEVICE int pi_place(const uint8_t* lens, int nsym, int s)
{
    const int l = lens[s];
    int r = 0;
    for (int j = 0; j < nsym; ++j) {
        const int m = lens[j];
        r += m && (m < l || (m == l && j < s));
    }
    return r;
}

// Table `which` from nsym code lengths -> 0 or PI_BAD_CODE.  No code at all is accepted here (a block of literals has no distance code).
PD_HOST_DEVICE int pi_build(PiTables& t, int which, const uint8_t* lens, int nsym, int kind, int lane, int nlanes)
{
    int count[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < nsym; ++s) {
        const int m = lens[s];
#pragma unroll
        for (int l = 0; l < 16; ++l) count[l] += m == l;     // no dynamic index into the private array
    }
    int left = 1, coded = 0;
    bool over = false;                                       // over-subscribed at some length
#pragma unroll
    for (int l = 1; l < 16; ++l) {
        left = left * 2 - count[l];
        coded += count[l];
        if (left < 0) { over = true; left = 0; }
    }
    if (over) return PI_BAD_CODE;
    if (left > 0 && coded > 0 && (kind == PI_CL || !(coded == 1 && count[1] == 1))) return PI_BAD_CODE;
    if (coded == 0 && kind == PI_CL) return PI_BAD_CODE;
    PI_SYNC();                                               // readers of the table it replaces are done
#pragma unroll
    for (int l = 0; l < 16; ++l)
        if (lane == 0) t.count[which][l] = (uint16_t)count[l];
    for (int i = lane; i < PI_FAST; i += nlanes) t.fast[which][i] = 0;
    PI_SYNC();
    for (int s = lane; s < nsym; s += nlanes) {
        const int l = lens[s];
        if (!l) continue;
        t.sorted[which][pi_place(lens, nsym, s)] = (uint16_t)s;
        if (l <= PI_FAST_BITS)
            for (uint32_t k = pd_code(lens, nsym, s); k < (uint32_t)PI_FAST; k += 1u << l) t.fast[which][k] = (uint16_t)(s << 4 | l);
    }
    PI_SYNC();
    return PI_OK;
}

// the symbol whose code begins at bit 0 of w, or -1; l: the bits of the code, 15 where there is none
PD_HOST_DEVICE int pi_symbol(const PiTables& t, int which, uint64_t w, int& l)
{
    const int e = t.fast[which][(uint32_t)w & (PI_FAST - 1)];
    if (e) { l = e & 15; return e >> 4; }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(w >> (len - 1)) & 1;
        const int c = t.count[which][len];
        if (code - c < first) { l = len; return t.sorted[which][index + (code - first)]; }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    l = 15;
    return -1;
}

// The token of a Huffman block that begins at bit 0 of w (64 stream bits, zeros past the end of the stream); `avail`: the bits the
// stream still has from there.  A token is at most 15 + 5 + 15 + 13 = 48 bits.
PD_HOST_DEVICE PiToken pi_token(const PiTables& t, uint64_t w, uint64_t avail)
{
    PiToken k = {0, 0, 0, 0, 0, 0};
    int l;
    const int sym = pi_symbol(t, PI_LIT, w, l);
    k.used = l;
    if (sym < 0 || sym >= PD_LIT) k.err = PI_NO_SYMBOL;
    else if (sym < 256) k.value = sym;
    else if (sym == 256) k.kind = 2;
    else {
        k.kind = 1;
        const int eb = pd_length_extra(sym);
        k.len = sym < 265 ? sym - 254 : sym == 285 ? 258 : 3 + ((4 + ((sym - 261) & 3)) << eb) + ((int)(w >> k.used) & ((1 << eb) - 1));
        k.used += eb;
        const int ds = pi_symbol(t, PI_DIST, w >> k.used, l);
        k.used += l;
        if (ds < 0 || ds >= PD_DIST) k.err = PI_NO_SYMBOL;
        else {
            const int db = ds < 4 ? 0 : (ds >> 1) - 1;
            k.dist = ds < 4 ? ds + 1 : 1 + ((2 + (ds & 1)) << db) + ((int)(w >> k.used) & ((1 << db) - 1));
            k.used += db;
        }
    }
    if ((uint64_t)k.used > avail) k.err = PI_INPUT_EXHAUSTED;
    return k;
}

// the tables of a fixed block
PD_HOST_DEVICE int pi_fixed_tables(PiTables& t, int lane, int nlanes)
{
    PI_SYNC();
    for (int s = lane; s < PI_LENS; s += nlanes) t.lens[s] = (uint8_t)(s < PI_MAX_SYM ? pd_fixed_length(s) : 5);
    PI_SYNC();
    const int e = pi_build(t, PI_LIT, t.lens, PI_MAX_SYM, PI_LIT, lane, nlanes);
    return e ? e : pi_build(t, PI_DIST, t.lens + PI_MAX_SYM, 32, PI_DIST, lane, nlanes);
}

// the header of a dynamic block at bit pos -> its tables; pos moves past it
template <class Src>
PD_HOST_DEVICE int pi_dynamic_tables(PiTables& t, Src& src, uint64_t& pos, int lane, int nlanes)
{
    const uint64_t nbits = src.nbits();
    if (pos + 14 > nbits) return PI_INPUT_EXHAUSTED;
    uint64_t w = src.peek(pos);
    const int nlen = 257 + ((int)w & 31), nd = 1 + ((int)(w >> 5) & 31), ncl = 4 + ((int)(w >> 10) & 15);
    pos += 14;
    if (nlen > PD_LIT || nd > PD_DIST) return PI_BAD_CODE;
    if (pos + 3 * (uint64_t)ncl > nbits) return PI_INPUT_EXHAUSTED;
    w = src.peek(pos);
    PI_SYNC();
    if (lane == 0)
        for (int k = 0; k < PD_CL; ++k) t.cl_lens[pd_cl_order(k)] = (uint8_t)(k < ncl ? (w >> (3 * k)) & 7 : 0);
    PI_SYNC();
    pos += 3 * (uint64_t)ncl;
    int e = pi_build(t, 0, t.cl_lens, PD_CL, PI_CL, lane, nlanes);
    if (e) return e;
    const int total = nlen + nd;
    int i = 0, prev = 0;                                  // prev: the length before position i
    while (i < total) {
        w = src.peek(pos);
        int l;
        const int sym = pi_symbol(t, 0, w, l);
        int used = l + (sym < 0 ? 0 : pd_cl_extra(sym));
        if (pos + (uint64_t)used > nbits) return PI_INPUT_EXHAUSTED;
        if (sym < 0) return PI_NO_SYMBOL;
        int n = 1, v = sym;
        if (sym == 16) {
            if (i == 0) return PI_BAD_CODE;
            v = prev; n = 3 + ((int)(w >> l) & 3);
        } else if (sym == 17) { v = 0; n = 3 + ((int)(w >> l) & 7); }
        else if (sym == 18) { v = 0; n = 11 + ((int)(w >> l) & 127); }
        if (i + n > total) return PI_BAD_CODE;
        if (lane == 0)
            for (int k = 0; k < n; ++k) t.lens[i + k] = (uint8_t)v;
        i += n; prev = v; pos += (uint64_t)used;
    }
    PI_SYNC();
    if (t.lens[256] == 0) return PI_BAD_CODE;
    e = pi_build(t, PI_LIT, t.lens, nlen, PI_LIT, lane, nlanes);
    return e ? e : pi_build(t, PI_DIST, t.lens + nlen, nd, PI_DIST, lane, nlanes);
}

// the tokens of one Huffman block, one a round: the plain walk
struct PiTokenWalk {
    template <class Src, class Sink>
    PD_HOST_DEVICE int operator()(const PiTables& t, Src& src, Sink& sink, uint64_t& pos, uint32_t& o, uint32_t total) const
    {
        const uint64_t nbits = src.nbits();
        for (;;) {
            const PiToken k = pi_token(t, src.peek(pos), nbits - pos);
            if (k.err) return k.err;
            pos += (uint64_t)k.used;
            if (k.kind == 2) return PI_OK;
            if (k.kind == 0) {
                if (o >= total) return PI_OUTPUT_LONG;
                sink.lit(o, k.value);
                o += 1;
            } else {
                if ((uint32_t)k.dist > o) return PI_BAD_DISTANCE;
                if ((uint32_t)k.len > total - o) return PI_OUTPUT_LONG;
                sink.match(o, k.len, k.dist);
                o += (uint32_t)k.len;
            }
            sink.advance(o);
        }
    }
};

// A zlib stream (its two header bytes checked by the caller) inflated to exactly `total` bytes and its Adler-32 compared -> status.
template <class Src, class Sink, class Walk>
PD_HOST_DEVICE int pi_inflate(PiTables& t, Src& src, Sink& sink, const Walk& walk, uint32_t total, int lane, int nlanes)
{
    const uint64_t nbits = src.nbits();
    uint64_t pos = 16;
    uint32_t o = 0;
    for (;;) {
        if (pos + 3 > nbits) return PI_INPUT_EXHAUSTED;
        const int head = (int)src.peek(pos) & 7;
        pos += 3;
        const int type = head >> 1;
        if (type == 3) return PI_BAD_BLOCK_TYPE;
        if (type == 0) {
            pos = (pos + 7) & ~(uint64_t)7;
            if (pos + 32 > nbits) return PI_INPUT_EXHAUSTED;
            const uint32_t w = (uint32_t)src.peek(pos);
            uint32_t len = w & 0xffffu;
            if (len != (~(w >> 16) & 0xffffu)) return PI_BAD_STORED_LEN;
            pos += 32;
            if (pos + 8 * (uint64_t)len > nbits) return PI_INPUT_EXHAUSTED;
            if (len > total - o) return PI_OUTPUT_LONG;
            while (len) {
                const uint32_t n = len < PI_STORED_PIECE ? len : PI_STORED_PIECE;
                sink.stored(o, pos >> 3, n);
                o += n; pos += 8 * (uint64_t)n; len -= n;
                sink.advance(o);
            }
        } else {
            int e = type == 1 ? pi_fixed_tables(t, lane, nlanes) : pi_dynamic_tables(t, src, pos, lane, nlanes);
            if (!e) e = walk(t, src, sink, pos, o, total);
            if (e) return e;
        }
        if (head & 1) break;
    }
    if (o != total) return PI_OUTPUT_SHORT;
    pos = (pos + 7) & ~(uint64_t)7;
    if (pos + 32 > nbits) return PI_INPUT_EXHAUSTED;
    const uint32_t w = (uint32_t)src.peek(pos);
    const uint32_t want = (w << 24) | ((w & 0xff00u) << 8) | ((w >> 8) & 0xff00u) | (w >> 24);
    return sink.finish(o) == want ? PI_OK : PI_BAD_ADLER;
}

// ---- PNG's filters, undone for one byte: a the byte bpp before it in its row, b the byte above, c the byte above a (all reconstructed) ----
PD_HOST_DEVICE int pi_unfilter_byte(int filter, int x, int a, int b, int c)
{
    int pred = 0;
    if (filter == 1) pred = a;
    else if (filter == 2) pred = b;
    else if (filter == 3) pred = (a + b) >> 1;
    else if (filter == 4) {
        const int p = a + b - c;
        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        pred = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
    }
    return (x + pred) & 255;
}
