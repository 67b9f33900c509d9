// Self-synchronising Huffman decoding of a baseline JPEG scan without restart markers: what one lane of
// jpeg_sync_index_kernel (jpeg_sync.hip) does with its subsequence, on top of the bit reader and the tables of jpeg_entropy.h.  One
// text for the kernel and for the host: tests/jpeg_sync_main.cpp runs the lanes one after another under the address and undefined-
// behaviour sanitizers, and tests/_jpeg_sync_ref.py states the same in Python.
//
// The scan is cut every JS_BYTES raw bytes.  A walker's state at a symbol boundary (a symbol = a Huffman code with its value bits) is
// JsState: the raw byte that holds the next bit, the bit in it, the block j of the MCU and the coefficient index k (0: a DC code comes
// next).  js_walk goes from such a state to the first symbol that begins at or after `stop`, counting the blocks it ends and each
// component's DC differences modulo 2^16, and returns the state there: its exit.  A lane first walks from an assumed state (the first
// bit of its subsequence, j = k = 0), then again from its neighbour's exit until no exit changes; the exits are then the serial
// walker's.  A bad code, size or index does not stop a walk: it is noted (JsCount::err) and the walk goes on, since for a lane that only
// assumed its state it is no error; once the exits stand, a lane that still has one marks where the serial walker stops.  Bits that
// are not there make the exit invalid (p = -1).
//
// Safety on any bytes: a walk reads [data, data + end) only, through JeBits; every turn of its loop consumes at least one bit, so it
// is bounded by the bytes; no private array is indexed dynamically.
#pragma once
#include "jpeg_entropy.h"

constexpr int JS_BYTES = 132;                // raw bytes of a subsequence (ops.JPEG_SYNC_BYTES): 33 words, so the lanes of a workgroup
                                             // that walk neighbouring subsequences in LDS start on 32 different banks
constexpr int JS_SLACK = 32;                 // bytes past a lane's stop that its last symbol and the reader's look-ahead may touch
static_assert(JS_BYTES >= 16 && JS_BYTES % 4 == 0, "a symbol (at most 27 bits, every byte stuffed) is shorter than a subsequence");

struct JsState {
    int p;                                   // raw index of the byte that holds the next bit (never the 00 of an FF 00 pair); -1: invalid
    int q;                                   // bit in that byte (0 = its MSB) | j << 3 | k << 6
};
struct JsCount {
    int blocks;                              // blocks that ended, up to the walk's first error
    int d0, d1, d2;                          // each component's DC differences, summed modulo 2^16
    int err;                                 // the JE_* code of the first error this walk met, or 0
};

TUP_HOST_DEVICE bool js_same(JsState a, JsState b) { return a.p == b.p && a.q == b.q; }
TUP_HOST_DEVICE bool js_mcu_start(JsState s) { return s.p >= 0 && (s.q >> 3) == 0; }

// the state a lane assumes for the subsequence that begins at raw byte `at` >= 1: its first bit, or the byte after if `at` is the 00
// of an FF 00 pair; j = k = 0
TUP_HOST_DEVICE JsState js_assume(const uint8_t* data, int at)
{
    return JsState{at + ((data[at - 1] == 0xFFu && data[at] == 0u) ? 1 : 0), 0};
}

// raw index of the byte that holds the reader's next bit: back from b.pos over the ceil(n / 8) bytes it holds, a stuffed one two bytes
TUP_HOST_DEVICE int js_byte(const JeBits& b)
{
    int p = b.pos;
    for (int c = (b.n + 7) >> 3; c > 0; --c) p -= (p >= 2 && b.data[p - 1] == 0u && b.data[p - 2] == 0xFFu) ? 2 : 1;
    return p;
}

struct JsNoVisit {
    TUP_HOST_DEVICE void operator()(const JeBits&, const JsCount&) const {}
};

// From state s to the first symbol that begins at raw byte >= stop (stop <= end).  visit(reader, counts so far) is called at every
// MCU start the walk passes before it stops or meets an error.  c: what this walk counted up to its first error, c.err: that error or
// 0.  Returns the exit: invalid where s was invalid or the bits ran out; after any other error the state of a walk that went on (see
// below), which a lane whose own state was only assumed hands to its successor all the same.
template <class Visit>
TUP_HOST_DEVICE JsState js_walk(const uint8_t* data, int end, int stop, JsState s, const JeTable* tables, const uint8_t* td, const uint8_t* ta,
                                int layout, JsCount& c, const Visit& visit)
{
    c.blocks = 0; c.d0 = 0; c.d1 = 0; c.d2 = 0; c.err = 0;
    const JsState invalid{-1, 0};
    if (s.p < 0) return invalid;
    JeBits b{data, s.p, end, 0u, 0, 0};
    const int bit = s.q & 7;
    if (bit) {                                                          // the byte was read before: its bits are there
        je_fill(b);
        if (b.n < bit) { c.err = b.hit ? b.hit : JE_END; return invalid; }
        b.acc <<= bit;
        b.n -= bit;
    }
    const int bpm = je_blocks_per_mcu(layout);
    int j = (s.q >> 3) & 7, k = s.q >> 6;
    for (;;) {                                                          // every turn consumes a bit or returns
        // where the next symbol begins: at most b.pos - ceil(n / 8); exactly that, were no byte behind the reader stuffed
        if (b.pos - ((b.n + 7) >> 3) >= stop) {
            const int p = js_byte(b);
            if (p >= stop) return JsState{p, ((8 - (b.n & 7)) & 7) | j << 3 | k << 6};
        }
        if (j == 0 && k == 0 && !c.err) visit(b, c);
        const int comp = je_component(layout, j);
        int err = JE_OK;
        if (k == 0) {
            const int size = je_symbol(b, tables[td[comp] & 1], err);
            if (!err && size > 11) {
                err = JE_BAD_SIZE;                                      // (going on: the code is consumed, no value bits)
            } else if (!err && size) {
                const int diff = je_receive(b, size, err) & 0xFFFF;
                if (!c.err) {
                    c.d0 = (c.d0 + (comp == 0 ? diff : 0)) & 0xFFFF;
                    c.d1 = (c.d1 + (comp == 1 ? diff : 0)) & 0xFFFF;
                    c.d2 = (c.d2 + (comp == 2 ? diff : 0)) & 0xFFFF;
                }
            }
            if (err != JE_BAD_CODE) k = 1;
        } else {
            const int rs = je_symbol(b, tables[2 + (ta[comp] & 1)], err);
            const int r = rs >> 4, size = rs & 15;
            if (!err) {
                if (size == 0) {
                    k = r == 15 ? k + 16 : 64;                          // ZRL, or EOB
                } else if (size > 10) {
                    err = JE_BAD_SIZE;                                  // (going on: the code is consumed, no value bits)
                    k += r + 1;
                } else {
                    k += r;
                    if (k > 63) { err = JE_BAD_INDEX; k = 64; }         // (going on: the block ends here)
                    else { je_receive(b, size, err); ++k; }
                }
            }
        }
        if (err) {
            // The first error ends what this walk counts and visits.  The walk itself goes on where it can, so that a lane that only
            // assumed its state still comes to an exit its successor can start from: a walker in the wrong place meets such errors
            // often, and one that stopped at them would never fall into step.  Without bits there is nowhere to go on.
            if (!c.err) c.err = err;
            if (err == JE_MARKER || err == JE_END) return invalid;
            if (err == JE_BAD_CODE) {                                   // nothing was consumed: skip a bit
                if (b.n < 1) return invalid;
                b.acc <<= 1;
                b.n -= 1;
            }
        }
        if (k >= 64) {                                                  // the block ends
            if (!c.err) ++c.blocks;
            k = 0;
            j = j + 1 == bpm ? 0 : j + 1;
        }
    }
}

// The blocks whose end is followed, inside one lane's walk, by the start of an MCU: with `before` blocks ended ahead of the lane and
// `blocks` in it, the MCU starts the lane passes are those after block lo .. hi (block 0: the start of the scan).  first_row_block:
// the first multiple of blocks-per-row in lo .. hi, or -1: the lane passes no start of an MCU row and need not walk again.
TUP_HOST_DEVICE int js_first_row_block(int before, int blocks, JsState entry, JsState exit, int blocks_per_row)
{
    const int lo = before + (js_mcu_start(entry) ? 0 : 1), hi = before + blocks - (js_mcu_start(exit) ? 1 : 0);
    const int first = (lo + blocks_per_row - 1) / blocks_per_row * blocks_per_row;
    return first <= hi ? first : -1;
}

// the DC predictor after differences that sum to d modulo 2^16 (je_block wraps it to int16 at every block, so wrapping sums compose)
TUP_HOST_DEVICE int js_pred(int d) { return (int)(int16_t)(uint16_t)(d & 0xFFFF); }
