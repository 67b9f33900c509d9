// The serial, index-heavy half of the PNG encoder (png_encode.hip): length-limited Huffman code lengths, canonical codes, the
// run-length coder of a dynamic block's code lengths, the fixed code, and CRC-32 / Adler-32 arithmetic.  One text for the kernels and for
// the host (tests/png_deflate_main.cpp runs it under the address and undefined-behaviour sanitizers); tests/_png_ref.py states the same
// rules in Python.  Every array is the caller's (LDS in the kernels): nothing here indexes a private array dynamically.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PD_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define PD_HOST_DEVICE inline
#endif

constexpr int PD_LIT = 286;                  // literal / length symbols
constexpr int PD_DIST = 30;                  // distance symbols
constexpr int PD_CL = 19;                    // symbols of the code-length alphabet
constexpr int PD_MAX_SEQ = PD_LIT + PD_DIST; // the longest code-length sequence of a dynamic header
constexpr uint32_t PD_ADLER = 65521u;
constexpr uint32_t PD_CRC_POLY = 0xEDB88320u;

// position k of a dynamic header's HCLEN list holds the length of this code-length symbol
PD_HOST_DEVICE int pd_cl_order(int k)
{
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return k < 3 ? 16 + k : k == 3 ? 0 : (k & 1) ? 8 - ((k - 3) >> 1) : 8 + ((k - 4) >> 1);
}

// the fixed literal / length code of deflate, symbols 0..287 (its distance code is five bits, the symbol itself)
PD_HOST_DEVICE int pd_fixed_length(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// extra bits that follow a length symbol 257..285
PD_HOST_DEVICE int pd_length_extra(int sym) { return sym >= 265 && sym < 285 ? (sym - 261) >> 2 : 0; }

// match length 3..258 -> its symbol; extra: how many bits follow, value: those bits
PD_HOST_DEVICE int pd_length_symbol(int len, int& extra, int& value)
{
    extra = value = 0;
    if (len == 258) return 285;
    const int v = len - 3;
    if (v < 8) return 257 + v;
    const int eb = 29 - __builtin_clz((unsigned)v);      // floor(log2 v) - 2, v in 8..254
    extra = eb;
    value = v & ((1 << eb) - 1);
    return 261 + 4 * eb + ((v >> eb) & 3);
}

// ---- code lengths ----
// The place of symbol s among the symbols with a count, ordered by (count, symbol); -1 for a symbol without one.  A lane per symbol in
// the kernels.
PD_HOST_DEVICE int pd_rank(const int* freq, int nsym, int s)
{
    const int f = freq[s];
    if (f <= 0) return -1;
    int r = 0;
    for (int j = 0; j < nsym; ++j) {
        const int g = freq[j];
        r += g > 0 && (g < f || (g == f && j < s));
    }
    return r;
}

// Moffat & Katajainen's in-place minimum-redundancy code: a[0..n) counts in ascending order -> code lengths, longest first.  n >= 2.
PD_HOST_DEVICE void pd_minimum_redundancy(int* a, int n)
{
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = next; }
        else a[next] = a[leaf++];
        if (leaf >= n || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = next; }
        else a[next] += a[leaf++];
    }
    a[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    int avail = 1, used = 0, depth = 0, root2 = n - 2, next = n - 1;
    while (avail > 0) {
        while (root2 >= 0 && a[root2] == depth) { ++used; --root2; }
        while (avail > used) { a[next--] = depth; --avail; }
        avail = 2 * used; ++depth; used = 0;
    }
}

// sorted[0..n): the counts in (count, symbol) order, overwritten; order[i]: the symbol at place i; lens[0..nsym): zeroed by the caller,
// receives the lengths, none above `limit`.  count: 16 words of work space.  A single symbol gets length 1; two or more get a complete
// code (Kraft sum 1): lengths above the limit are clamped, then codes are moved down from the limit until the sum is 1 again, and the
// longest lengths go to the first symbols of the order.
PD_HOST_DEVICE void pd_lengths(int* sorted, const uint16_t* order, int n, int limit, int* count, uint8_t* lens)
{
    if (n < 1) return;
    if (n == 1) { lens[order[0]] = 1; return; }
    pd_minimum_redundancy(sorted, n);
    for (int l = 0; l <= 15; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) count[sorted[i] < limit ? sorted[i] : limit] += 1;
    uint32_t total = 0;
    for (int l = 1; l <= limit; ++l) total += (uint32_t)count[l] << (limit - l);
    while (total > (1u << limit)) {
        count[limit] -= 1;
        for (int l = limit - 1; l > 0; --l)
            if (count[l]) { count[l] -= 1; count[l + 1] += 2; break; }
        --total;
    }
    int i = 0;
    for (int l = limit; l > 0; --l)
        for (int c = count[l]; c > 0; --c) lens[order[i++]] = (uint8_t)l;
}

// the whole builder, serial: what the host runs; the kernels run pd_rank on a lane per symbol and pd_lengths on one lane
PD_HOST_DEVICE void pd_build_lengths(const int* freq, int nsym, int limit, int* sorted, uint16_t* order, int* count, uint8_t* lens)
{
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        lens[s] = 0;
        const int r = pd_rank(freq, nsym, s);
        if (r >= 0) { sorted[r] = freq[s]; order[r] = (uint16_t)s; ++n; }
    }
    pd_lengths(sorted, order, n, limit, count, lens);
}

// the canonical code of symbol s, its bits reversed (deflate sends a code's first bit first, in a stream filled from bit 0 up)
PD_HOST_DEVICE uint32_t pd_code(const uint8_t* lens, int nsym, int s)
{
    const int l = lens[s];
    if (!l) return 0;
    uint32_t code = 0;                       // sum over shorter lengths of their codes, scaled to this length, plus equals before s
    for (int j = 0; j < nsym; ++j) {
        const int m = lens[j];
        if (m && m < l) code += 1u << (l - m);
        else if (m == l && j < s) code += 1u;
    }
    uint32_t r = 0;
    for (int k = 0; k < l; ++k) r |= ((code >> k) & 1u) << (l - 1 - k);
    return r;
}

// ---- the code lengths of a dynamic header, run-length coded ----
// seq[0..n): the HLIT literal/length lengths followed by the HDIST distance lengths.  tokens[]: symbol | extra-bit value << 8, at most n
// of them; cl_freq[19] is counted.  Zeros: 18 (11..138) while 11 or more remain, then 17 (3..10), then single zeros.  A length v: v
// once, then 16 (3..6) while 3 or more remain, then single v.
PD_HOST_DEVICE int pd_run_length_code(const uint8_t* seq, int n, uint16_t* tokens, int* cl_freq)
{
    for (int s = 0; s < PD_CL; ++s) cl_freq[s] = 0;
    int nt = 0, i = 0;
    while (i < n) {
        const int v = seq[i];
        int j = i;
        while (j < n && seq[j] == v) ++j;
        int c = j - i;
        i = j;
        if (v == 0) {
            while (c >= 11) {
                const int k = c < 138 ? c : 138;
                tokens[nt++] = (uint16_t)(18 | ((k - 11) << 8)); cl_freq[18] += 1; c -= k;
            }
            if (c >= 3) { tokens[nt++] = (uint16_t)(17 | ((c - 3) << 8)); cl_freq[17] += 1; c = 0; }
        } else {
            tokens[nt++] = (uint16_t)v; cl_freq[v] += 1; --c;
            while (c >= 3) {
                const int k = c < 6 ? c : 6;
                tokens[nt++] = (uint16_t)(16 | ((k - 3) << 8)); cl_freq[16] += 1; c -= k;
            }
        }
        for (; c > 0; --c) { tokens[nt++] = (uint16_t)v; cl_freq[v] += 1; }
    }
    return nt;
}
PD_HOST_DEVICE int pd_cl_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// ---- CRC-32 (reflected, as PNG and zlib use it) ----
// A CRC state is a polynomial over GF(2) modulo the CRC polynomial, bit 31 the coefficient of x^0.  With s(init, M) the state after the
// bytes M:  s(init, M) = s(init, zeros of M's length) ^ s(0, M),  s(v, k zero bytes) = v * x^(8k),  s(0, A B) = s(0, A) * x^(8 |B|) ^ s(0, B).
// So lanes take the state of their own pieces from zero, and the pieces combine with multiplications.
PD_HOST_DEVICE uint32_t pd_crc_byte(uint32_t state, uint32_t byte)
{
    state ^= byte;
    for (int k = 0; k < 8; ++k) state = (state >> 1) ^ (PD_CRC_POLY & (0u - (state & 1u)));
    return state;
}
PD_HOST_DEVICE uint32_t pd_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        p ^= b & (0u - ((a >> (31 - k)) & 1u));
        b = (b >> 1) ^ (PD_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 nbytes)
PD_HOST_DEVICE uint32_t pd_crc_shift(uint32_t nbytes)
{
    uint32_t p = 0x80000000u, base = 0x00800000u;        // x^0, x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) p = pd_crc_mul(p, base);
        base = pd_crc_mul(base, base);
    }
    return p;
}
// the CRC-32 of `total` bytes from the XOR of every piece's  s(0, piece) * x^(8 * bytes after the piece)
PD_HOST_DEVICE uint32_t pd_crc_finish(uint32_t pieces, uint32_t total) { return pd_crc_mul(0xFFFFFFFFu, pd_crc_shift(total)) ^ pieces ^ 0xFFFFFFFFu; }

// ---- Adler-32 ----
// A block of n bytes d has the partial (a, b) = (sum d[i], sum (n - i) d[i]) mod 65521, packed b << 16 | a.  A stream's state (A, B)
// starts at (1, 0); a block moves it to (A + a, B + n A + b).
PD_HOST_DEVICE void pd_adler_append(uint32_t& A, uint32_t& B, uint32_t partial, uint32_t n)
{
    B = (B + (n % PD_ADLER) * A % PD_ADLER + (partial >> 16)) % PD_ADLER;
    A = (A + (partial & 0xffffu)) % PD_ADLER;
}
