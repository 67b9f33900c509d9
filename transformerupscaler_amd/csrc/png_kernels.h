// The kernels of the PNG encoder as templates on BPS, the bytes of a sample (1: 8-bit files, 2: 16-bit files), and the launchers of the
// three that read pixels.  png_encode.hip instantiates BPS = 1 and holds the depth-independent scan; png16_encode.hip instantiates
// BPS = 2.  png_encode.hip's head comment describes the encoder.
#pragma once
#include "common.h"
#include "jpeg_dct.h"
#include "png_deflate.h"

namespace {
constexpr int PN_THREADS = 256;
constexpr int PN_MIN_BLOCK = 256, PN_MAX_BLOCK = 32768;
constexpr int PN_DIST_AT = 288;                             // the distance symbols follow the literal / length symbols in one array
constexpr int PN_SYMS = 320;
constexpr int PN_ADAPTIVE = 5;
constexpr int PN_HEAD = 33, PN_TAIL = 28;                   // signature + IHDR; the Adler IDAT + IEND

struct PnShared {
    int hist[4][PN_SYMS];                                   // per wave; [0] holds the sum afterwards
    int sorted[PD_LIT + 2];
    uint32_t codes[PN_SYMS];                                // length << 16 | code, bits reversed
    int scan[2][PN_THREADS];
    int count[16];
    int cl_freq[PD_CL + 1], cl_sorted[PD_CL + 1];
    uint32_t cl_codes[PD_CL + 1];
    int n_used, n_cl, hlit, hclen, header_bits;
    int body_bits[2];                                       // fixed, dynamic
    uint32_t adler[2], crc;
    uint16_t order[PD_LIT + 2], cl_order[PD_CL + 1], cl_tokens[PD_MAX_SEQ];
    uint8_t lens[PN_SYMS], seq[PN_SYMS], cl_lens[PD_CL + 1];
};
constexpr int pn_round16(int v) { return (v + 15) & ~15; }
constexpr int PN_SHARED = pn_round16((int)sizeof(PnShared));
constexpr int pn_data_bytes(int bb) { return pn_round16(bb + 16); }
constexpr int pn_out_bytes(int bb) { return pn_round16(bb + 64); }      // 3 of misalignment + 12 + 2 + 5 + n, and a word of slack for the puts

TUP_DEVICE int pn_to_u8(float x) { return (int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }      // tensor_to_frames' rule (image_io.hip)
// q_16 ("P010 frames"): t = x * 65535, NaN -> 0, clamp, (int)(t + 0.5f); the clamp keeps the multiply and the add apart
TUP_DEVICE int pn_to_u16(float x) { const float t = fminf(fmaxf(x * 65535.0f, 0.0f), 65535.0f); return (int)(t + 0.5f); }

// byte x of row y of the image's 3 BPS W bytes a row; exactly one of u8 (HWC: uint8 for BPS = 1, uint16 for BPS = 2) and f32 (CHW) is set
template <int BPS>
TUP_DEVICE int pn_raw(const uint8_t* u8, const float* f32, size_t plane, int W, int y, int x)
{
    if (BPS == 1) {
        if (u8) return u8[(size_t)y * W * 3 + x];
        const int px = x / 3, ch = x - 3 * px;
        return pn_to_u8(f32[ch * plane + (size_t)y * W + px]);
    }
    const int sx = x >> 1, px = sx / 3, ch = sx - 3 * px;                          // the file's samples are big-endian: high byte first
    const int v = u8 ? reinterpret_cast<const uint16_t*>(u8)[(size_t)y * W * 3 + sx] : pn_to_u16(f32[ch * plane + (size_t)y * W + px]);
    return (x & 1) ? v & 255 : v >> 8;
}

TUP_DEVICE int pn_paeth(int a, int b, int c)
{
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the filtered byte at column x (of 3 BPS W) of row y under filter ft
template <int BPS>
TUP_DEVICE int pn_filtered(const uint8_t* u8, const float* f32, size_t plane, int W, int y, int x, int ft)
{
    constexpr int BPP = 3 * BPS;
    const int cur = pn_raw<BPS>(u8, f32, plane, W, y, x);
    if (ft == 0) return cur;
    const int a = (ft != 2 && x >= BPP) ? pn_raw<BPS>(u8, f32, plane, W, y, x - BPP) : 0;
    const int b = (ft != 1 && y > 0) ? pn_raw<BPS>(u8, f32, plane, W, y - 1, x) : 0;
    if (ft == 1) return (cur - a) & 255;
    if (ft == 2) return (cur - b) & 255;
    if (ft == 3) return (cur - ((a + b) >> 1)) & 255;
    const int c = (x >= BPP && y > 0) ? pn_raw<BPS>(u8, f32, plane, W, y - 1, x - BPP) : 0;
    return (cur - pn_paeth(a, b, c)) & 255;
}

// ---- launch 0 ----
template <int BPS>
__global__ __launch_bounds__(PN_THREADS) void png_filter_kernel(const uint8_t* __restrict__ frames_u8, const float* __restrict__ frames_f32,
                                                                int H, int W, uint8_t* __restrict__ filters)
{
    __shared__ int part[PN_THREADS / 64][5];
    const int tid = threadIdx.x, y = blockIdx.x, b = blockIdx.y;
    const size_t plane = (size_t)H * W;
    constexpr int BPP = 3 * BPS;
    const uint8_t* u8 = frames_u8 ? frames_u8 + (size_t)b * plane * BPP : nullptr;
    const float* f32 = frames_f32 ? frames_f32 + (size_t)b * plane * 3 : nullptr;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int x = tid; x < BPP * W; x += PN_THREADS) {
        const int cur = pn_raw<BPS>(u8, f32, plane, W, y, x);
        const int a = x >= BPP ? pn_raw<BPS>(u8, f32, plane, W, y, x - BPP) : 0;
        const int up = y > 0 ? pn_raw<BPS>(u8, f32, plane, W, y - 1, x) : 0;
        const int c = (x >= BPP && y > 0) ? pn_raw<BPS>(u8, f32, plane, W, y - 1, x - BPP) : 0;
        int r;                                                                     // |residual| with the byte read as signed
        r = cur;                              s0 += r < 128 ? r : 256 - r;
        r = (cur - a) & 255;                  s1 += r < 128 ? r : 256 - r;
        r = (cur - up) & 255;                 s2 += r < 128 ? r : 256 - r;
        r = (cur - ((a + up) >> 1)) & 255;    s3 += r < 128 ? r : 256 - r;
        r = (cur - pn_paeth(a, up, c)) & 255; s4 += r < 128 ? r : 256 - r;
    }
    for (int d = 32; d > 0; d >>= 1) {
        s0 += __shfl_down(s0, d); s1 += __shfl_down(s1, d); s2 += __shfl_down(s2, d); s3 += __shfl_down(s3, d); s4 += __shfl_down(s4, d);
    }
    if ((tid & 63) == 0) {
        int* p = part[tid >> 6];
        p[0] = s0; p[1] = s1; p[2] = s2; p[3] = s3; p[4] = s4;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0, best_sum = 0;
        for (int f = 0; f < 5; ++f) {
            const int s = part[0][f] + part[1][f] + part[2][f] + part[3][f];
            if (f == 0 || s < best_sum) { best = f; best_sum = s; }                // a tie keeps the lower filter
        }
        filters[(size_t)b * H + y] = (uint8_t)best;
    }
}

// ---- launches 1 and 3 ----
// `len` <= 32 bits of `val` at bit `pos` of the stream; bit p of the stream is bit p % 32 of word p / 32
TUP_DEVICE void pn_put(uint32_t* bits, int& pos, uint32_t val, int len)
{
    const uint64_t v = (uint64_t)val << (pos & 31);
    if ((uint32_t)v) atomicOr(&bits[pos >> 5], (uint32_t)v);
    if ((uint32_t)(v >> 32)) atomicOr(&bits[(pos >> 5) + 1], (uint32_t)(v >> 32));
    pos += len;
}

// f(byte, run length) for every maximal run that starts in [first, a1); a run that reaches a1 ends at next_start
template <class F>
TUP_DEVICE void pn_runs(const uint8_t* d, int first, int a1, int next_start, F&& f)
{
    int p = first;
    while (p < a1) {
        const int v = d[p];
        int e = p + 1;
        while (e < a1 && d[e] == v) ++e;
        if (e == a1) e = next_start;
        f(v, e - p);
        p = e;
    }
}

// byte i < 29 of signature + IHDR: everything before IHDR's CRC
TUP_DEVICE uint32_t pn_head_plain(int i, int H, int W, uint32_t depth)
{
    if (i < 8) return (uint32_t)(0x0A1A0A0D474E5089ull >> (8 * i)) & 255u;
    if (i < 12) return i == 11 ? 13u : 0u;
    if (i < 16) return (0x52444849u >> (8 * (i - 12))) & 255u;                     // "IHDR"
    if (i < 20) return ((uint32_t)W >> (8 * (19 - i))) & 255u;
    if (i < 24) return ((uint32_t)H >> (8 * (23 - i))) & 255u;
    return i == 24 ? depth : i == 25 ? 2u : 0u;                                    // 8 or 16 bits, colour type 2, deflate, filter method 0, no interlace
}
// byte i < 33 of signature + IHDR
TUP_DEVICE uint32_t pn_head_byte(int i, int H, int W, uint32_t depth)
{
    if (i < 29) return pn_head_plain(i, H, W, depth);
    uint32_t s = 0xFFFFFFFFu;
    for (int j = 12; j < 29; ++j) s = pd_crc_byte(s, pn_head_plain(j, H, W, depth));
    return ((s ^ 0xFFFFFFFFu) >> (8 * (32 - i))) & 255u;
}
// byte i < 28 of what follows the last block's chunk: the IDAT with the Adler-32, then IEND
TUP_DEVICE uint32_t pn_tail_byte(int i, uint32_t adler)
{
    if (i < 4) return i == 3 ? 4u : 0u;
    if (i < 8) return (0x54414449u >> (8 * (i - 4))) & 255u;                       // "IDAT"
    if (i < 12) return (adler >> (8 * (11 - i))) & 255u;
    if (i < 16) {
        uint32_t s = 0xFFFFFFFFu;
        for (int j = 0; j < 4; ++j) s = pd_crc_byte(s, (0x54414449u >> (8 * j)) & 255u);
        for (int j = 0; j < 4; ++j) s = pd_crc_byte(s, (adler >> (8 * (3 - j))) & 255u);
        return ((s ^ 0xFFFFFFFFu) >> (8 * (15 - i))) & 255u;
    }
    if (i < 20) return 0u;
    if (i < 24) return (0x444E4549u >> (8 * (i - 20))) & 255u;                     // "IEND"
    return (0xAE426082u >> (8 * (27 - i))) & 255u;                                 // its CRC
}

// WRITE = false: sizes[b][k] <- the bytes block k adds to the file, partials[b][k] <- its Adler partial.
// WRITE = true: offsets[b][k] is where block k's chunk starts in its image's row of `data`.
template <bool WRITE, int BPS>
__global__ __launch_bounds__(PN_THREADS) void png_block_kernel(const uint8_t* __restrict__ frames_u8, const float* __restrict__ frames_f32,
                                                               int H, int W, int filter, int bb, int N, const uint8_t* __restrict__ filters,
                                                               int* __restrict__ sizes, int* __restrict__ partials,
                                                               const int* __restrict__ offsets, const int* __restrict__ lengths,
                                                               const int* __restrict__ adlers, uint8_t* __restrict__ data, long long capacity)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PnShared& sh = *reinterpret_cast<PnShared*>(smem);
    uint8_t* d = smem + PN_SHARED;                                                 // the block's filtered bytes
    uint32_t* out = reinterpret_cast<uint32_t*>(smem + PN_SHARED + pn_data_bytes(bb));      // WRITE: the chunk, as it goes to memory
    const int tid = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
    if (WRITE && lengths[b] < 0) return;                                           // the file does not fit its row: nothing of it is written

    const int rowlen = 1 + 3 * BPS * W;
    const int L = H * rowlen;                                                      // below 2^31 (tup_png_blocks / tup_png16_blocks)
    const int s0 = k * bb, n = min(bb, L - s0);
    const bool last = k == N - 1;
    const size_t plane = (size_t)H * W;
    const uint8_t* u8 = frames_u8 ? frames_u8 + (size_t)b * plane * 3 * BPS : nullptr;
    const float* f32 = frames_f32 ? frames_f32 + (size_t)b * plane * 3 : nullptr;
    const uint8_t* ft_row = filter == PN_ADAPTIVE ? filters + (size_t)b * H : nullptr;

    for (int i = tid; i < 4 * PN_SYMS; i += PN_THREADS) (&sh.hist[0][0])[i] = 0;
    for (int i = tid; i < PN_SYMS; i += PN_THREADS) sh.lens[i] = 0;
    if (tid == 0) { sh.n_used = 0; sh.body_bits[0] = sh.body_bits[1] = 0; sh.adler[0] = sh.adler[1] = 0; sh.crc = 0; }
    __syncthreads();

    // ---- a. the filtered bytes ----
    {
        uint32_t sa = 0, sb = 0;
        for (int i = tid; i < n; i += PN_THREADS) {
            const uint32_t pos = (uint32_t)(s0 + i);
            const int y = (int)(pos / (uint32_t)rowlen), c = (int)(pos - (uint32_t)y * (uint32_t)rowlen);
            const int ft = ft_row ? ft_row[y] : filter;
            const int v = c == 0 ? ft : pn_filtered<BPS>(u8, f32, plane, W, y, c - 1, ft);
            d[i] = (uint8_t)v;
            sa += (uint32_t)v;
            sb += (uint32_t)(n - i) * (uint32_t)v;                                 // 128 terms below 2^23 each
        }
        if (!WRITE) {
            atomicAdd(&sh.adler[0], sa % PD_ADLER);
            atomicAdd(&sh.adler[1], sb % PD_ADLER);
        }
    }
    __syncthreads();

    // ---- b. runs: the first start in every lane's piece, and where a run that leaves the piece ends ----
    const int per = 4 * ((((n + PN_THREADS - 1) / PN_THREADS + 3) >> 2) | 1);
    const int a0 = min(tid * per, n), a1 = min(a0 + per, n);
    int first = n;
    for (int p = a0; p < a1; ++p)
        if (p == 0 || d[p] != d[p - 1]) { first = p; break; }
    int next_start;
    {
        int cur = 0;
        sh.scan[0][tid] = first;
        __syncthreads();
        for (int s = 1; s < PN_THREADS; s <<= 1) {
            int x = sh.scan[cur][tid];
            if (tid + s < PN_THREADS) x = min(x, sh.scan[cur][tid + s]);
            sh.scan[cur ^ 1][tid] = x;
            cur ^= 1;
            __syncthreads();
        }
        next_start = tid + 1 < PN_THREADS ? sh.scan[cur][tid + 1] : n;
        __syncthreads();
    }

    // ---- c. histograms, code lengths, the bits of every form ----
    {
        int* h = sh.hist[tid >> 6];
        pn_runs(d, first, a1, next_start, [&](int v, int r) {
            const int m = r - 1, q = m / 258, t = m - 258 * q;
            atomicAdd(&h[v], 1 + (t < 3 ? t : 0));
            if (q) atomicAdd(&h[285], q);
            if (t >= 3) {
                int e, x;
                atomicAdd(&h[pd_length_symbol(t, e, x)], 1);
            }
            if (q + (t >= 3)) atomicAdd(&h[PN_DIST_AT], q + (t >= 3));
        });
    }
    __syncthreads();
    for (int i = tid; i < PN_SYMS; i += PN_THREADS) sh.hist[0][i] += sh.hist[1][i] + sh.hist[2][i] + sh.hist[3][i] + (i == 256);      // end of block
    __syncthreads();
    for (int s = tid; s < PD_LIT; s += PN_THREADS) {
        const int r = pd_rank(sh.hist[0], PD_LIT, s);
        if (r >= 0) { sh.sorted[r] = sh.hist[0][s]; sh.order[r] = (uint16_t)s; atomicAdd(&sh.n_used, 1); }
    }
    __syncthreads();
    if (tid == 0) {
        pd_lengths(sh.sorted, sh.order, sh.n_used, 15, sh.count, sh.lens);
        int hlit = PD_LIT;
        while (hlit > 257 && sh.lens[hlit - 1] == 0) --hlit;
        sh.hlit = hlit;
        sh.lens[PN_DIST_AT] = sh.hist[0][PN_DIST_AT] > 0;                          // distance 1 is the one distance: symbol 0, one bit
    }
    __syncthreads();
    const int hlit = sh.hlit;
    for (int i = tid; i <= hlit; i += PN_THREADS) sh.seq[i] = i < hlit ? sh.lens[i] : sh.lens[PN_DIST_AT];      // HDIST = 1
    __syncthreads();
    if (tid == 0) {
        sh.n_cl = pd_run_length_code(sh.seq, hlit + 1, sh.cl_tokens, sh.cl_freq);
        pd_build_lengths(sh.cl_freq, PD_CL, 7, sh.cl_sorted, sh.cl_order, sh.count, sh.cl_lens);
        int hclen = PD_CL;
        while (hclen > 4 && sh.cl_lens[pd_cl_order(hclen - 1)] == 0) --hclen;
        sh.hclen = hclen;
        int hb = 14 + 3 * hclen;
        for (int s = 0; s < PD_CL; ++s) hb += sh.cl_freq[s] * (sh.cl_lens[s] + pd_cl_extra(s));
        sh.header_bits = hb;
    }
    {
        int fixed = 0, dyn = 0;
        for (int s = tid; s < PD_LIT; s += PN_THREADS) {
            const int f = sh.hist[0][s], e = pd_length_extra(s);
            fixed += f * (pd_fixed_length(s) + e);
            dyn += f * (sh.lens[s] + e);
        }
        if (tid == 0) { fixed += 5 * sh.hist[0][PN_DIST_AT]; dyn += sh.lens[PN_DIST_AT] * sh.hist[0][PN_DIST_AT]; }
        if (fixed) atomicAdd(&sh.body_bits[0], fixed);
        if (dyn) atomicAdd(&sh.body_bits[1], dyn);
    }
    __syncthreads();
    // The Huffman form is the fixed one unless the dynamic one has fewer bits; the block is stored unless the Huffman form, with the
    // empty stored block that realigns the stream after every block but the last, has fewer bytes.
    const int bits_fixed = 3 + sh.body_bits[0], bits_dyn = 3 + sh.header_bits + sh.body_bits[1];
    const bool dynamic = bits_dyn < bits_fixed;
    const int bits = dynamic ? bits_dyn : bits_fixed;
    const int huff_bytes = last ? (bits + 7) >> 3 : ((bits + 3 + 7) >> 3) + 4;
    const bool stored = 5 + n <= huff_bytes;
    const int zhdr = k == 0 ? 2 : 0;
    const int payload = zhdr + (stored ? 5 + n : huff_bytes);
    const int chunk = 12 + payload;

    if (!WRITE) {
        if (tid == 0) {
            sizes[(size_t)b * N + k] = chunk + (last ? PN_TAIL : 0);
            partials[(size_t)b * N + k] = (int)((sh.adler[1] % PD_ADLER) << 16 | (sh.adler[0] % PD_ADLER));
        }
        return;
    } else {
        // ---- d. the chunk in LDS, placed so that its words are the destination's words ----
        const long long at = offsets[(size_t)b * N + k];
        if (at < PN_HEAD || at + chunk + (last ? PN_TAIL : 0) > capacity) return;  // not what launch 2 computed from these sizes
        uint8_t* dst = data + (size_t)b * (size_t)capacity + at;
        const int mis = (int)((uintptr_t)dst & 3);
        uint8_t* ob = reinterpret_cast<uint8_t*>(out);
        const int nwords = (mis + chunk + 3) >> 2;
        for (int i = tid; i <= nwords; i += PN_THREADS) out[i] = 0;
        if (!stored) {
            if (!dynamic) {
                // all 288 symbols of the fixed code: 286 and 287 are never sent, but their 8-bit codes come before the 9-bit ones
                for (int s = tid; s < PN_DIST_AT; s += PN_THREADS) sh.lens[s] = (uint8_t)pd_fixed_length(s);
                if (tid == 0) sh.lens[PN_DIST_AT] = 5;
            }
        }
        __syncthreads();
        const int body = mis + 8 + zhdr;                                           // the byte of `out` where the deflate block starts
        if (tid == 0) {
            ob[mis + 0] = (uint8_t)((uint32_t)payload >> 24); ob[mis + 1] = (uint8_t)(payload >> 16);
            ob[mis + 2] = (uint8_t)(payload >> 8); ob[mis + 3] = (uint8_t)payload;
            ob[mis + 4] = 'I'; ob[mis + 5] = 'D'; ob[mis + 6] = 'A'; ob[mis + 7] = 'T';
            if (zhdr) { ob[mis + 8] = 0x78; ob[mis + 9] = 0x01; }
            if (stored) {
                ob[body] = last ? 1 : 0;
                ob[body + 1] = (uint8_t)n; ob[body + 2] = (uint8_t)(n >> 8);
                ob[body + 3] = (uint8_t)~n; ob[body + 4] = (uint8_t)(~n >> 8);
            } else if (!last) {
                ob[body + huff_bytes - 2] = 0xFF; ob[body + huff_bytes - 1] = 0xFF;        // ... 00 00 FF FF
            }
        }
        if (stored) {
            for (int i = tid; i < n; i += PN_THREADS) ob[body + 5 + i] = d[i];
        } else {
            for (int s = tid; s < PD_LIT; s += PN_THREADS) sh.codes[s] = (uint32_t)sh.lens[s] << 16 | pd_code(sh.lens, PN_DIST_AT, s);
            if (tid == 0) sh.codes[PN_DIST_AT] = (uint32_t)sh.lens[PN_DIST_AT] << 16;      // the one distance code is 0
            if (tid < PD_CL) sh.cl_codes[tid] = (uint32_t)sh.cl_lens[tid] << 16 | pd_code(sh.cl_lens, PD_CL, tid);
        }
        __syncthreads();                                                           // the bytes above are in place before any word is OR-ed
        if (!stored) {
            const uint32_t dcode = sh.codes[PN_DIST_AT] & 0xffffu;
            const int dlen = (int)(sh.codes[PN_DIST_AT] >> 16);
            const uint32_t c258 = sh.codes[285];
            int mine = 0;
            pn_runs(d, first, a1, next_start, [&](int v, int r) {
                const int m = r - 1, q = m / 258, t = m - 258 * q;
                mine += (1 + (t < 3 ? t : 0)) * (int)(sh.codes[v] >> 16) + q * ((int)(c258 >> 16) + dlen);
                if (t >= 3) {
                    int e, x;
                    mine += (int)(sh.codes[pd_length_symbol(t, e, x)] >> 16) + e + dlen;
                }
            });
            int total;
            const int before = dg_scan256(mine, sh.scan, tid, total);
            const int head_bits = 3 + (dynamic ? sh.header_bits : 0);
            // the lanes' walks and the histogram count the same tokens; were they ever to disagree, nothing is put outside the chunk
            const bool agree = head_bits + total + (int)(sh.codes[256] >> 16) == bits;
            if (agree && tid == 0) {
                int pos = 8 * body;
                pn_put(out, pos, (last ? 1u : 0u) | (dynamic ? 4u : 2u), 3);
                if (dynamic) {
                    pn_put(out, pos, (uint32_t)(hlit - 257) | 0u << 5 | (uint32_t)(sh.hclen - 4) << 10, 14);
                    for (int i = 0; i < sh.hclen; ++i) pn_put(out, pos, sh.cl_lens[pd_cl_order(i)], 3);
                    for (int i = 0; i < sh.n_cl; ++i) {
                        const int tok = sh.cl_tokens[i], s = tok & 255;
                        const uint32_t c = sh.cl_codes[s];
                        pn_put(out, pos, (c & 0xffffu) | (uint32_t)(tok >> 8) << (c >> 16), (int)(c >> 16) + pd_cl_extra(s));
                    }
                }
            }
            if (agree && tid == PN_THREADS - 1) {
                int pos = 8 * body + head_bits + total;
                pn_put(out, pos, sh.codes[256] & 0xffffu, (int)(sh.codes[256] >> 16));
            }
            int pos = 8 * body + head_bits + before;
            pn_runs(d, first, agree ? a1 : 0, next_start, [&](int v, int r) {
                const int m = r - 1, q = m / 258, t = m - 258 * q;
                const uint32_t c = sh.codes[v];
                pn_put(out, pos, c & 0xffffu, (int)(c >> 16));
                for (int i = 0; i < q; ++i) {
                    pn_put(out, pos, c258 & 0xffffu, (int)(c258 >> 16));
                    pn_put(out, pos, dcode, dlen);
                }
                if (t >= 3) {
                    int e, x;
                    const uint32_t lc = sh.codes[pd_length_symbol(t, e, x)];
                    pn_put(out, pos, (lc & 0xffffu) | (uint32_t)x << (lc >> 16), (int)(lc >> 16) + e);
                    pn_put(out, pos, dcode, dlen);
                } else {
                    for (int i = 0; i < t; ++i) pn_put(out, pos, c & 0xffffu, (int)(c >> 16));
                }
            });
        }
        __syncthreads();

        // the chunk's CRC over type and payload: a piece per lane from state zero, moved to its place by a multiplication
        {
            const int T = 4 + payload;
            const int cper = 4 * ((((T + PN_THREADS - 1) / PN_THREADS + 3) >> 2) | 1);
            const int p0 = min(tid * cper, T), p1 = min(p0 + cper, T);
            if (p1 > p0) {
                uint32_t s = 0;
                for (int i = p0; i < p1; ++i) s = pd_crc_byte(s, ob[mis + 4 + i]);
                atomicXor(&sh.crc, pd_crc_mul(s, pd_crc_shift((uint32_t)(T - p1))));
            }
            __syncthreads();
            if (tid == 0) {
                const uint32_t crc = pd_crc_finish(sh.crc, (uint32_t)T);
                uint8_t* p = ob + mis + 8 + payload;
                p[0] = (uint8_t)(crc >> 24); p[1] = (uint8_t)(crc >> 16); p[2] = (uint8_t)(crc >> 8); p[3] = (uint8_t)crc;
            }
            __syncthreads();
        }

        // out: whole dwords where a word of `out` lies inside the chunk, bytes at its two ends
        {
            uint8_t* base = dst - mis;                                             // 4-byte aligned
            for (int w = tid; w < nwords; w += PN_THREADS) {
                if (4 * w >= mis && 4 * w + 4 <= mis + chunk) {
                    *reinterpret_cast<uint32_t*>(base + 4 * w) = out[w];
                } else {
                    for (int j = max(4 * w, mis); j < min(4 * w + 4, mis + chunk); ++j) base[j] = ob[j];
                }
            }
            if (k == 0 && tid < PN_HEAD) data[(size_t)b * (size_t)capacity + tid] = (uint8_t)pn_head_byte(tid, H, W, 8u * BPS);
            if (last && tid < PN_TAIL) dst[chunk + tid] = (uint8_t)pn_tail_byte(tid, (uint32_t)adlers[b]);
        }
    }
}

int pn_blocks(int H, int W, int bb, int bps)
{
    if (H < 1 || W < 1 || bb < PN_MIN_BLOCK || bb > PN_MAX_BLOCK) return -1;
    const long long L = (long long)H * (1 + 3LL * bps * W);
    if (L >= 0x80000000LL) return -1;
    return (int)((L + bb - 1) / bb);
}
bool pn_frames_ok(const void* u8, const float* f32, int B) { return (!u8) != (!f32) && B >= 1 && B <= 65535; }

// the four launches behind the tup_png_* (BPS = 1) and tup_png16_* (BPS = 2) entries
template <int BPS>
int pn_filters(const void* frames, const float* frames_f32, int B, int H, int W, void* filters, void* stream)
{
    if (pn_blocks(H, W, PN_MAX_BLOCK, BPS) < 1 || !pn_frames_ok(frames, frames_f32, B) || !filters) return (int)hipErrorInvalidValue;
    png_filter_kernel<BPS><<<dim3((unsigned)H, (unsigned)B), dim3(PN_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)frames, frames_f32, H, W, (uint8_t*)filters);
    TUP_CHECK_LAUNCH();
    return 0;
}

template <int BPS>
int pn_sizes(const void* frames, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, const void* filters, int* sizes,
             int* partials, void* stream)
{
    const int N = pn_blocks(H, W, block_bytes, BPS);
    if (N < 1 || !pn_frames_ok(frames, frames_f32, B) || filter < 0 || filter > PN_ADAPTIVE || (filter == PN_ADAPTIVE && !filters) || !sizes ||
        !partials)
        return (int)hipErrorInvalidValue;
    TUP_SET_DYN_LDS((png_block_kernel<false, BPS>), PN_SHARED + pn_data_bytes(PN_MAX_BLOCK));
    png_block_kernel<false, BPS><<<dim3((unsigned)N, (unsigned)B), dim3(PN_THREADS), (size_t)(PN_SHARED + pn_data_bytes(block_bytes)),
                                   reinterpret_cast<hipStream_t>(stream)>>>((const uint8_t*)frames, frames_f32, H, W, filter, block_bytes, N,
                                                                            (const uint8_t*)filters, sizes, partials, nullptr, nullptr, nullptr,
                                                                            nullptr, 0);
    TUP_CHECK_LAUNCH();
    return 0;
}

template <int BPS>
int pn_write(const void* frames, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, const void* filters,
             const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity, void* stream)
{
    const int N = pn_blocks(H, W, block_bytes, BPS);
    if (N < 1 || !pn_frames_ok(frames, frames_f32, B) || filter < 0 || filter > PN_ADAPTIVE || (filter == PN_ADAPTIVE && !filters) || !offsets ||
        !lengths || !adlers || capacity < 0 || capacity > 0x7fffffffLL || (!data && capacity > 0))
        return (int)hipErrorInvalidValue;
    if (capacity == 0) return 0;                                                   // nothing fits: every length is -1 already
    TUP_SET_DYN_LDS((png_block_kernel<true, BPS>), PN_SHARED + pn_data_bytes(PN_MAX_BLOCK) + pn_out_bytes(PN_MAX_BLOCK));
    png_block_kernel<true, BPS><<<dim3((unsigned)N, (unsigned)B), dim3(PN_THREADS),
                                  (size_t)(PN_SHARED + pn_data_bytes(block_bytes) + pn_out_bytes(block_bytes)), reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)frames, frames_f32, H, W, filter, block_bytes, N, (const uint8_t*)filters, nullptr, nullptr, offsets, lengths, adlers,
        (uint8_t*)data, capacity);
    TUP_CHECK_LAUNCH();
    return 0;
}
}  // namespace
