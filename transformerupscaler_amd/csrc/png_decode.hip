// PNG files (8 bits a sample, colour types 0, 2, 3, 4, 6, no interlace) of a whole batch decoded on the GPU: `ops.png_decode`, DESIGN 7n.
// Pixel for pixel what Pillow's Image.open(file).convert("RGB") returns; tests/_png_decode_ref.py states it in Python.
//
// The host walks the chunks (ops.png_parse) and uploads, once, a PngImage record per image followed by every image's IDAT payloads
// joined without chunk framing (one zlib stream), each at a multiple of 16 bytes.  All images share H and W.  Two launches:
//   1. png_inflate_kernel   one wave per image.  LDS holds the decode tables (png_inflate.h), a window of PNG_WIN input bytes and a
//                           64 KB ring of output.  The ring holds deflate's 32 KB window: a match reads the ring, never memory the
//                           wave has just written.  Every 32 KB the older half goes to the image's workspace in whole dwords and
//                           into the Adler-32 (per-lane sums d and (n - i) d, png_deflate.h's pd_adler_append).  Matches are copied
//                           64 bytes a step, source index modulo the distance.  WAVE = false: png_inflate.h's plain walk, one
//                           token a round, every lane holding the same reader state.  WAVE = true: lane i decodes the token that
//                           would begin at bit p + i; the true chain is followed from lane 0 by lane reads; a prefix sum of the
//                           on-chain lanes' output lengths places their tokens; literals are stored by their own lanes, matches
//                           are executed in order, each across the wave.  Headers and stored blocks take the plain path.
//   2. png_finish_kernel    one workgroup of PF_WAVES waves per image undoes the filters, maps channels or palette to RGB and writes
//                           uint8 [B][H][W][3] or fp32 [B][3][H][W] = byte / 255.  A wave takes a band of 64 rows; lane j works on
//                           pixel x = t - j at step t, so its left neighbour is its own last result and its upper neighbours are
//                           lane j - 1's last two.  Lane 0's upper row is the band above's last row, which that band's lane 63
//                           leaves in a row buffer of the workspace; the waves run their bands two 64-step chunks apart with a
//                           barrier per chunk, which orders those stores and loads.  A filter byte above 4 sets the status.
// Status (png_inflate.h, PiStatus): launch 1 stores 0 or the first error of the stream, launch 2 replaces 0 or a bad Adler-32 by a
// bad filter byte.  A damaged stream reads nothing outside its own input range and writes nothing outside its workspace and frame:
// every token is checked against stream_bytes before it is written.  All global writes are ordinary vector stores.
#include "common.h"
#include "png_inflate.h"

struct PngImage {
    int off, len;                 // the zlib stream: bytes from the start of the stream area (a multiple of 16), length
    int color_type, channels;     // PNG's colour type; bytes per pixel of the filtered stream
    uint8_t palette[768];         // colour type 3: PLTE, zero-filled
};
static_assert(sizeof(PngImage) == 784, "image record = 784 bytes (the host packs it)");

namespace {
constexpr int PNG_WIN = 4096;                                // input bytes staged in LDS
constexpr int PNG_WIN_WORDS = PNG_WIN / 4 + 8;
constexpr uint32_t PNG_RING = 65536, PNG_HALF = 32768;
constexpr int PF_WAVES = 16;

TUP_DEVICE uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

TUP_DEVICE uint64_t uniform64(uint64_t v)                    // a value every lane holds, moved to scalar registers
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)hi << 32 | lo;
}

// 64 stream bits from any bit position, out of the LDS window
struct PngSrc {
    const uint8_t* in;
    uint32_t n, wbase;
    uint32_t* win;
    int lane;
    TUP_DEVICE uint64_t nbits() const { return 8ull * n; }
    TUP_DEVICE void refill(uint32_t base)
    {
        wbase = base;
        for (int i = lane; i < PNG_WIN_WORDS; i += 64) {
            const uint32_t bo = base + 4u * (uint32_t)i;
            uint32_t v = 0;
            if (bo < n) {                                    // the dword lies inside the image's 16-byte-padded area
                v = *reinterpret_cast<const uint32_t*>(in + bo);
                if (n - bo < 4) v &= (1u << (8 * (n - bo))) - 1u;
            }
            win[i] = v;
        }
        __syncthreads();
    }
    TUP_DEVICE void ensure(uint64_t pos)                     // pos: the same in every lane
    {
        const uint32_t byte = (uint32_t)(pos >> 3);
        if (byte < wbase || byte - wbase > (uint32_t)(PNG_WIN - 16)) {
            __syncthreads();
            refill(byte & ~15u);
        }
    }
    TUP_DEVICE uint64_t peek_window(uint64_t pos) const      // up to 63 bits after an ensured position
    {
        const uint32_t d = (uint32_t)(pos >> 5) - (wbase >> 2), s = (uint32_t)pos & 31u;
        const uint64_t lo = (uint64_t)win[d] | ((uint64_t)win[d + 1] << 32);
        return s ? (lo >> s) | ((uint64_t)win[d + 2] << (64 - s)) : lo;
    }
    TUP_DEVICE uint64_t peek(uint64_t pos) { ensure(pos); return peek_window(pos); }
};

// the output: a 64 KB ring in LDS, flushed to the workspace 32 KB at a time
struct PngSink {
    uint32_t* ring32;
    const uint8_t* in;
    uint8_t* ws;
    uint32_t flushed, A, B;
    int lane;
    TUP_DEVICE uint8_t* ring() const { return reinterpret_cast<uint8_t*>(ring32); }
    TUP_DEVICE void lit(uint32_t o, int v)
    {
        if (lane == 0) ring()[o & (PNG_RING - 1)] = (uint8_t)v;
        __builtin_amdgcn_wave_barrier();
    }
    TUP_DEVICE void match(uint32_t o, int len, int dist)
    {
        uint8_t* r = ring();
        for (int k = lane; k < len; k += 64) {
            const int q = dist >= len ? k : k % dist;        // every source byte lies before o
            r[(o + (uint32_t)k) & (PNG_RING - 1)] = r[(o - (uint32_t)dist + (uint32_t)q) & (PNG_RING - 1)];
        }
        __builtin_amdgcn_wave_barrier();
    }
    TUP_DEVICE void stored(uint32_t o, uint64_t byte, uint32_t n)
    {
        uint8_t* r = ring();
        for (uint32_t k = (uint32_t)lane; k < n; k += 64) r[(o + k) & (PNG_RING - 1)] = in[(size_t)byte + k];
        __builtin_amdgcn_wave_barrier();
    }
    TUP_DEVICE void flush(uint32_t nbytes)
    {
        __builtin_amdgcn_wave_barrier();
        const uint32_t nd = (nbytes + 3) >> 2;
        uint64_t a = 0, b = 0;
        for (uint32_t k = (uint32_t)lane; k < nd; k += 64) {
            const uint32_t v = ring32[((flushed >> 2) + k) & (PNG_RING / 4 - 1)];
            *reinterpret_cast<uint32_t*>(ws + (size_t)flushed + 4 * (size_t)k) = v;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = 4 * k + j, d = (v >> (8 * j)) & 255u;
                if (i < nbytes) { a += d; b += (uint64_t)(nbytes - i) * d; }
            }
        }
        const uint32_t sa = wave_sum((uint32_t)(a % PD_ADLER)) % PD_ADLER, sb = wave_sum((uint32_t)(b % PD_ADLER)) % PD_ADLER;
        pd_adler_append(A, B, sb << 16 | sa, nbytes);
        flushed += nbytes;
    }
    TUP_DEVICE void advance(uint32_t o)
    {
        while (o - flushed >= PNG_HALF) flush(PNG_HALF);
    }
    TUP_DEVICE uint32_t finish(uint32_t o)
    {
        if (o > flushed) flush(o - flushed);
        return B << 16 | A;
    }
};

// the tokens of one Huffman block, up to 64 a round
struct PngWaveWalk {
    TUP_DEVICE int operator()(const PiTables& t, PngSrc& src, PngSink& sink, uint64_t& pos, uint32_t& o, uint32_t total) const
    {
        const uint64_t nbits = src.nbits();
        const int lane = src.lane;
        for (;;) {
            pos = uniform64(pos);                            // the round's control flow is scalar
            o = (uint32_t)__builtin_amdgcn_readfirstlane((int)o);
            src.ensure(pos);
            const uint64_t mine = pos + (uint64_t)lane;
            const PiToken k = pi_token(t, src.peek_window(mine), nbits > mine ? nbits - mine : 0);
            const int ends = k.err || k.kind == 2;
            // the chain of true token starts from lane 0, by scalar lane reads; a link of 0 ends it
            const int link = ends ? 0 : k.used;
            int cur = 0, last = 0;
            bool ended = false;
            uint64_t chain = 0;
            while (cur < 64) {
                chain |= 1ull << cur;
                last = cur;
                const int step = __builtin_amdgcn_readlane(link, cur);
                if (!step) { ended = true; break; }
                cur += step;
            }
            const bool on = (chain >> lane) & 1ull;
            const uint32_t outlen = on && !ends ? (k.kind == 0 ? 1u : (uint32_t)k.len) : 0u;
            uint32_t incl = outlen;                          // the on-chain lanes hold the round's tokens in stream order
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = (uint32_t)__shfl_up((int)incl, d);
                if (lane >= d) incl += u;
            }
            const uint32_t at = o + (incl - outlen);         // no overflow: o <= total < 2^31 and a round adds at most 64 * 258
            int fail = 0;
            if (on && ends) fail = k.err;
            else if (on && k.kind == 0) fail = at >= total ? PI_OUTPUT_LONG : 0;
            else if (on) fail = (uint32_t)k.dist > at ? PI_BAD_DISTANCE : (uint32_t)k.len > total - at ? PI_OUTPUT_LONG : 0;
            const uint64_t failed = __ballot(fail != 0);
            if (failed) return __builtin_amdgcn_readlane(fail, __builtin_ctzll(failed));
            if (on && !ends && k.kind == 0) sink.ring()[at & (PNG_RING - 1)] = (uint8_t)k.value;
            __builtin_amdgcn_wave_barrier();
            uint64_t matches = __ballot(on && !ends && k.kind == 1);
            while (matches) {
                const int l = __builtin_ctzll(matches);
                matches &= matches - 1;
                sink.match((uint32_t)__builtin_amdgcn_readlane((int)at, l), __builtin_amdgcn_readlane(k.len, l), __builtin_amdgcn_readlane(k.dist, l));
            }
            o += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            sink.advance(o);
            if (ended) {                                     // an end of block (errors have returned)
                pos += (uint64_t)(last + __builtin_amdgcn_readlane(k.used, last));
                return PI_OK;
            }
            pos += (uint64_t)cur;
        }
    }
};

template <bool WAVE>
__global__ __launch_bounds__(64) void png_inflate_kernel(const PngImage* __restrict__ records, const uint8_t* __restrict__ streams,
                                                         long long streams_bytes, int H, int W, uint8_t* __restrict__ workspace,
                                                         long long ws_bytes, long long stream_room, int* __restrict__ status)
{
    __shared__ uint32_t ring32[PNG_RING / 4];
    __shared__ PiTables tables;
    __shared__ uint32_t win[PNG_WIN_WORDS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const PngImage* rec = records + b;
    const int off = rec->off, len = rec->len, ch = rec->channels;
    const long long total = ch >= 1 && ch <= 4 ? (long long)H * (1 + (long long)ch * W) : -1;
    int st;
    if (off < 0 || (off & 15) || len < 2 || (long long)off + len > streams_bytes || total < 0 || total > stream_room) {
        st = PI_INPUT_EXHAUSTED;                             // a record the host would not have written: nothing is touched
    } else {
        PngSrc src = {streams + off, (uint32_t)len, 0u, win, lane};
        PngSink sink = {ring32, streams + off, workspace + (size_t)b * (size_t)ws_bytes, 0u, 1u, 0u, lane};
        src.refill(0);
        if (WAVE) st = pi_inflate(tables, src, sink, PngWaveWalk(), (uint32_t)total, lane, 64);
        else st = pi_inflate(tables, src, sink, PiTokenWalk(), (uint32_t)total, lane, 64);
    }
    if (lane == 0) status[b] = st;
}

// one band of 64 rows a wave; see the head of the file
template <int BPP>
TUP_DEVICE int png_unfilter_image(const uint8_t* ws, uint32_t* carry, int H, int W, int color_type,
                                  const uint8_t* pal, uint8_t* __restrict__ out_u8, float* __restrict__ out_f32)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t stride = 1 + (size_t)BPP * W, hw = (size_t)H * W;
    const int nbands = (H + 63) >> 6, nchunks = (W + 63 + 63) >> 6;       // steps t = 0 .. W + 62
    int bad = 0;
    for (int first = 0; first < nbands; first += PF_WAVES) {
        const int band = first + wv, row = band * 64 + lane;
        const int waves = nbands - first < PF_WAVES ? nbands - first : PF_WAVES;
        const bool live = band < nbands && row < H;
        const uint8_t* rp = ws + (size_t)(live ? row : 0) * stride;
        int ft = 0;
        if (live) {
            ft = rp[0];
            if (ft > 4) { bad = 1; ft = 0; }
        }
        const uint32_t* cin = carry + (size_t)((band + 1) & 1) * W;      // the band above's last row
        uint32_t* cout = carry + (size_t)(band & 1) * W;
        uint32_t left = 0, upleft = 0, mine = 0;
        for (int c = 0; c < nchunks + 2 * (waves - 1); ++c) {
            const int cc = c - 2 * wv;
            if (band < nbands && cc >= 0 && cc < nchunks) {
                const int x0 = cc * 64;
                uint32_t cv = 0;
                if (band > 0 && x0 + lane < W) cv = cin[x0 + lane];
                for (int s = 0; s < 64; ++s) {
                    const int x = x0 + s - lane;
                    uint32_t up = (uint32_t)__shfl_up((int)mine, 1);
                    const uint32_t above = (uint32_t)__shfl((int)cv, s);
                    if (lane == 0) up = above;
                    uint32_t px = 0;
                    if (live && x >= 0 && x < W) {
                        if (x == 0) left = upleft = 0;
                        const uint8_t* p = rp + 1 + (size_t)x * BPP;
#pragma unroll
                        for (int k = 0; k < BPP; ++k)
                            px |= (uint32_t)pi_unfilter_byte(ft, p[k], (left >> (8 * k)) & 255, (up >> (8 * k)) & 255, (upleft >> (8 * k)) & 255) << (8 * k);
                        left = px;
                        if (lane == 63) cout[x] = px;
                        int R = px & 255, G = R, Bl = R;
                        if (BPP >= 3) { G = (px >> 8) & 255; Bl = (px >> 16) & 255; }
                        else if (color_type == 3) { G = pal[3 * R + 1]; Bl = pal[3 * R + 2]; R = pal[3 * R]; }
                        const size_t i = (size_t)row * W + x;
                        if (out_u8) {
                            uint8_t* d = out_u8 + i * 3;
                            d[0] = (uint8_t)R; d[1] = (uint8_t)G; d[2] = (uint8_t)Bl;
                        } else {                                                 // tup_u8hwc_to_f32chw's rule
                            float* d = out_f32 + i;
                            d[0] = (float)R / 255.0f; d[hw] = (float)G / 255.0f; d[2 * hw] = (float)Bl / 255.0f;
                        }
                    }
                    upleft = up;
                    mine = px;
                }
            }
            __syncthreads();
        }
    }
    return bad;
}

__global__ __launch_bounds__(PF_WAVES * 64) void png_finish_kernel(const PngImage* __restrict__ records, uint8_t* workspace,
                                                                  long long ws_bytes, long long stream_room, int H, int W,
                                                                  uint8_t* __restrict__ out_u8, float* __restrict__ out_f32,
                                                                  int* __restrict__ status)
{
    __shared__ uint8_t pal[768];
    const int b = blockIdx.x;
    const PngImage* rec = records + b;
    const int ch = rec->channels, ct = rec->color_type;
    if (ch < 1 || ch > 4 || (long long)H * (1 + (long long)ch * W) > stream_room) return;      // launch 1 has set the status
    for (int i = threadIdx.x; i < 768; i += PF_WAVES * 64) pal[i] = rec->palette[i];
    __syncthreads();
    const uint8_t* ws = workspace + (size_t)b * (size_t)ws_bytes;
    uint32_t* carry = reinterpret_cast<uint32_t*>(workspace + (size_t)b * (size_t)ws_bytes + (size_t)stream_room);
    const size_t hw = (size_t)H * W;
    uint8_t* o8 = out_u8 ? out_u8 + (size_t)b * hw * 3 : nullptr;
    float* o32 = out_f32 ? out_f32 + (size_t)b * hw * 3 : nullptr;
    int bad;
    if (ch == 1) bad = png_unfilter_image<1>(ws, carry, H, W, ct, pal, o8, o32);
    else if (ch == 2) bad = png_unfilter_image<2>(ws, carry, H, W, ct, pal, o8, o32);
    else if (ch == 3) bad = png_unfilter_image<3>(ws, carry, H, W, ct, pal, o8, o32);
    else bad = png_unfilter_image<4>(ws, carry, H, W, ct, pal, o8, o32);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0 && bad && (status[b] == PI_OK || status[b] == PI_BAD_ADLER)) status[b] = PI_BAD_FILTER;
}

// the workspace of one image: the filtered stream of `channels` bytes a pixel, then two rows of packed pixels; both multiples of 16
bool png_geometry(int H, int W, int channels, long long& stream_room, long long& ws)
{
    if (H < 1 || W < 1 || channels < 1 || channels > 4 || (long long)H * (1 + 4ll * W) >= (1ll << 31)) return false;
    stream_room = ((long long)H * (1 + (long long)channels * W) + 15) & ~15ll;
    ws = stream_room + ((8ll * W + 15) & ~15ll);
    return ws < (1ll << 31);
}
}  // namespace

// The bytes of workspace one image needs (what sizes `workspace`), or -1 for what the decoder refuses: H or W below 1, channels (the
// most bytes per pixel of any image of the batch) outside 1..4, H (1 + 4 W) or the workspace itself of 2^31 or more.
extern "C" int tup_png_decode_workspace(int H, int W, int channels)
{
    long long room, ws;
    return png_geometry(H, W, channels, room, ws) ? (int)ws : -1;
}

// Launch 1: the filtered stream of every image -> its workspace, status int32 [B] <- 0 or the stream's first error.  walk 0: a token a
// round; 1: a wave of token candidates a round.
extern "C" int tup_png_decode_inflate(const void* records, const void* streams, long long streams_bytes, int B, int H, int W, int channels,
                                      int walk, void* workspace, long long ws_bytes, int* status, void* stream)
{
    long long room, ws;
    if (!png_geometry(H, W, channels, room, ws) || ws != ws_bytes || B < 1 || B > 65535 || streams_bytes < 0 || (walk != 0 && walk != 1))
        return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (walk)
        png_inflate_kernel<true><<<dim3((unsigned)B), dim3(64), 0, s>>>((const PngImage*)records, (const uint8_t*)streams, streams_bytes, H, W,
                                                                       (uint8_t*)workspace, ws_bytes, room, status);
    else
        png_inflate_kernel<false><<<dim3((unsigned)B), dim3(64), 0, s>>>((const PngImage*)records, (const uint8_t*)streams, streams_bytes, H, W,
                                                                        (uint8_t*)workspace, ws_bytes, room, status);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Launch 2: exactly one of out_u8 (uint8 [B][H][W][3], RGB) and out_f32 (fp32 [B][3][H][W] = byte / 255) <- the pixels; status
// <- a bad filter byte where the stream itself was sound.
extern "C" int tup_png_decode_finish(const void* records, void* workspace, long long ws_bytes, int B, int H, int W, int channels, void* out_u8,
                                     float* out_f32, int* status, void* stream)
{
    long long room, ws;
    if (!png_geometry(H, W, channels, room, ws) || ws != ws_bytes || B < 1 || B > 65535 || (out_u8 == nullptr) == (out_f32 == nullptr))
        return (int)hipErrorInvalidValue;
    png_finish_kernel<<<dim3((unsigned)B), dim3(PF_WAVES * 64), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const PngImage*)records, (uint8_t*)workspace, ws_bytes, room, H, W, (uint8_t*)out_u8, out_f32, status);
    TUP_CHECK_LAUNCH();
    return 0;
}
