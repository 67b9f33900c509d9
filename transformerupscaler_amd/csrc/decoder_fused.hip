// Inference decoder: decoder_conv1 (64->64, +bias, ReLU) and decoder_conv2 (64->3, +bias) in two launches, without the
// 64-channel map between them ever reaching HBM (reference models/FastTransformer/model.py:228-229,312-313).
//
// decoder_conv2 is linear, so it is evaluated in scatter form:
//     residual(q) = b + sum_{dy,dx} Z_{dy,dx}(q + (dy-1, dx-1)),      Z_{dy,dx}(p) = W2[:, :, dy, dx] . dec(p)
// Each dec pixel needs only its 27 projections (9 taps x 3 channels).  The persistent ping-pong conv (conv_pingpong.h: tile walk,
// halo DMA, K loop and staging are the ones conv_c64_persistent_kernel<4,0,3> uses; this kernel adds decoder_conv2's A fragments,
// the store phase below and a phase loop that counts their loads and stores) computes them in its epilogue, where dec(p) already
// sits in registers:
//   * B operand = the epilogue's packed ReLU'd bf16 words: lane (g, p) holds channels 16g + 8s + j (j = 0..7) of pixel p in
//     pk[4s .. 4s+3], i.e. a valid 16x16x32 B fragment per K-step s = 0, 1 with logical k = 8g + j.  The host packs the
//     decoder_conv2 weight image with its columns permuted the same way (packing.pack_dec2_scatter), so no data moves.
//   * A operand = that image, rows m = 16 dy + 4 c + dx (48 rows, c = 3 / dx = 3 zero): tile dy of the result leaves lane
//     (g = c, p) with Z_{dy, 0..2, c}(p) in its four accumulator registers.  24 MFMAs per wave and tile (the K loop has 288).
//   * dx sum: DPP row shifts inside the 16-pixel groups, the edge lanes of the two groups of a row from each other.  dy sum: the
//     wave holds two dec rows (2w, 2w+1 of the tile, globally even / odd), so output row 2w gets H_1(2w) + H_2(2w+1) here
//     and H_0(2w-1) from the wave above; row 2w+1 gets H_0(2w) + H_1(2w+1) here and H_2(2w+2) from the wave below.
// What crosses a wave boundary goes to HBM and the finishing kernel adds it in a fixed order (no float atomics: a batch
// computes bit-identically to its images one at a time):
//   part   [B][3][H][W]  the wave's own sum for its two rows (becomes residual in place)
//   seamv  [B][3][H][W]  row y's term from the other wave: H_0(y-1) for even y, H_2(y+1) for odd y (one writer per row)
//   cseam  [B][H][tilesX][2][4][4]  raw Z of the tile's first (side 0: dx = 2, to column x-1) and last (side 1: dx = 0,
//                        to column x+1) dec column: [c][dy]
// dec pixels outside the image hold ReLU(bias), not conv2's zero padding, so edge tiles zero them before the second GEMM.
// At scale 2 the only reader of residual is the streaming output tail, which adds the pieces itself in the same order as it reads
// them (tup_decoder_fused_parts_fwd here, tail_stream.hip PARTS): the finishing kernel then does not run.
#include "conv_pingpong.h"

namespace {

constexpr int TH = 8, TW = 32, HALO_W = TW + 2, HALO_H = TH + 2, NPIX_HALO = HALO_H * HALO_W;
constexpr int IN_BYTES = NPIX_HALO * 128;
constexpr int WROWS = 64, WSLAB = WROWS * 128;
constexpr size_t DEC_LDS = (size_t)9 * WSLAB + 2 * (size_t)IN_BYTES + 256;          // + bias
static_assert(DEC_LDS <= 163840, "LDS budget");

__global__ __launch_bounds__(512, 2) void decoder_fused_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, const float* __restrict__ bias,
    const bf16_t* __restrict__ wz, float* __restrict__ part, float* __restrict__ seamv, float* __restrict__ cseam,
    int B, int H, int W, int tilesX, int tilesY)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* w_lds = smem;                              // [9][64 rows][128 B]
    char* in_lds = smem + 9 * WSLAB;                 // [2 groups][IN_BYTES]

    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, p = lane & 15;
    const int total_tiles = tilesX * tilesY * B;
    char* my_in = in_lds + grp * IN_BYTES;

    using Dma = HaloDma<HALO_H, HALO_W, 1>;
    constexpr int NPIECE = Dma::NPIECE;
    const Dma dma(W, tid);
    auto prefetch_tile = [&](const TC& c) { dma.prefetch(x, c.b, c.ty * TH, c.tx * TW, H, W, my_in, tup_zero_line); };

    uint32_t poff[9][2];
    pixel_frag_offsets<3, HALO_W>(poff, my_in, wave, g, p);
    const uint32_t wbase0 = weight_frag_base(w_lds, g, p);

    f32x4 acc[4][4];
    float* bias_lds = reinterpret_cast<float*>(in_lds + 2 * IN_BYTES);
    const uint32_t bias_addr = lds_addr(bias_lds) + (uint32_t)(g * 64);
    // decoder_conv2's A fragments ([dy][K-step s], 24 registers, not resident: the K loop uses 211).  Loaded from L2 at the top of
    // the store phase from inline asm, so that hipcc's waitcnt pass does not see them: it would wait vmcnt(0) for them after the
    // halo DMA, i.e. for the DMA to land before the epilogue starts.  The phase loop waits for them by count instead.
    bf16x8 zf[3][2];
    const uint32_t wz_voff = (uint32_t)(p * 128 + g * 16);
    auto load_zf = [&]() {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const bf16_t* base = wz + dy * 1024;
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(zf[dy][0]) : "v"(wz_voff), "s"(base));
            asm volatile("global_load_dwordx4 %0, %1, %2 offset:64" : "=v"(zf[dy][1]) : "v"(wz_voff), "s"(base));
        }
    };

    // epilogue: dec (bf16, ReLU) -> the 27 projections -> in-wave gather -> 10 stores per wave
    auto store_tile = [&](const TC& c) {
        const int b = c.b, y0 = c.ty * TH + 2 * wave, x0 = c.tx * TW;
        const bool edge = c.ty * TH + TH > H || x0 + TW > W;          // wave-uniform: some dec pixel of the tile is outside
        f32x4 z[4][3];
#pragma unroll
        for (int pg = 0; pg < 4; ++pg) {
            typedef short s16x2 __attribute__((ext_vector_type(2)));
            uint32_t pk[8];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                pk[ct * 2 + 0] = pack_bf16x2(acc[pg][ct][0], acc[pg][ct][1]);
                pk[ct * 2 + 1] = pack_bf16x2(acc[pg][ct][2], acc[pg][ct][3]);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                pk[q] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pk[q]), s16x2{0, 0}));
            if (edge) {
                const bool ok = y0 + (pg >> 1) < H && x0 + (pg & 1) * 16 + p < W;
#pragma unroll
                for (int q = 0; q < 8; ++q) pk[q] = ok ? pk[q] : 0u;
            }
            const bf16x8 b0 = __builtin_bit_cast(bf16x8, u32x4{pk[0], pk[1], pk[2], pk[3]});
            const bf16x8 b1 = __builtin_bit_cast(bf16x8, u32x4{pk[4], pk[5], pk[6], pk[7]});
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                z[pg][dy] = mfma16x16x32(zf[dy][0], b0, f32x4{0.f, 0.f, 0.f, 0.f});
                z[pg][dy] = mfma16x16x32(zf[dy][1], b1, z[pg][dy]);
            }
        }
        // The DPP adds below are inline asm, which hipcc's hazard recognizer does not check against the MFMAs that wrote their
        // operands (an XDL result needs 11 wait states before a VALU reads it): keep the MFMAs above, and wait them out.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 4" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // H[rw][cg][dy] = sum_dx Z_{dy,dx}(x + dx - 1) over this wave's 32 columns (pg = 2 rw + cg)
        float h[2][2][3];
#pragma unroll
        for (int rw = 0; rw < 2; ++rw)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const f32x4 l = z[2 * rw][dy], r = z[2 * rw + 1][dy];
                float v0 = l[1], v1 = r[1];
                TUP_ADD_DPP(v0, l[0], "row_shr:1"); TUP_ADD_DPP(v0, l[2], "row_shl:1"); TUP_ADD_DPP(v0, r[2], "row_shr:15");
                TUP_ADD_DPP(v1, r[0], "row_shr:1"); TUP_ADD_DPP(v1, r[2], "row_shl:1"); TUP_ADD_DPP(v1, l[0], "row_shl:15");
                h[rw][0][dy] = v0; h[rw][1][dy] = v1;
            }
        // Stores through buffer resources (one per image and buffer): a lane without a target gets an offset past the
        // resource's end and the store is dropped, so every wave issues exactly NSTORES store instructions per tile (the
        // counted vmcnt of the phase loop) with no branches around them.
        const bool live = g < 3;                      // lane (g, p) = channel g
        const int plane = H * W, nrec = 3 * plane * 4;
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(part + (size_t)b * 3 * plane, 0, nrec, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(seamv + (size_t)b * 3 * plane, 0, nrec, 0x00020000);
        const int crec = H * tilesX * 128;
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(cseam + (size_t)b * H * tilesX * 32, 0, crec, 0x00020000);
        const int cbase = (g * plane + y0 * W) * 4;   // byte offset of (channel g, row y0, column 0)
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
            const int ox = x0 + cg * 16 + p;
            const bool colok = live && ox < W;
            const int o = cbase + ox * 4, rowb = W * 4;
            // own rows: 2w gets H_1(2w) + H_2(2w+1), 2w+1 gets H_0(2w) + H_1(2w+1)
            const float o0 = h[0][cg][1] + h[1][cg][2], o1 = h[0][cg][0] + h[1][cg][1];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, o0), rp, colok && y0 < H ? o : nrec, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, o1), rp, colok && y0 + 1 < H ? o + rowb : nrec, 0, 0);
            // to the waves above / below: H_2(2w) -> row 2w-1, H_0(2w+1) -> row 2w+2
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, h[0][cg][2]), rs,
                                                  colok && y0 >= 1 && y0 < H ? o - rowb : nrec, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, h[1][cg][0]), rs,
                                                  colok && y0 + 2 < H ? o + 2 * rowb : nrec, 0, 0);
        }
        // tile-edge columns: raw Z of dec column 0 (dx = 2, lane p = 0) and column 31 (dx = 0, lane p = 15), [c][dy] per row
#pragma unroll
        for (int rw = 0; rw < 2; ++rw) {
            const int y = y0 + rw;
            const bool left = p == 0;
            const f32x4 v = left ? f32x4{z[2 * rw][0][2], z[2 * rw][1][2], z[2 * rw][2][2], 0.f}
                                 : f32x4{z[2 * rw + 1][0][0], z[2 * rw + 1][1][0], z[2 * rw + 1][2][0], 0.f};
            const bool ok = live & (y < H) & (left | ((p == 15) & (x0 + TW <= W)));          // no short-circuit branches
            const int off = ((y * tilesX + c.tx) * 2 + (left ? 0 : 1)) * 64 + g * 16;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rc, ok ? off : crec, 0, 0);
        }
    };
    constexpr int NSTORES = 10;                       // store instructions per wave in store_tile

    const TileWalk walk(total_tiles, tilesX, tilesY, grp, true);
    const int my_count = walk.my_count, nphases = walk.nphases;
    const TC c_first = walk.first;

    stage_weights<4, 9>(w_lds, wp);
    stage_bias<4, false>(bias_lds, bias, 0, 64);
    if (grp == 0 && my_count > 0) prefetch_tile(c_first);
    __syncthreads();
    TC c_done = c_first, c_next = c_first;
    if (grp == 0) walk.advance(c_next);

    for (int ph = 0; ph < nphases; ++ph) {
        const int k = ph >> 1;
        if ((ph & 1) == grp) {
            if (k < my_count) k_loop<4, 9>(acc, poff, wbase0, bias_addr);
        } else {
            const int done = grp == 0 ? k : k - 1;
            const int nxt = done + 1;
            const bool store = done >= 0 && done < my_count;
            const bool fetch = nxt < my_count;
            if (store) load_zf();
            if (fetch) prefetch_tile(c_next);
            if (store) {
                // zf is older than every DMA piece, and each wave issues at least NPIECE - 1 of those
                if (fetch) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPIECE - 1) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                store_tile(c_done);
                // the DMA (issued first) must have landed before the barrier, the stores after it need not
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTORES) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            c_done = c_next;
            walk.advance(c_next);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// residual = bias + part + seamv + the tile-edge column terms, in that order (in place over part).  One workgroup row per image
// row (blockIdx.y = b * H + y): no 64-bit index division per pixel; V = 4 consecutive pixels per thread (16-byte accesses) when
// W % 4 == 0.
template <int V>
__global__ __launch_bounds__(256) void decoder_finish_kernel(
    float* __restrict__ res, const float* __restrict__ seamv, const float* __restrict__ cseam, const float* __restrict__ bias,
    int H, int W, int tilesX)
{
    typedef float fv __attribute__((ext_vector_type(V)));
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (x0 >= W) return;
    const int row = blockIdx.y, b = row / H, y = row - b * H;
    const size_t plane = (size_t)H * W;
    const int ys = (y & 1) ? y + 1 : y - 1;           // the dec row whose wave wrote seamv for this row
    const bool has_seam = ys >= 0 && ys < H;
    const size_t o0 = (size_t)b * 3 * plane + (size_t)y * W + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = o0 + c * plane;
        fv v = *reinterpret_cast<const fv*>(res + o);
        const fv sv = has_seam ? *reinterpret_cast<const fv*>(seamv + o) : fv{};
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int xq = x0 + e;
            float t = bias[c] + v[e];
            if (has_seam) t += sv[e];
            // column 31 of a tile takes the next tile's column 0 (side 0), column 0 the previous tile's column 31 (side 1)
            int ctile = -1, side = 0;
            if ((xq & 31) == 31 && xq + 1 < W) { ctile = (xq >> 5) + 1; side = 0; }
            else if ((xq & 31) == 0 && xq > 0) { ctile = (xq >> 5) - 1; side = 1; }
            if (ctile >= 0) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int yy = y + dy - 1;
                    if (yy >= 0 && yy < H) t += cseam[((((size_t)b * H + yy) * tilesX + ctile) * 2 + side) * 16 + c * 4 + dy];
                }
            }
            v[e] = t;
        }
        *reinterpret_cast<fv*>(res + o) = v;
    }
}

}  // namespace

namespace {
// decoder_fused_kernel alone: part, seamv and cseam are left in HBM as the header of this file describes them
int launch_decoder_parts(const void* x, const void* w1, const float* b1, const void* wz, float* part, float* seamv, float* cseam,
                         int B, int H, int W, void* stream)
{
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    const long long nt = (long long)tilesX * tilesY * B;
    // buffer-resource byte offsets are 32-bit and per image
    if (nt > 0x7fffffffLL || (long long)H * W * 12 > 0x7fffffffLL || (long long)H * tilesX * 128 > 0x7fffffffLL)
        return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TUP_SET_DYN_LDS(decoder_fused_kernel, DEC_LDS);
    const int grid = (int)(nt < 256 ? nt : 256);                 // one workgroup per CU
    decoder_fused_kernel<<<dim3(grid), dim3(512), DEC_LDS, s>>>((const bf16_t*)x, (const bf16_t*)w1, b1, (const bf16_t*)wz, part,
                                                                 seamv, cseam, B, H, W, tilesX, tilesY);
    TUP_CHECK_LAUNCH();
    return 0;
}
}  // namespace

// combined bf16 NHWC [B][H][W][64]; w1 bf16 [1][1][9][64][64] + b1 fp32 [64] (tup_conv3x3_c64_fwd's out_mode 0 packing);
// wz bf16 [48][64] (decoder_conv2 in scatter form, packing.pack_dec2_scatter); b2 fp32 [3];
// seamv fp32 [B][3][H][W], cseam fp32 [B][H][ceil(W/32)][32] workspaces; out fp32 [B][3][H][W].
extern "C" int tup_decoder_fused_fwd(const void* x, const void* w1, const float* b1, const void* wz, const float* b2,
                                     float* seamv, float* cseam, float* out, int B, int H, int W, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int tilesX = (W + TW - 1) / TW;
    if (const int err = launch_decoder_parts(x, w1, b1, wz, out, seamv, cseam, B, H, W, stream)) return err;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((long long)B * H > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    if (W % 4 == 0)
        decoder_finish_kernel<4><<<dim3((unsigned)((W / 4 + 255) / 256), (unsigned)(B * H)), dim3(256), 0, s>>>(out, seamv, cseam, b2, H, W, tilesX);
    else
        decoder_finish_kernel<1><<<dim3((unsigned)((W + 255) / 256), (unsigned)(B * H)), dim3(256), 0, s>>>(out, seamv, cseam, b2, H, W, tilesX);
    TUP_CHECK_LAUNCH();
    return 0;
}

// The fused kernel without the finishing launch: part, seamv fp32 [B][3][H][W] and cseam fp32 [B][H][ceil(W/32)][32] stay unfinished
// (rows of seamv without a seam partner and the pad words of cseam are not written).  tup_tail_stream_r2_parts_fwd /
// tup_tail_stream_r2_resize_parts_fwd (tail_stream.hip) add them, with decoder_conv2's bias, where they read the plane.
extern "C" int tup_decoder_fused_parts_fwd(const void* x, const void* w1, const float* b1, const void* wz,
                                           float* part, float* seamv, float* cseam, int B, int H, int W, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return launch_decoder_parts(x, w1, b1, wz, part, seamv, cseam, B, H, W, stream);
}
