// 3x3 same-pad convolution with 64 input channels as an implicit GEMM on MFMA (gfx950).
//
// Stands in for the aten conv2d call sites of the reference:
//   conv2            models/FastTransformer/model.py:204,252   (64->64, +bias, ReLU)
//   up1 convs        models/FastTransformer/utils.py:62,74,83  (64->64*r*r, +bias) + PixelShuffle(r) utils.py:63,75,84
//   up1_conv         models/FastTransformer/utils.py:32-40     (64->3, no bias, ReLU)
//   decoder_conv1/2  models/FastTransformer/model.py:228-229,312-313
//
// Layout: activations NHWC bf16 (128 B per pixel); weights pre-packed on the host to
// [ntile][tap][n_local][cin] bf16 so that one (ntile, tap) slab is contiguous.  One
// workgroup = 4 waves = an 8x32-pixel output tile; the (8+2)x(32+2) halo tile is staged
// once into LDS (XOR-swizzled 128-B rows) and reused by all 9 taps and all cout tiles
// (for the up-convs the PixelShuffle sub-pixel index IS the cout tile, so every tile
// iteration writes whole 128-B NHWC pixels of the shuffled image -- the shuffle is free).
// MFMA operands: A = weights (rows = cout), B = pixels (cols), v_mfma_f32_16x16x32_bf16,
// so a lane ends up with 16 consecutive output channels of one pixel (32-B stores).
#include "conv_pingpong.h"
#include <stdlib.h>

namespace {

constexpr int TH = 8, TW = 32;
constexpr int in_tile_bytes(int ks) { return (TH + ks - 1) * (TW + ks - 1) * 128; }

enum { OUT_NHWC_BF16 = 0, OUT_PLANAR_F32 = 1 };

template <int CT, int OUT_MODE, int KS>
__global__ __launch_bounds__(256, (CT <= 4 && KS == 3) ? 2 : 1) void conv3x3_c64_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, const float* __restrict__ bias,
    const bf16_t* __restrict__ add, const bf16_t* __restrict__ mask,
    void* __restrict__ out, int H, int W, int ntiles, int r, int cout_valid, int relu,
    int tilesX, int tilesY, int in_r)
{
    constexpr int PADK = KS / 2, HALO_W = TW + KS - 1, HALO_H = TH + KS - 1, NPIX_HALO = HALO_H * HALO_W;
    constexpr int NTAPS = KS * KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* in_lds = smem;
    char* w_lds = smem + in_tile_bytes(KS);
    constexpr int WROWS = CT * 16;            // weight rows per (ntile, tap) slab
    constexpr int WSLAB = WROWS * 128;        // bytes
    constexpr int WCH = WROWS * 8;            // 16-byte chunks per slab
    constexpr int WREGS = (WCH + 255) / 256;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, p = lane & 15;
    int bid = blockIdx.x;
    const int tx = bid % tilesX; bid /= tilesX;
    const int ty = bid % tilesY;
    const int b = bid / tilesY;
    const int ty0 = ty * TH, tx0 = tx * TW;

    // ---- stage the haloed input tile (zero outside the image).  With in_r > 1 the logical input has
    // 64*in_r^2 channels stored pixel-shuffled as [B][H*in_r][W*in_r][64]; chunk ci = sub-pixel (si, sj)
    // (the gradient of an Upsampler conv output, read back through PixelShuffle^-1) ----
    const int nci = in_r * in_r;
    const int Hin = H * in_r, Win = W * in_r;
    const bf16_t* xb = x + (size_t)b * Hin * Win * 64;
    // All of a thread's halo loads are issued before any is stored (unconditional loads from a clamped address, zeroed at
    // the store): the rolled load -> store loop paid one global round trip per iteration, eleven per staged chunk.
    constexpr int NSI = (NPIX_HALO * 8 + 255) / 256;
    auto stage_input = [&](int ci) {
        const int si = ci / in_r, sj = ci - si * in_r;
        u32x4 v[NSI];
        auto pos = [&](int idx, int& q, int& c, size_t& off) -> bool {
            q = idx >> 3; c = idx & 7;
            const int yy = q / HALO_W, xx = q - yy * HALO_W;
            const int iy = ty0 - PADK + yy, ix = tx0 - PADK + xx;
            const bool ok = idx < NPIX_HALO * 8 && iy >= 0 && iy < H && ix >= 0 && ix < W;
            off = ok ? ((size_t)(iy * in_r + si) * Win + (ix * in_r + sj)) * 64 + c * 8 : 0;
            return ok;
        };
#pragma unroll
        for (int k = 0; k < NSI; ++k) {
            int q, c; size_t off;
            pos(tid + k * 256, q, c, off);
            v[k] = *reinterpret_cast<const u32x4*>(xb + off);
        }
#pragma unroll
        for (int k = 0; k < NSI; ++k) {
            const int idx = tid + k * 256;
            int q, c; size_t off;
            const bool ok = pos(idx, q, c, off);
            if (idx < NPIX_HALO * 8) *reinterpret_cast<u32x4*>(in_lds + swz128(q, c)) = ok ? v[k] : u32x4{0u, 0u, 0u, 0u};
        }
    };
    stage_input(0);

    u32x4 wreg[WREGS];
    auto wload = [&](int it) {
#pragma unroll
        for (int u = 0; u < WREGS; ++u) {
            const int idx = tid + u * 256;
            if (idx < WCH) wreg[u] = *reinterpret_cast<const u32x4*>(wp + (size_t)it * WROWS * 64 + idx * 8);
        }
    };
    auto wstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < WREGS; ++u) {
            const int idx = tid + u * 256;
            if (idx < WCH) *reinterpret_cast<u32x4*>(w_lds + buf * WSLAB + swz128(idx >> 3, idx & 7)) = wreg[u];
        }
    };

    // halo index of this lane's pixel for each of the wave's 4 pixel groups (tap (0,0) corner)
    int qb[4];
#pragma unroll
    for (int pg = 0; pg < 4; ++pg) qb[pg] = (2 * wave + (pg >> 1)) * HALO_W + (pg & 1) * 16 + p;

    f32x4 acc[4][CT], bv[CT];
    const int total = ntiles * nci * NTAPS;
    wload(0);
    wstore(0);
    __syncthreads();

    for (int it = 0; it < total; ++it) {
        const int tap = it % NTAPS, chunk_it = it / NTAPS;
        const int ci = chunk_it % nci, nt = chunk_it / nci;
        const int buf = it & 1;
        if (tap == 0 && it > 0 && nci > 1) {      // next input-channel chunk (all waves are past the last barrier)
            stage_input(ci);
            __syncthreads();
        }
        if (it + 1 < total) wload(it + 1);
        if (tap == 0 && ci == 0) {
#pragma unroll
            for (int pg = 0; pg < 4; ++pg)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[pg][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {       // bias of this lane's channels, one vector load per cout tile
                bv[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (bias) {
                    if constexpr (OUT_MODE == OUT_NHWC_BF16) bv[ct] = *reinterpret_cast<const f32x4*>(bias + nt * 64 + g * 16 + ct * 4);
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const int co = 16 * ct + 4 * g + e; bv[ct][e] = co < cout_valid ? bias[co] : 0.f; }
                    }
                }
            }
        }
        const int dy = tap / KS, dx = tap - dy * KS;
        const int qoff = dy * HALO_W + dx;
        const char* wb = w_lds + buf * WSLAB;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const int chunk = kh * 4 + g;
            bf16x8 pf[4], wf[CT];
#pragma unroll
            for (int pg = 0; pg < 4; ++pg)
                pf[pg] = *reinterpret_cast<const bf16x8*>(in_lds + swz128(qb[pg] + qoff, chunk));
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                wf[ct] = *reinterpret_cast<const bf16x8*>(wb + swz128(ct * 16 + p, chunk));
#pragma unroll
            for (int pg = 0; pg < 4; ++pg)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[pg][ct] = mfma16x16x32(wf[ct], pf[pg], acc[pg][ct]);
        }
        if (it + 1 < total) wstore(buf ^ 1);
        __syncthreads();

        if (tap == NTAPS - 1 && ci == nci - 1) {
            // ---- epilogue for cout tile nt ----
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) {
                const int oy = ty0 + 2 * wave + (pg >> 1);
                const int ox = tx0 + (pg & 1) * 16 + p;
                if (oy >= H || ox >= W) continue;
                if constexpr (OUT_MODE == OUT_NHWC_BF16) {
                    // lane holds channels g*16 + ct*4 + reg (host packed the weight rows that way)
                    const int si = nt / r, sj = nt - si * r;
                    const int Hr = H * r, Wr = W * r;
                    bf16_t* o = reinterpret_cast<bf16_t*>(out) +
                                (((size_t)b * Hr + (oy * r + si)) * Wr + (ox * r + sj)) * 64 + g * 16;
                    uint32_t pk[8];
                    // optional fused "+ add" and "* (mask > 0)" (ReLU backward) on same-shaped NHWC tensors
                    const size_t eoff = (((size_t)b * Hr + (oy * r + si)) * Wr + (ox * r + sj)) * 64 + g * 16;
                    uint32_t aw[8], mw[8];
                    if (add) {
                        const u32x4 a0 = *reinterpret_cast<const u32x4*>(add + eoff), a1 = *reinterpret_cast<const u32x4*>(add + eoff + 8);
#pragma unroll
                        for (int q = 0; q < 4; ++q) { aw[q] = a0[q]; aw[4 + q] = a1[q]; }
                    }
                    if (mask) {
                        const u32x4 m0 = *reinterpret_cast<const u32x4*>(mask + eoff), m1 = *reinterpret_cast<const u32x4*>(mask + eoff + 8);
#pragma unroll
                        for (int q = 0; q < 4; ++q) { mw[q] = m0[q]; mw[4 + q] = m1[q]; }
                    }
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = acc[pg][ct][e];
                            v[e] += bv[ct][e];
                            if (relu) v[e] = fmaxf(v[e], 0.f);
                            const int wi = (ct * 4 + e) >> 1;
                            if (add) v[e] += __builtin_bit_cast(float, (e & 1) ? (aw[wi] & 0xffff0000u) : (aw[wi] << 16));
                            if (mask) {
                                const float mv = __builtin_bit_cast(float, (e & 1) ? (mw[wi] & 0xffff0000u) : (mw[wi] << 16));
                                if (!(mv > 0.f)) v[e] = 0.f;
                            }
                        }
                        pk[ct * 2 + 0] = pack_bf16x2(v[0], v[1]);
                        pk[ct * 2 + 1] = pack_bf16x2(v[2], v[3]);
                    }
                    if constexpr (CT == 4) {
                        *reinterpret_cast<u32x4*>(o) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                        *reinterpret_cast<u32x4*>(o + 8) = u32x4{pk[4], pk[5], pk[6], pk[7]};
                    }
                } else {
                    // thin output: rows 16ct+4g+reg are the real couts (< cout_valid); fp32 planar NCHW, written
                    // through PixelShuffle(r): cout n = c*r*r + si*r + sj -> out[b][c][oy*r+si][ox*r+sj]
                    float* o = reinterpret_cast<float*>(out);
                    const int rr = r * r, cimg = cout_valid / rr, Hr = H * r, Wr = W * r;
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int co = 16 * ct + 4 * g + e;
                            if (co < cout_valid) {
                                float v = acc[pg][ct][e];
                                v += bv[ct][e];
                                if (relu) v = fmaxf(v, 0.f);
                                const int c = co / rr, sp = co - c * rr;
                                const int si = sp / r, sj = sp - si * r;
                                o[(((size_t)b * cimg + c) * Hr + (oy * r + si)) * Wr + (ox * r + sj)] = v;
                            }
                        }
                }
            }
        }
    }
}



// ------------------------------------------------------------------------------------------------
// Persistent ping-pong variant (single input chunk, in_r = 1): one 8-wave workgroup per CU walks the
// pixel tiles.
//   * all NTAPS weight slabs of the current cout tile stay resident in LDS (73.7 KB for 3x3 / 64 couts),
//     so a tile is NTAPS*2 MFMA K-steps with no barrier in between (fragment reads hand-pipelined);
//   * the two wave groups (waves 0-3 / 4-7, one wave of each per SIMD) own one input buffer each and run
//     half a period apart: while group A issues the K loop of its tile, group B converts / stores its
//     previous tile and DMA-fetches its next halo image (global_load_lds_dwordx4; per-lane source address
//     carries the XOR swizzle and the halo clipping, out-of-image lanes read a zero line), then they swap.
//     The MFMA pipe of every SIMD always has one wave in a K loop; epilogue VALU, stores and DMA issue --
//     40 % of the time when a single group did everything in sequence -- hide under it.
// LDS: 9*8 KB + 2*43.5 KB = 160,768 B of the CU's 163,840 B.
// ------------------------------------------------------------------------------------------------
// Timing experiments (TUP_CONV_STAMPS=1, scripts/_conv_stamps.py): s_memtime of wave 0 of each group of workgroup 100
// at the phase boundaries of the first phases.  [group][phase][0 = phase start, 1 = K loop end | DMA issued,
// 2 = stores issued, 3 = vmcnt wait over, 4 = barrier passed]
__device__ unsigned long long tup_conv_stamps[2][16][5];

template <int CT, int OUT_MODE, int KS>
__global__ __launch_bounds__(512, 2) void conv_c64_persistent_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, const float* __restrict__ bias,
    const bf16_t* __restrict__ add, const bf16_t* __restrict__ mask,
    void* __restrict__ out, int B, int H, int W, int ntiles, int r, int cout_valid, int relu,
    int tilesX, int tilesY, int stamps)
{
    constexpr int PADK = KS / 2, HALO_W = TW + KS - 1, HALO_H = TH + KS - 1, NPIX_HALO = HALO_H * HALO_W;
    constexpr int NTAPS = KS * KS;
    constexpr int IN_BYTES = NPIX_HALO * 128;
    constexpr int WROWS = CT * 16, WSLAB = WROWS * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* w_lds = smem;                              // [NTAPS][WROWS][128 B]
    char* in_lds = smem + NTAPS * WSLAB;             // [2 groups][IN_BYTES]

    // wave group 0 / 1; scalar so that the tile bookkeeping runs on the SALU
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;      // indices inside the group
    const int g = lane >> 4, p = lane & 15;
    const int total_tiles = tilesX * tilesY * B;
    char* my_in = in_lds + grp * IN_BYTES;

    const HaloDma<HALO_H, HALO_W, PADK> dma(W, tid);
    auto prefetch_tile = [&](const TC& c) { dma.prefetch(x, c.b, c.ty * TH, c.tx * TW, H, W, my_in, tup_zero_line); };

    // loop-invariant LDS byte offsets of this lane's fragments
    uint32_t poff[NTAPS][2];
    pixel_frag_offsets<KS, HALO_W>(poff, my_in, wave, g, p);
    const uint32_t wbase0 = weight_frag_base(w_lds, g, p);

    f32x4 acc[4][CT];
    // this lane's bias values live in LDS ([g][ct][4] floats after the two input images), not in 4*CT registers
    float* bias_lds = reinterpret_cast<float*>(in_lds + 2 * IN_BYTES);
    const uint32_t bias_addr = lds_addr(bias_lds) + (uint32_t)(g * CT * 16);

    auto store_tile = [&](const TC& c, int nt) {
        const int tx = c.tx, ty = c.ty, b = c.b;
#pragma unroll
        for (int pg = 0; pg < 4; ++pg) {
            const int oy = ty * TH + 2 * wave + (pg >> 1);
            const int ox = tx * TW + (pg & 1) * 16 + p;
            const bool ok = oy < H && ox < W;
            if constexpr (OUT_MODE == OUT_NHWC_BF16) {
                const int si = nt / r, sj = nt - si * r;
                const int Hr = H * r, Wr = W * r;
                const size_t eoff = (((size_t)b * Hr + (oy * r + si)) * Wr + (ox * r + sj)) * 64 + g * 16;
                uint32_t pk[8], aw[8], mw[8];
                if (add && ok) {
                    const u32x4 a0 = *reinterpret_cast<const u32x4*>(add + eoff), a1 = *reinterpret_cast<const u32x4*>(add + eoff + 8);
#pragma unroll
                    for (int q = 0; q < 4; ++q) { aw[q] = a0[q]; aw[4 + q] = a1[q]; }
                }
                if (mask && ok) {
                    const u32x4 m0 = *reinterpret_cast<const u32x4*>(mask + eoff), m1 = *reinterpret_cast<const u32x4*>(mask + eoff + 8);
#pragma unroll
                    for (int q = 0; q < 4; ++q) { mw[q] = m0[q]; mw[4 + q] = m1[q]; }
                }
                if (!add && !mask) {
                    // common case: ReLU on the packed bf16 pairs as a signed-16-bit max with 0 (negative bf16 = negative
                    // int16), one v_pk_max_i16 per two values instead of one v_max_f32 per value
                    typedef short s16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        pk[ct * 2 + 0] = pack_bf16x2(acc[pg][ct][0], acc[pg][ct][1]);
                        pk[ct * 2 + 1] = pack_bf16x2(acc[pg][ct][2], acc[pg][ct][3]);
                    }
                    if (relu) {
#pragma unroll
                        for (int q = 0; q < 2 * CT; ++q)
                            pk[q] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, pk[q]), s16x2{0, 0}));
                    }
                } else
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = acc[pg][ct][e];                     // bias already in the accumulator
                        if (relu) v[e] = fmaxf(v[e], 0.f);
                        const int wi = (ct * 4 + e) >> 1;
                        if (add && ok) v[e] += __builtin_bit_cast(float, (e & 1) ? (aw[wi] & 0xffff0000u) : (aw[wi] << 16));
                        if (mask && ok) {
                            const float mv = __builtin_bit_cast(float, (e & 1) ? (mw[wi] & 0xffff0000u) : (mw[wi] << 16));
                            if (!(mv > 0.f)) v[e] = 0.f;
                        }
                    }
                    pk[ct * 2 + 0] = pack_bf16x2(v[0], v[1]);
                    pk[ct * 2 + 1] = pack_bf16x2(v[2], v[3]);
                }
                if constexpr (CT == 4) {
                    // exactly two store instructions per pixel group for every wave (out-of-image lanes hit the sink)
                    bf16_t* o = ok ? reinterpret_cast<bf16_t*>(out) + eoff : reinterpret_cast<bf16_t*>(tup_store_sink) + lane * 16;
                    *reinterpret_cast<u32x4*>(o) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                    *reinterpret_cast<u32x4*>(o + 8) = u32x4{pk[4], pk[5], pk[6], pk[7]};
                }
            } else {
                // thin output (the entry admits it with r = 1 only): rows 16ct+4g+reg are the real couts (< cout_valid), fp32 planar NCHW
                if (!ok) continue;
                float* o = reinterpret_cast<float*>(out);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int co = 16 * ct + 4 * g + e;
                        if (co < cout_valid) {
                            float v = acc[pg][ct][e];
                            if (relu) v = fmaxf(v, 0.f);
                            o[(((size_t)b * cout_valid + co) * H + oy) * W + ox] = v;
                        }
                    }
            }
        }
    };

    // tiles of this workgroup; group `grp` takes every second one
    const TileWalk walk(total_tiles, tilesX, tilesY, grp, !(stamps & 2));
    const int my_count = walk.my_count, nphases = walk.nphases;
    const TC c_first = walk.first;

    for (int nt = 0; nt < ntiles; ++nt) {
        stage_weights<CT, NTAPS>(w_lds, wp + (size_t)nt * NTAPS * WROWS * 64);
        stage_bias<CT, OUT_MODE != OUT_NHWC_BF16>(bias_lds, bias, nt, cout_valid);
        if (grp == 0 && my_count > 0) prefetch_tile(c_first);
        __syncthreads();            // weights + group 0's first tile visible (the barrier's vmcnt(0) retires the DMA)
        // c_done = the tile this group computed last (to be stored), c_next = the one to fetch next
        TC c_done = c_first, c_next = c_first;
        if (grp == 0) walk.advance(c_next);

        // phase ph: group (ph & 1) runs the K loop of its tile k = ph >> 1; the other group stores its previous
        // tile and DMA-fetches its next one into its (now idle) buffer.  One workgroup barrier per phase.
        const bool st_on = (stamps & 1) && blockIdx.x == 100 && (threadIdx.x & 255) == 0 && nt == 0;
        auto stamp = [&](int ph, int i) { if (st_on && ph < 16) tup_conv_stamps[grp][ph][i] = __builtin_amdgcn_s_memtime(); };
        for (int ph = 0; ph < nphases; ++ph) {
            const int k = ph >> 1;
            stamp(ph, 0);
            if ((ph & 1) == grp) {
                if (k < my_count && !(stamps & 16)) k_loop<CT, NTAPS>(acc, poff, wbase0, bias_addr);
                stamp(ph, 1);
            } else {
                // group 0 is here on odd phases (just computed tile k, next is k+1); group 1 on even phases
                // (computed tile k-1 in phase ph-1, next is k)
                const int done = grp == 0 ? k : k - 1;
                const int nxt = done + 1;
                // DMA first: it then has the whole phase (the other group's K loop) to land; the buffer is idle
                // because this group's own K loop ended before the last barrier
                if (nxt < my_count && !(stamps & 8)) prefetch_tile(c_next);
                stamp(ph, 1);
                if (done >= 0 && done < my_count && !(stamps & 4)) {
                    store_tile(c_done, nt);
                    stamp(ph, 2);
                    // The DMA (issued first) must have landed before the barrier; the 8 stores issued after it need
                    // not: vmcnt counts in issue order, so "all but the youngest 8" = the DMA.  (A __syncthreads()
                    // here makes hipcc wait vmcnt(0), i.e. for the stores' write latency, which was the longest
                    // item of the phase.)
                    if constexpr (OUT_MODE == OUT_NHWC_BF16 && CT == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                c_done = c_next;                     // the tile just fetched is computed next and stored in this group's next idle phase
                walk.advance(c_next);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            stamp(ph, 3);
            __builtin_amdgcn_s_barrier();
            stamp(ph, 4);
        }
        // drain before the next pass restages the weights / the kernel ends
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

template <int CT, int OUT_MODE, int KS>
int launch_persistent(const void* x, const void* wp, const float* bias, const void* add, const void* mask, void* out,
                      int B, int H, int W, int ntiles, int r, int cout_valid, int relu, hipStream_t s)
{
    constexpr int NPIX_HALO = (TH + KS - 1) * (TW + KS - 1);
    constexpr size_t lds = (size_t)KS * KS * CT * 16 * 128 + 2 * (size_t)NPIX_HALO * 128 + 256;     // + bias
    static_assert(lds <= 163840, "LDS budget");
    TUP_SET_DYN_LDS((conv_c64_persistent_kernel<CT, OUT_MODE, KS>), lds);
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    const long long nt = (long long)tilesX * tilesY * B;
    if (nt > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const int grid = (int)(nt < 256 ? nt : 256);                 // one workgroup per CU
    // bit 0: s_memtime stamps; bit 1: round-robin tiles instead of XCD bands; timing experiments (wrong results): TUP_CONV_ABLATE
    // bits 4 = no stores, 8 = no DMA, 16 = no K loop
#ifdef TUP_DIAG          // `make diag` only; the product library always passes 0
    static const int conv_stamps_on = (getenv("TUP_CONV_STAMPS") ? 1 : 0) | (getenv("TUP_CONV_NO_XCD_BANDS") ? 2 : 0) |
                                      (getenv("TUP_CONV_ABLATE") ? (atoi(getenv("TUP_CONV_ABLATE")) & 28) : 0);
#else
    constexpr int conv_stamps_on = 0;
#endif
    conv_c64_persistent_kernel<CT, OUT_MODE, KS><<<dim3(grid), dim3(512), lds, s>>>(
        (const bf16_t*)x, (const bf16_t*)wp, bias, (const bf16_t*)add, (const bf16_t*)mask, out, B, H, W, ntiles, r,
        cout_valid, relu, tilesX, tilesY, conv_stamps_on);
    TUP_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Composed branch A at r = 2 (12 outputs) as a ROW GEMM.  A 25-tap form of the kernel above (CT = 1, KS = 5; rounds 1-2, since
// removed) read four pixel fragments and one weight fragment from LDS for every four MFMAs -- each halo pixel 25 times -- and ran
// exactly at the LDS read rate (1 MB per tile, 8 k cycles against 3.2 k of MFMA issue).  Here the horizontal taps ride in the
// GEMM's N instead:
//     part[y][x'][(c, dx)] = sum_dy sum_ci  in[y + dy][x'][ci] * w[dy][dx][c][ci]
//     out[y][x][c]         = sum_dx part[y][x + dx][(c, dx)]
// so a halo pixel is read five times (once per dy).  Only the LIVE taps are visited: the composition (packing.compose_branch_a)
// puts sub-pixel (si, sj)'s kernel on a 4 x 4 block of the 5 x 5 -- tap row 4 is zero for si = 0, row 0 for si = 1, column 4 for
// sj = 0, column 0 for sj = 1 -- so each of the four 16-row weight tiles belongs to ONE sub-pixel t = si*2 + sj:
//     row 4*ch + k of tile t  =  output ch*4 + t, tap column dx = k + sj        (rows 12..15 zero)
// The K-steps of dy = 0 run the two si = 0 tiles only and those of dy = 4 the two si = 1 tiles: 6*16 + 4*8 = 128 MFMAs and
// 6*8 + 4*6 = 72 fragment reads per wave and tile (the dense form: 160 and 80).  Lane (g, p) of the accumulators ends with image
// channel g's four live dx of all four sub-pixels at halo column p (group 3 idles): the dx sum is 3-4 (+ 3-4 across the 16-column
// seam) DPP row shifts per output, no LDS round trip, and the two sj of an HR row leave in one 8-byte store.
// Tile = 8 rows x 28 output columns (halo image 12 x 32 pixels: two whole 16-pixel groups per row); tile walk and halo DMA
// are conv_pingpong.h's, the row-GEMM K loop is its own.  LDS: 16 slabs * 2 KB + 2*48 KB = 131,072 B.
// ------------------------------------------------------------------------------------------------
constexpr int R5_TW = 28, R5_HW = 32, R5_HH = TH + 4, R5_NPIX = R5_HH * R5_HW, R5_IN_BYTES = R5_NPIX * 128;
constexpr int R5_NSLAB = 2 + 3 * 4 + 2, R5_W_BYTES = R5_NSLAB * 16 * 128;
// weight slab (16 rows x 128 B) of tap row dy and tile t: dy = 0 holds tiles 0, 1; dy = 1..3 all four; dy = 4 tiles 2, 3
constexpr int r5_slab(int dy, int t) { return dy == 0 ? t : (dy == 4 ? 12 + t : 2 + (dy - 1) * 4 + t); }
constexpr int r5_ntiles(int dy) { return (dy == 0 || dy == 4) ? 2 : 4; }        // live tiles of a tap row ...
constexpr int r5_tile0(int dy) { return dy == 4 ? 2 : 0; }                      // ... starting at this one

__global__ __launch_bounds__(512, 2) void bra_rows_persistent_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, const float* __restrict__ bias,
    float* __restrict__ out, int B, int H, int W, int relu, int tilesX, int tilesY, int ablate)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* w_lds = smem;                              // [16 slabs (dy, t)][16 rows][128 B]
    char* in_lds = smem + R5_W_BYTES;                // [2 groups][R5_IN_BYTES]
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));      // scalar: tile bookkeeping on the SALU
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, p = lane & 15;
    const int total_tiles = tilesX * tilesY * B;
    char* my_in = in_lds + grp * R5_IN_BYTES;

    using Dma = HaloDma<R5_HH, R5_HW, 2>;
    static_assert(!Dma::LAST_PARTIAL && Dma::NPIECE == 12, "12 whole DMA pieces");
    const Dma dma(W, tid);
    auto prefetch_tile = [&](const TC& c) { dma.prefetch(x, c.b, c.ty * TH, c.tx * R5_TW, H, W, my_in, tup_zero_line); };

    // weights: LDS row 4*ch + k of slab (dy, t) <- tap (dy, dx = k + sj), output co = ch*4 + t of the 25-tap packing
    // [25][16][64].  The dead taps of wp (tap row 4 / 0 of si = 0 / 1, tap column 4 / 0 of sj = 0 / 1) are never read.
    for (int idx = threadIdx.x; idx < R5_NSLAB * 16 * 8; idx += 512) {
        const int row = idx >> 3, c = idx & 7;
        const int slab = row >> 4, r16 = row & 15;
        const int dy = slab < 2 ? 0 : (slab < 14 ? 1 + ((slab - 2) >> 2) : 4);
        const int t = slab < 2 ? slab : (slab < 14 ? (slab - 2) & 3 : slab - 12);
        const int ch = r16 >> 2, dx = (r16 & 3) + (t & 1);
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (ch < 3) v = *reinterpret_cast<const u32x4*>(wp + ((size_t)((dy * 5 + dx) * 16 + ch * 4 + t)) * 64 + c * 8);
        *reinterpret_cast<u32x4*>(w_lds + swz128(row, c)) = v;
    }
    float bsp[4];                                    // this lane's image channel g, sub-pixels 0..3 (group 3 idles)
#pragma unroll
    for (int t = 0; t < 4; ++t) bsp[t] = (bias && g < 3) ? bias[g * 4 + t] : 0.f;

    // fragment addresses: the swizzle phase ((q >> 1) & 7) of pixel q = row*32 + cg*16 + p and of weight row slab*16 + p
    // is (p >> 1) & 7 for both, so one base register each and everything else in the 16-bit immediate
    const uint32_t pbase = lds_addr(my_in) + (uint32_t)(2 * wave * R5_HW * 128) + (uint32_t)swz128(p, g);
    const uint32_t wbase = lds_addr(w_lds) + (uint32_t)swz128(p, g);

    f32x4 acc[2][2][4];                              // [output row of the wave][16-column group][weight tile = sub-pixel]
    // K loop: 10 steps (dy, K half) of 4 pixel + 2 or 4 weight fragments and 8 or 16 MFMAs, fragments requested two steps ahead
    // (3-slot ring).  The requests of step + 2 are spread between the MFMA pairs of the step: issued in a block at the top of the
    // step they cost the wave ~60 cycles per step in which its matrix pipe idles, and with one wave per SIMD in a K loop nothing
    // else fills it.
    auto compute_tile = [&]() {
        constexpr int NSTEPS = 10;
        bf16x8 pf[3][4], wf[3][4];
        auto load_frag = [&](int step, int slot, int j) {          // j = 0..3 pixel fragments (rw*2 + cg), 4.. live weight tiles
            const int dy = step >> 1;
            if (j < 4) {
                const int off = ((j >> 1) + dy) * (R5_HW * 128) + (j & 1) * 2048;
                pf[slot][j] = (step & 1) ? lds_read_b128_asm_off_x64(pbase, off) : lds_read_b128_asm_off(pbase, off);
            } else {
                const int off = r5_slab(dy, r5_tile0(dy) + j - 4) * 2048;
                wf[slot][j - 4] = (step & 1) ? lds_read_b128_asm_off_x64(wbase, off) : lds_read_b128_asm_off(wbase, off);
            }
        };
        auto nfrag = [](int step) { return 4 + r5_ntiles(step >> 1); };
#pragma unroll
        for (int j = 0; j < nfrag(0); ++j) load_frag(0, 0, j);
#pragma unroll
        for (int j = 0; j < nfrag(1); ++j) load_frag(1, 1, j);
#pragma unroll
        for (int rw = 0; rw < 2; ++rw)
#pragma unroll
            for (int cg = 0; cg < 2; ++cg)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[rw][cg][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int step = 0; step < NSTEPS; ++step) {
            const int cur = step % 3, dy = step >> 1;
            const int npair = 2 * r5_ntiles(dy), t00 = r5_tile0(dy);
            const int nld = step + 2 < NSTEPS ? nfrag(step + 2) : 0;
            // this step's fragments; the next step's may still fly
            if (step + 1 >= NSTEPS) lds_wait<0>(); else if (nfrag(step + 1) == 8) lds_wait<8>(); else lds_wait<6>();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < npair; ++j) {
#pragma unroll
                for (int l = j * nld / npair; l < (j + 1) * nld / npair; ++l) load_frag(step + 2, (step + 2) % 3, l);
                // MFMA pair j: pixel fragment i, two live weight tiles
                const int i = npair == 8 ? (j >> 1) : j, w0 = npair == 8 ? (j & 1) * 2 : 0, t0 = t00 + w0;
                acc[i >> 1][i & 1][t0] = mfma16x16x32(wf[cur][w0], pf[cur][i], acc[i >> 1][i & 1][t0]);
                acc[i >> 1][i & 1][t0 + 1] = mfma16x16x32(wf[cur][w0 + 1], pf[cur][i], acc[i >> 1][i & 1][t0 + 1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // RELU is a compile-time copy of `relu`: as a run-time value hipcc turns every output's clamp into v_max x, x + v_max 0 +
    // v_cndmask (48 of the phase's vector instructions, all issued out of the other group's MFMA stream)
    auto store_tile = [&](const TC& c, auto RELU) {
        const int tx = c.tx, ty = c.ty, b = c.b;
        const int Wr = W * 2;
        float* outb = out + ((size_t)b * 3 + g) * 4 * H * W;                       // this lane's HR plane
        // The idle group sits the phase out with its lanes switched off -- sent to the sink, a quarter of every store of every
        // wave on the chip lands on the same 512 bytes, and the store leg alone takes 198 us instead of 157.  Groups 0..2 are
        // in every wave, so each store below still issues once per wave.
        if (g >= 3) return;
#pragma unroll
        for (int rw = 0; rw < 2; ++rw) {
            const int oy = ty * TH + 2 * wave + rw;
#pragma unroll
            for (int cg = 0; cg < 2; ++cg) {
                const int xo = cg * 16 + p, ox = tx * R5_TW + xo;
                const bool ok = oy < H && ox < W;
                // exactly 8 store instructions per wave and tile (the counted wait of the phase loop): lanes outside the image go
                // to the sink, because a whole wave can be outside it.  The halo columns 28..31 (lanes p >= 12 of the second
                // group, beside twelve live lanes in every wave) are switched off for the store alone: the DPP adds of lanes
                // 8..11 read them, and a switched-off source lane reads as zero
                float* o = ok ? outb + (oy * 2 * Wr + ox * 2) : reinterpret_cast<float*>(tup_store_sink) + 2 * lane;
                const int rstep = ok ? Wr : 0;
#pragma unroll
                for (int si = 0; si < 2; ++si) {
                    // dx ascending with the bias first, as the dense form summed them: sj = 0 has dx = k, sj = 1 has dx = k + 1
                    const f32x4 &a0 = acc[rw][cg][si * 2], &a1 = acc[rw][cg][si * 2 + 1];
                    float v0 = a0[0] + bsp[si * 2], v1 = bsp[si * 2 + 1];
                    TUP_ADD_DPP(v0, a0[1], "row_shl:1"); TUP_ADD_DPP(v0, a0[2], "row_shl:2"); TUP_ADD_DPP(v0, a0[3], "row_shl:3");
                    TUP_ADD_DPP(v1, a1[0], "row_shl:1"); TUP_ADD_DPP(v1, a1[1], "row_shl:2");
                    TUP_ADD_DPP(v1, a1[2], "row_shl:3"); TUP_ADD_DPP(v1, a1[3], "row_shl:4");
                    if (cg == 0) {                   // halo columns 16..19 live in the next group's lanes 0..3
                        const f32x4 &n0 = acc[rw][1][si * 2], &n1 = acc[rw][1][si * 2 + 1];
                        TUP_ADD_DPP(v0, n0[1], "row_shr:15"); TUP_ADD_DPP(v0, n0[2], "row_shr:14"); TUP_ADD_DPP(v0, n0[3], "row_shr:13");
                        TUP_ADD_DPP(v1, n1[0], "row_shr:15"); TUP_ADD_DPP(v1, n1[1], "row_shr:14");
                        TUP_ADD_DPP(v1, n1[2], "row_shr:13"); TUP_ADD_DPP(v1, n1[3], "row_shr:12");
                    }
                    if constexpr (decltype(RELU)::value) {           // = fmaxf(v, 0) without the canonicalising v_max v, v in front
                        asm("v_max_f32 %0, 0, %0" : "+v"(v0));
                        asm("v_max_f32 %0, 0, %0" : "+v"(v1));
                    }
                    if (cg == 0 || p < R5_TW - 16) *reinterpret_cast<f32x2*>(o + si * rstep) = f32x2{v0, v1};
                }
            }
        }
    };

    // Tiles of this workgroup, in XCD bands (xcd_band): with round-robin tiles the halo a tile shares with its neighbours crossed
    // the fabric once per XCD (halo image / tile = 1.71: the DMA alone ran at the same 227 us with nothing else on).
    const TileWalk walk(total_tiles, tilesX, tilesY, grp, !(ablate & 8));
    const int my_count = walk.my_count, nphases = walk.nphases;
    TC c_done = walk.first, c_next = walk.first;
    if (grp == 0 && my_count > 0) prefetch_tile(c_next);
    if (grp == 0) walk.advance(c_next);
    __syncthreads();
    for (int ph = 0; ph < nphases; ++ph) {
        const int k = ph >> 1;
        if ((ph & 1) == grp) {
            if (k < my_count && !(ablate & 1)) compute_tile();
        } else {
            const int done = grp == 0 ? k : k - 1;
            const int nxt = done + 1;
            if (nxt < my_count && !(ablate & 4)) prefetch_tile(c_next);
            if (done >= 0 && done < my_count && !(ablate & 2)) {
                if (relu) store_tile(c_done, std::true_type{}); else store_tile(c_done, std::false_type{});
                // the DMA (issued first) must have landed before the barrier, the 8 stores after it need not
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            c_done = c_next;                         // the tile just fetched: computed next, stored in this group's next idle phase
            walk.advance(c_next);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

int launch_bra_rows(const void* x, const void* wp, const float* bias, float* out, int B, int H, int W, int relu, hipStream_t s)
{
    constexpr size_t lds = (size_t)R5_W_BYTES + 2 * (size_t)R5_IN_BYTES;
    static_assert(lds <= 163840, "LDS budget");
    TUP_SET_DYN_LDS(bra_rows_persistent_kernel, lds);
    const int tilesX = (W + R5_TW - 1) / R5_TW, tilesY = (H + TH - 1) / TH;
    const long long nt = (long long)tilesX * tilesY * B;
    if (nt > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(out) & 7)) return (int)hipErrorInvalidValue;     // 8-byte stores
    const int grid = (int)(nt < 256 ? nt : 256);                 // one workgroup per CU
    static const int ablate = TUP_ENV_INT("TUP_BRA_ABLATE", 0);     // timing experiments: 1 no K loop, 2 no stores, 4 no DMA
    bra_rows_persistent_kernel<<<dim3(grid), dim3(512), lds, s>>>((const bf16_t*)x, (const bf16_t*)wp, bias, out, B, H, W, relu, tilesX, tilesY, ablate);
    TUP_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// 64 -> (<= 4) channel 3x3 conv with planar fp32 output (decoder_conv2; up1_conv in training) as a row GEMM: N = (channel c,
// dx) = weight row 4c + dx, K = 3 dy x 64, so a halo pixel is read from LDS three times, a wave's whole K loop is 24 MFMAs with
// the six weight fragments in registers, and out[x][c] = part[c][0](x) + part[c][1](x + 1) + part[c][2](x + 2) is two DPP row
// shifts.  The kernel is HBM-class (reads 128 B per pixel, writes 12): the ping-pong form above keeps ONE 43.5 KB tile in flight
// per CU and its phases were the DMA latency (3.9 TB/s).  Here a workgroup is 4 waves with one 40 KB halo image (8 x 28 output
// pixels, halo 10 x 32), THREE workgroups per CU each walking its own tiles: three images in flight per CU, no counted waits.
// ------------------------------------------------------------------------------------------------
constexpr int T3_TW = 28, T3_HW = 32, T3_HH = TH + 2, T3_NPIX = T3_HH * T3_HW, T3_IN_BYTES = T3_NPIX * 128;

__global__ __launch_bounds__(256, 3) void conv3_thin_rows_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp, const float* __restrict__ bias,
    float* __restrict__ out, int B, int H, int W, int cout, int relu, int tilesX, int tilesY)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];              // one halo image
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, p = lane & 15;
    const int total_tiles = tilesX * tilesY * B;

    using Dma = HaloDma<T3_HH, T3_HW, 1>;
    static_assert(!Dma::LAST_PARTIAL && Dma::NPIECE == 10, "10 whole DMA pieces");
    const Dma dma(W, tid);
    auto prefetch_tile = [&](int tile) {
        int t = tile;
        const int tx = t % tilesX; t /= tilesX;
        const int ty = t % tilesY;
        const int b = t / tilesY;
        dma.prefetch(x, b, ty * TH, tx * T3_TW, H, W, smem, tup_zero_line);
    };

    // weight fragments (A operand: lane (g, p) = row p = 4c + dx, channels 8g.. of K half kh) straight from the packed
    // [9 taps][16 rows][64] tensor (row = output channel): six 16-byte loads per lane, once
    bf16x8 wfr[3][2];
    {
        const int c = p >> 2, dx = p & 3;
        const bool live = dx < 3 && c < cout;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                u32x4 v = u32x4{0u, 0u, 0u, 0u};
                if (live) v = *reinterpret_cast<const u32x4*>(wp + ((size_t)((dy * 3 + dx) * 16 + c)) * 64 + kh * 32 + g * 8);
                wfr[dy][kh] = __builtin_bit_cast(bf16x8, v);
            }
    }
    const float bv = (bias && g < cout) ? bias[g] : 0.f;       // the accumulators' lane (g, p) = channel g
    const uint32_t pbase = lds_addr(smem) + (uint32_t)(2 * wave * T3_HW * 128) + (uint32_t)swz128(p, g);

    f32x4 acc[2][2];                                 // [output row of the wave][16-column group]
    auto compute_tile = [&]() {
        bf16x8 pf[6][4];
#pragma unroll
        for (int st = 0; st < 6; ++st)               // st = dy*2 + kh
#pragma unroll
            for (int i = 0; i < 4; ++i) {            // i = rw*2 + cg
                const int off = ((i >> 1) + (st >> 1)) * (T3_HW * 128) + (i & 1) * 2048;
                pf[st][i] = (st & 1) ? lds_read_b128_asm_off_x64(pbase, off) : lds_read_b128_asm_off(pbase, off);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            if (st == 0) lds_wait<15>(); else if (st == 1) lds_wait<15>(); else if (st == 2) lds_wait<12>();
            else if (st == 3) lds_wait<8>(); else if (st == 4) lds_wait<4>(); else lds_wait<0>();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = mfma16x16x32(wfr[st >> 1][st & 1], pf[st][i], acc[i >> 1][i & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto store_tile = [&](int tile) {
        int t = tile;
        const int tx = t % tilesX; t /= tilesX;
        const int ty = t % tilesY;
        const int b = t / tilesY;
        float* outb = out + ((size_t)b * cout + g) * H * W;
#pragma unroll
        for (int rw = 0; rw < 2; ++rw) {
            const int oy = ty * TH + 2 * wave + rw;
#pragma unroll
            for (int cg = 0; cg < 2; ++cg) {
                const int xo = cg * 16 + p, ox = tx * T3_TW + xo;
                float v = acc[rw][cg][0] + bv;
                TUP_ADD_DPP(v, acc[rw][cg][1], "row_shl:1"); TUP_ADD_DPP(v, acc[rw][cg][2], "row_shl:2");
                if (cg == 0) { TUP_ADD_DPP(v, acc[rw][1][1], "row_shr:15"); TUP_ADD_DPP(v, acc[rw][1][2], "row_shr:14"); }
                if (relu) v = fmaxf(v, 0.f);
                if (g < cout && oy < H && ox < W && xo < T3_TW) outb[(size_t)oy * W + ox] = v;
            }
        }
    };

    // tiles: XCD-contiguous bands (blockIdx & 7 = XCD)
    int first, stride, limit;
    xcd_band(total_tiles, true, first, stride, limit);
    if (first < limit) prefetch_tile(first);
    for (int tile = first; tile < limit; tile += stride) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                // the image of `tile` is complete
        compute_tile();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                // everyone's fragment reads are done: the image may be overwritten
        if (tile + stride < limit) prefetch_tile(tile + stride);
        store_tile(tile);                            // under the next image's flight
    }
}

int launch_thin_rows(const void* x, const void* wp, const float* bias, float* out, int B, int H, int W, int cout, int relu, hipStream_t s)
{
    const int tilesX = (W + T3_TW - 1) / T3_TW, tilesY = (H + TH - 1) / TH;
    const long long nt = (long long)tilesX * tilesY * B;
    if (nt > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const int grid = (int)(nt < 768 ? nt : 768);                 // three workgroups per CU
    conv3_thin_rows_kernel<<<dim3(grid), dim3(256), T3_IN_BYTES, s>>>((const bf16_t*)x, (const bf16_t*)wp, bias, out, B, H, W, cout, relu, tilesX, tilesY);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Border fix-up of the composed branch-A conv (see tup_conv5x5_c64_planar_fwd): one wave per HR border
// pixel recomputes it with the weight variant that leaves out the 64->3 conv's taps falling outside
// the HR image (those see zero padding in the reference, not a virtual up-conv value).
// The pixel, its variant and its live taps are the same for the whole wave: they are derived from a readfirstlane'd wave index and
// blockIdx (image = blockIdx.y, no division by the ring length) with r a template constant, so that all of it runs on the scalar
// unit -- the kernel is bound by the number of vector instructions its 64 k waves issue.
template <int R>
__global__ __launch_bounds__(256) void conv5x5_border_fix_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wv, const float* __restrict__ bv,
    float* __restrict__ out, int B, int H, int W, int relu)
{
    constexpr int r = R, rr = r * r, nout = 3 * rr;
    const int lane = threadIdx.x & 63;
    const int Hs = H * r, Ws = W * r;
    const int per_img = 2 * Ws + 2 * (Hs - 2);
    int k = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= per_img) return;
    int Y, X;
    if (k < Ws) { Y = 0; X = k; }
    else if (k < 2 * Ws) { Y = Hs - 1; X = k - Ws; }
    else { k -= 2 * Ws; Y = 1 + (k >> 1); X = (k & 1) ? Ws - 1 : 0; }
    const int rowmode = (Y == 0) ? 1 : (Y == Hs - 1 ? 2 : 0), colmode = (X == 0) ? 1 : (X == Ws - 1 ? 2 : 0);
    const int v = rowmode * 3 + colmode;
    const int y = Y / r, si = Y - y * r, xx0 = X / r, sj = X - xx0 * r;
    const int sp = si * r + sj;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {          // one image per blockIdx.y (a loop only beyond 65,535 images)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        // The live taps of a ring pixel, in closed form and wave-uniform (the weights are not consulted).  The variant keeps the
        // 64->3 conv's taps dy in [dlo, dhi] (rowmode 1 / 2 drops dy = 0 / 2); HR row Y + dy - 1 is LR row offset
        // oy = floor((si + dy - 1) / r), whose up-conv taps cover tap rows oy + 1 .. oy + 3; the image keeps 2 - y <= ty <= H + 1 - y.
        // Columns alike.  A ring pixel has rowmode != 0 (then si + dy - 1 stays within one LR row: tap rows 1..3, of which the image
        // edge keeps two, by at most four columns) or colmode != 0 (at most four rows by two columns): never more than 8 live taps,
        // for every r.  packing.compose_branch_a produces exactly this support; taps outside it are not read.
        const int ylo = (si + (rowmode == 1 ? 1 : 0) - 1 + r) / r, yhi = (si + (rowmode == 2 ? 1 : 2) - 1 + r) / r + 2;   // = oy + 1, oy + 3
        const int xlo = (sj + (colmode == 1 ? 1 : 0) - 1 + r) / r, xhi = (sj + (colmode == 2 ? 1 : 2) - 1 + r) / r + 2;
        const int ty0 = max(ylo, 2 - y), tx0 = max(xlo, 2 - xx0);
        const int ny = min(yhi, H + 1 - y) - ty0 + 1, nx = min(xhi, W + 1 - xx0) - tx0 + 1;         // both >= 1: tap (2, 2) is always live
        // lane = (tap slot t8 = lane >> 3, channel chunk c8 = lane & 7): slot t8 takes tap (ty0 + t8 / nx, tx0 + t8 % nx) -- one round
        // of eight slots, every load 16 bytes (eight bf16 channels) and all four requested before the first use: one global round
        // trip per pixel.  (The dense form walked all 25 taps in four such rounds; round 2's one-channel-per-lane form issued 100
        // two-byte loads in five dependent rounds and ran at 0.6 TB/s, 75 us for the ring.)
        const int t8 = lane >> 3, c8 = lane & 7;
        const int rcp = nx == 1 ? 32 : (nx == 2 ? 16 : (nx == 3 ? 11 : 8));          // t8 / nx = (t8 * ceil(32 / nx)) >> 5 for t8 < 8, nx <= 4
        const int qy = (t8 * rcp) >> 5, ty = ty0 + qy, tx = tx0 + t8 - qy * nx;
        const bool use = t8 < ny * nx;
        const int tapc = use ? ty * 5 + tx : 12;                                     // idle slots load the centre tap: always in bounds
        const int iyc = use ? y + ty - 2 : y, ixc = use ? xx0 + tx - 2 : xx0;
        const u32x4 fx = *reinterpret_cast<const u32x4*>(x + (((size_t)b * H + iyc) * W + ixc) * 64 + c8 * 8);
        const bf16_t* wb = wv + (((size_t)v * nout) * 25 + tapc) * 64 + c8 * 8;                                    // [v][n][tap][ci]
        u32x4 fw[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) fw[c] = *reinterpret_cast<const u32x4*>(wb + (size_t)(c * rr + sp) * 25 * 64);
        if (use) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float xl = __builtin_bit_cast(float, fx[q] << 16), xh = __builtin_bit_cast(float, fx[q] & 0xffff0000u);
                a0 = fmaf(xl, __builtin_bit_cast(float, fw[0][q] << 16), a0); a0 = fmaf(xh, __builtin_bit_cast(float, fw[0][q] & 0xffff0000u), a0);
                a1 = fmaf(xl, __builtin_bit_cast(float, fw[1][q] << 16), a1); a1 = fmaf(xh, __builtin_bit_cast(float, fw[1][q] & 0xffff0000u), a1);
                a2 = fmaf(xl, __builtin_bit_cast(float, fw[2][q] << 16), a2); a2 = fmaf(xh, __builtin_bit_cast(float, fw[2][q] & 0xffff0000u), a2);
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); }
        if (lane < 3) {
            float val = (lane == 0 ? a0 : (lane == 1 ? a1 : a2)) + bv[v * nout + lane * rr + sp];
            if (relu) val = fmaxf(val, 0.f);
            out[(((size_t)b * 3 + lane) * Hs + Y) * Ws + X] = val;
        }
    }
}

}  // namespace

// x: [B][H*in_r][W*in_r][64] bf16 (in_r = 1: plain 64-channel map; in_r > 1: 64*in_r^2 logical input
// channels stored pixel-shuffled, i.e. the gradient of an Upsampler stage's output -- this makes the
// same kernel the input-gradient conv of the up-convs).  wp: [ntiles][in_r^2][9][rows][64] bf16.
// out_mode 0: out = [B][H*r][W*r][64] bf16, ntiles = r*r, bias fp32 [ntiles][64] or NULL; optional
//   add / mask (bf16, same shape as out): out = (conv + bias [relu] + add) * (mask > 0).
// out_mode 1: out = [B][cout_valid][H][W] fp32, cout_valid <= 16, ntiles = 1, r = 1.
extern "C" int tup_conv3x3_c64_fwd(const void* x, const void* wp, const float* bias, const void* add,
                                   const void* mask, void* out, int B, int H, int W, int ntiles, int r,
                                   int cout_valid, int relu, int out_mode, int in_r, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (in_r < 1 || in_r > 6) return (int)hipErrorInvalidValue;
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    const long long nblk = (long long)tilesX * tilesY * B;
    if (nblk > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    static const bool use_persistent = !TUP_ENV_FLAG("TUP_CONV_NONPERSISTENT");
    if (in_r == 1 && use_persistent) {
        if (out_mode == OUT_NHWC_BF16) {
            if (ntiles != r * r || r < 1) return (int)hipErrorInvalidValue;
            return launch_persistent<4, OUT_NHWC_BF16, 3>(x, wp, bias, add, mask, out, B, H, W, ntiles, r, 64, relu, s);
        }
        if (out_mode == OUT_PLANAR_F32) {
            if (ntiles != 1 || r != 1 || cout_valid < 1 || cout_valid > 16 || add || mask) return (int)hipErrorInvalidValue;
            if (cout_valid <= 4) return launch_thin_rows(x, wp, bias, (float*)out, B, H, W, cout_valid, relu, s);
            return launch_persistent<1, OUT_PLANAR_F32, 3>(x, wp, bias, nullptr, nullptr, out, B, H, W, 1, 1, cout_valid, relu, s);
        }
        return (int)hipErrorInvalidValue;
    }
    if (out_mode == OUT_NHWC_BF16) {
        if (ntiles != r * r || r < 1) return (int)hipErrorInvalidValue;
        const size_t lds = in_tile_bytes(3) + 2 * 64 * 128;
        conv3x3_c64_kernel<4, OUT_NHWC_BF16, 3><<<dim3((unsigned)nblk), dim3(256), lds, s>>>(
            (const bf16_t*)x, (const bf16_t*)wp, bias, (const bf16_t*)add, (const bf16_t*)mask, out, H, W, ntiles, r,
            64, relu, tilesX, tilesY, in_r);
    } else if (out_mode == OUT_PLANAR_F32) {
        if (ntiles != 1 || r != 1 || cout_valid < 1 || cout_valid > 16 || add || mask) return (int)hipErrorInvalidValue;
        const size_t lds = in_tile_bytes(3) + 2 * 16 * 128;
        conv3x3_c64_kernel<1, OUT_PLANAR_F32, 3><<<dim3((unsigned)nblk), dim3(256), lds, s>>>(
            (const bf16_t*)x, (const bf16_t*)wp, bias, nullptr, nullptr, out, H, W, 1, 1, cout_valid, relu, tilesX,
            tilesY, in_r);
    } else {
        return (int)hipErrorInvalidValue;
    }
    TUP_CHECK_LAUNCH();
    return 0;
}

// Composed branch A for inference: Upsampler's last conv (64 -> 64*r*r, +bias), PixelShuffle(r) and
// up1_conv (64 -> 3, no bias, ReLU) (reference utils.py:62-63,74-75,83-84 + utils.py:32-40, called at
// model.py:264-265) have no non-linearity between them, so they are ONE linear map from the 64-channel LR
// map to the 3-channel HR image: a 5x5 (LR taps) conv with 3*r*r outputs written through PixelShuffle.
// K = 25*64 = 1600 and N = 3*r*r replace K = 576, N = 64*r*r followed by an HR 64->3 conv (12x fewer
// FLOPs at r = 2) and the 64-channel HR tensor never exists.  Exactness: the composition is exact in
// real arithmetic except on the outermost HR pixel ring, where the reference zero-pads the HR
// intermediate; those pixels are recomputed with per-border weight variants (wv/bv).
// x bf16 NHWC [B][H][W][64]; wp bf16 [25][rows][64] (rows = 16/32/112 for r = 2/3/6, row n = c*r*r+si*r+sj);
// bias fp32 [3rr]; wv bf16 [9][3rr][25][64], bv fp32 [9][3rr] (variant = rowmode*3+colmode, mode 0 interior,
// 1 first row/col, 2 last row/col); out fp32 [B][3][H*r][W*r].
// wp / wv must come from a composition (packing.pack_branch_a, tup_bra_compose): output (si, sj)'s kernel is supported on the tap
// rows / columns floor((s + d - 1) / r) + 1 .. + 3 over the 64->3 conv's taps d the variant keeps.  The border ring (wv, every r)
// and the r = 2 row GEMM (wp: tap row 4 / 0 dead for si = 0 / 1, tap column 4 / 0 for sj = 0 / 1) read only the taps inside each
// output's support and ignore whatever the other taps hold; the dense r = 3 / 6 kernels multiply through all 25.
// r = 2: out must be 8-byte aligned (the two sj of an HR row leave in one store).
extern "C" int tup_conv5x5_c64_planar_fwd(const void* x, const void* wp, const float* bias, const void* wv,
                                          const float* bv, float* out, int B, int H, int W, int r, int relu,
                                          void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    if (!(r == 2 || r == 3 || r == 6)) return (int)hipErrorInvalidValue;
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    const long long nblk = (long long)tilesX * tilesY * B;
    if (nblk > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nout = 3 * r * r;
    if (r == 2) {
        const int e = launch_bra_rows(x, wp, bias, out, B, H, W, relu, s);
        if (e) return e;
    } else if (r == 3) {
        const size_t lds = in_tile_bytes(5) + 2 * 32 * 128;
        TUP_SET_DYN_LDS((conv3x3_c64_kernel<2, OUT_PLANAR_F32, 5>), lds);
        conv3x3_c64_kernel<2, OUT_PLANAR_F32, 5><<<dim3((unsigned)nblk), dim3(256), lds, s>>>(
            (const bf16_t*)x, (const bf16_t*)wp, bias, nullptr, nullptr, out, H, W, 1, r, nout, relu, tilesX, tilesY, 1);
    } else {
        const size_t lds = in_tile_bytes(5) + 2 * 112 * 128;
        TUP_SET_DYN_LDS((conv3x3_c64_kernel<7, OUT_PLANAR_F32, 5>), lds);
        conv3x3_c64_kernel<7, OUT_PLANAR_F32, 5><<<dim3((unsigned)nblk), dim3(256), lds, s>>>(
            (const bf16_t*)x, (const bf16_t*)wp, bias, nullptr, nullptr, out, H, W, 1, r, nout, relu, tilesX, tilesY, 1);
    }
    TUP_CHECK_LAUNCH();
    const long long per_img = 2LL * W * r + 2LL * (H * r - 2);                  // HR ring pixels of one image, four to a workgroup
    if (per_img > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const dim3 ring_grid((unsigned)((per_img + 3) / 4), (unsigned)(B < 65535 ? B : 65535));
    const bf16_t* xb = (const bf16_t*)x; const bf16_t* wvb = (const bf16_t*)wv;
    if (r == 2) conv5x5_border_fix_kernel<2><<<ring_grid, dim3(256), 0, s>>>(xb, wvb, bv, out, B, H, W, relu);
    else if (r == 3) conv5x5_border_fix_kernel<3><<<ring_grid, dim3(256), 0, s>>>(xb, wvb, bv, out, B, H, W, relu);
    else conv5x5_border_fix_kernel<6><<<ring_grid, dim3(256), 0, s>>>(xb, wvb, bv, out, B, H, W, relu);
    TUP_CHECK_LAUNCH();
    return 0;
}

#ifdef TUP_DIAG
// Timing experiments only (`make diag`): the s_memtime stamps of the last launch under TUP_CONV_STAMPS=1 (2 groups x 16 phases x 5).
extern "C" int tup_debug_conv_stamps(unsigned long long* host_out)
{
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(tup_conv_stamps), sizeof(unsigned long long) * 2 * 16 * 5);
}
#endif
