// The persistent "ping-pong" convolution skeleton (device code only), shared by conv_c64_persistent_kernel and
// bra_rows_persistent_kernel (conv3x3_c64.hip), decoder_fused_kernel (decoder_fused.hip) and conv12_fused_kernel
// (conv12_fused.hip): one 8-wave workgroup per CU walks the pixel tiles; its two wave groups (waves 0-3 / 4-7, one wave of each per
// SIMD) own one halo image in LDS each and run half a period apart -- while one group runs a barrier-free K loop out of LDS, the
// other stores its previous tile and fetches its next halo image by LDS-DMA, then they swap.
//
// Here: the tile walk, the halo-image DMA, the fragment address table and the 3-slot K loop, weight / bias staging, and the small
// things the store phases share.  NOT here: the phase loops and the store phases.  They differ exactly where the hand-counted
// s_waitcnt vmcnt(N) live (how many stores / loads each kernel issues behind the DMA), so every kernel keeps its own.
#pragma once
#include "common.h"

namespace {

// DMA source of halo chunks outside the image (HaloDma::prefetch's `zero`).
[[maybe_unused]] __device__ __attribute__((aligned(16))) unsigned int tup_zero_line[4] = {0u, 0u, 0u, 0u};
// Store sink for lanes whose pixel is outside the image: keeps the number of store instructions per wave fixed (the counted
// vmcnt of the phase loops relies on it); never read.
[[maybe_unused]] __device__ __attribute__((aligned(16))) unsigned int tup_store_sink[64 * 8];

// acc += (v of lane p + n of the same 16-lane row, 0 past its end) / (v of lane p - n, 0 before its start): one v_add_f32 with a DPP
// source (hipcc keeps a v_mov_b32_dpp + v_add_f32 pair per term: 154 instead of 82 instructions in branch A's store phase, and every
// VALU instruction of that phase takes issue cycles from the other group's MFMA stream on the same SIMD)
#define TUP_ADD_DPP(acc, v, ctrl) asm("v_add_f32_dpp %0, %1, %0 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(acc) : "v"(v))

// ReLU'd bf16 pair: ONE v_cvt_pk_bf16_f32 (RNE, the rounding of pack_bf16x2) + v_pk_max_i16 against 0 (a negative bf16 is a negative
// int16).  pack_bf16x2's two scalar conversions compile to two v_cvt_pk_bf16_f32 and a v_perm_b32.
TUP_DEVICE uint32_t relu_pack_bf16x2(float lo, float hi) {
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, v), s16x2{0, 0}));
}

// ---- tile walk ----
// Tiles of one workgroup: first, first + stride, ... < limit.  Workgroups go to the eight XCDs round-robin (blockIdx & 7), each
// with its own L2: when the grid is a multiple of 8, an XCD takes one contiguous eighth of the tile list and its workgroups walk
// it side by side, so the halo a tile shares with its left / right neighbours (same moment) and with the tile row above is found
// in THAT L2 instead of crossing the fabric once per XCD.  Otherwise (or with use_bands off) tiles go round-robin.
TUP_DEVICE void xcd_band(int total, bool use_bands, int& first, int& stride, int& limit) {
    if ((gridDim.x & 7) == 0 && use_bands) {
        const int band = (total + 7) >> 3, start = (blockIdx.x & 7) * band;
        limit = min(total, start + band);
        first = start + (blockIdx.x >> 3);
        stride = gridDim.x >> 3;
    } else {
        limit = total; first = blockIdx.x; stride = gridDim.x;
    }
}

// Tile coordinates are carried, not decoded: a tile index -> (tx, ty, b) decode is two integer divisions = ~30 VALU instructions
// each even for a wave-uniform value, twice per phase, and every VALU instruction of the idle wave group costs the other group's
// K loop ~5 cycles of MFMA issue.  A group's tiles advance by a fixed stride: one carry chain per phase.
struct TC { int tx, ty, b; };

// The two-group walk: wave group `grp` takes every second tile of the workgroup's list.
struct TileWalk {
    int my_count;                // tiles of this group
    int nphases;                 // uniform for the whole workgroup: 2 * (group 0's count, >= group 1's) + 1
    TC first;                    // this group's first tile
    int tilesX, tilesY, step_x, step_y, step_b;

    TUP_DEVICE TileWalk(int total_tiles, int tilesX_, int tilesY_, int grp, bool use_bands) : tilesX(tilesX_), tilesY(tilesY_) {
        int first0, per, limit;
        xcd_band(total_tiles, use_bands, first0, per, limit);
        const int first_tile = first0 + grp * per, stride = 2 * per;
        my_count = first_tile < limit ? (limit - first_tile + stride - 1) / stride : 0;
        const int cnt0 = first0 < limit ? (limit - first0 + stride - 1) / stride : 0;
        nphases = 2 * cnt0 + 1;
        first.tx = first_tile % tilesX; const int t = first_tile / tilesX; first.ty = t % tilesY; first.b = t / tilesY;
        step_x = stride % tilesX; step_y = (stride / tilesX) % tilesY; step_b = stride / (tilesX * tilesY);
    }
    TUP_DEVICE void advance(TC& c) const {            // + stride tiles
        c.tx += step_x;
        if (c.tx >= tilesX) { c.tx -= tilesX; ++c.ty; }
        c.ty += step_y; c.b += step_b;
        if (c.ty >= tilesY) { c.ty -= tilesY; ++c.b; }
    }
};

// ---- halo-image DMA ----
// One 256-thread wave group fetches the HALO_H x HALO_W pixel image (128-B NHWC pixels, PAD halo pixels on every side) of the tile
// at (ty0, tx0) into LDS by global_load_lds_dwordx4: the per-lane source address carries the XOR swizzle and the halo clipping,
// out-of-image lanes read the zero line.  The (pixel, chunk) -> source-offset map of a lane's pieces does not depend on the tile, so
// it is computed once (rel[]); an interior tile then costs one 64-bit add + one DMA per piece.  (The issuing group shares its SIMDs
// with the other group's MFMA stream and gets roughly one VALU issue per 12-18 cycles: the ~30 address instructions per piece of
// the general path made DMA issue 4.1 k cycles of a 12.5 k-cycle phase.)  A wave issues NPIECE DMAs per tile, or NPIECE - 1 when
// the last piece is partial and the wave has no chunk in it.
// `zero` = tup_zero_line, named by the calling kernel: a __device__ variable that only device functions name gets internal
// linkage and pc-relative addressing, which takes the s_load of its address and an s_waitcnt lgkmcnt(0) out of the clipped path
// of every kernel -- a change to their instruction streams, which sharing this code is not meant to make.
template <int HALO_H, int HALO_W, int PAD>
struct HaloDma {
    static constexpr int IN_CHUNKS = HALO_H * HALO_W * 8, NPIECE = (IN_CHUNKS + 255) / 256;
    static constexpr bool LAST_PARTIAL = (IN_CHUNKS % 256) != 0;
    int rel[NPIECE];
    int tid, wave;               // inside the group
    bool last_ok;

    TUP_DEVICE HaloDma(int W, int tid_) : tid(tid_), wave(tid_ >> 6), last_ok((NPIECE - 1) * 256 + tid_ < IN_CHUNKS) {
#pragma unroll
        for (int it = 0; it < NPIECE; ++it) {
            const int idx = LAST_PARTIAL ? min(it * 256 + tid, IN_CHUNKS - 1) : it * 256 + tid;
            const int q = idx >> 3, c = (idx & 7) ^ ((q >> 1) & 7);
            const int yy = q / HALO_W, xx = q - yy * HALO_W;
            rel[it] = ((yy - PAD) * W + (xx - PAD)) * 128 + c * 16;
        }
    }
    TUP_DEVICE void prefetch(const bf16_t* x, int b, int ty0, int tx0, int H, int W, char* my_in, const void* zero) const {
        const char* xb = reinterpret_cast<const char*>(x + (size_t)b * H * W * 64);
        if (ty0 >= PAD && ty0 + HALO_H - PAD <= H && tx0 >= PAD && tx0 + HALO_W - PAD <= W) {       // interior tile
            const char* tb = xb + ((size_t)ty0 * W + tx0) * 128;
#pragma unroll
            for (int it = 0; it < NPIECE; ++it) {
                if (LAST_PARTIAL && it == NPIECE - 1 && !last_ok) continue;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(tb + rel[it]),
                                                 (__attribute__((address_space(3))) void*)(my_in + (it * 256 + wave * 64) * 16), 16, 0, 0);
            }
            return;
        }
#pragma unroll 1
        for (int base = 0; base < IN_CHUNKS; base += 256) {
            const int idx = base + tid;                     // physical 16-B chunk of the LDS image
            if (!LAST_PARTIAL || idx < IN_CHUNKS) {
                const int q = idx >> 3, cphys = idx & 7;
                const int c = cphys ^ ((q >> 1) & 7);       // logical chunk stored there (swizzle on the SOURCE side)
                const int yy = q / HALO_W, xx = q - yy * HALO_W;
                const int iy = ty0 - PAD + yy, ix = tx0 - PAD + xx;
                const void* src = (iy >= 0 && iy < H && ix >= 0 && ix < W)
                                      ? (const void*)(xb + ((size_t)(iy * W + ix) * 128 + c * 16)) : zero;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(my_in + (base + wave * 64) * 16), 16, 0, 0);
            }
        }
    }
};

// ---- fragment addresses and the K loop of the KS x KS conv on an 8 x 32 pixel tile (wave w: rows 2w, 2w + 1) ----
// Fragment addresses = a few base registers + the ds_read immediate offset.  Pixel group pg = 2*row + half: the second half of a
// row is 16 pixels = 2048 B further and has the same swizzle phase ((q >> 1) & 7 is unchanged by q + 16), so the table holds the
// two rows of each tap (with the group's image base folded in; the image is 128-B aligned, so the kh = 1 form is still "^ 64").
template <int KS, int HALO_W>
TUP_DEVICE void pixel_frag_offsets(uint32_t (&poff)[KS * KS][2], const char* my_in, int wave, int g, int p) {
#pragma unroll
    for (int tap = 0; tap < KS * KS; ++tap)
#pragma unroll
        for (int rw = 0; rw < 2; ++rw)
            poff[tap][rw] = lds_addr(my_in) + (uint32_t)swz128((2 * wave + rw) * HALO_W + p + (tap / KS) * HALO_W + (tap % KS), g);
}
// Weights ([NTAPS][CT * 16 rows][128 B], swizzled): row p of slab (tap, ct) = this base + a constant.
TUP_DEVICE uint32_t weight_frag_base(const char* w_lds, int g, int p) { return lds_addr(w_lds) + (uint32_t)swz128(p, g); }

// One tile: acc[pg][ct] = bias + sum over NTAPS taps x 2 K halves, no barrier inside.  bias_addr = this lane's [ct][4] floats in LDS
// (the bias rides in the accumulator).  Fragments are requested TWO K-steps ahead (3-slot ring).  With the other group's DMA
// landing in LDS and its epilogue on the same SIMDs a ds_read_b128 takes ~500 cycles (stamped); one step (16 MFMAs = 256 cycles)
// of distance left the loop waiting on LDS: 10.4 k cycles per tile instead of the 4.6 k its MFMAs need.
template <int CT, int NTAPS>
TUP_DEVICE void k_loop(f32x4 (&acc)[4][CT], const uint32_t (&poff)[NTAPS][2], uint32_t wbase0, uint32_t bias_addr) {
    constexpr int WROWS = CT * 16;
    const uint32_t wbase1 = wbase0 ^ 64u;
    const uint32_t wbase0h = wbase0 + 57344u, wbase1h = wbase1 + 57344u;          // second window of the 16-bit offset
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[0][ct] = __builtin_bit_cast(f32x4, lds_read_b128_asm(bias_addr + ct * 16));
    lds_wait<0>();
#pragma unroll
    for (int pg = 1; pg < 4; ++pg)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[pg][ct] = acc[0][ct];
    constexpr int NSTEPS = NTAPS * 2;
    constexpr int PER = 4 + CT;                                         // ds_reads per K-step
    constexpr int NM = 4 * CT;                                          // MFMAs per K-step
    bf16x8 pf[3][4], wf[3][CT];
    auto load_one = [&](int step, int slot, int j) {                    // j = 0..3 pixel fragments, 4.. weight fragments
        const int tap = step >> 1;
        if (j < 4) {
            pf[slot][j] = (step & 1) ? lds_read_b128_asm_off_x64(poff[tap][j >> 1], (j & 1) * 2048)
                                     : lds_read_b128_asm_off(poff[tap][j >> 1], (j & 1) * 2048);
        } else {
            const int ct = j - 4;
            const int woff = (tap * WROWS + ct * 16) * 128;
            wf[slot][ct] = woff < 57344 ? lds_read_b128_asm_off((step & 1) ? wbase1 : wbase0, woff)
                                        : lds_read_b128_asm_off((step & 1) ? wbase1h : wbase0h, woff - 57344);
        }
    };
#pragma unroll
    for (int j = 0; j < PER; ++j) load_one(0, 0, j);
#pragma unroll
    for (int j = 0; j < PER; ++j) load_one(1, 1, j);
    // the requests of step + 2 are spread over the step's MFMAs (one per NM / PER of them): issued as a block at the top of the
    // step they cost the wave ~60 issue cycles per step in which its matrix pipe idles (conv2: 450 -> 425 us)
#pragma unroll
    for (int step = 0; step < NSTEPS; ++step) {
        const int cur = step % 3;
        if (step + 1 < NSTEPS) lds_wait<PER>(); else lds_wait<0>();
        __builtin_amdgcn_sched_barrier(0);
        int rd = 0;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            if (step + 2 < NSTEPS) {
#pragma unroll
                // request j goes out before MFMA m = floor(j NM / PER): every one of the PER requests is issued also when the
                // step has fewer MFMAs than requests (CT = 1: NM = 4, PER = 5; "j NM <= m PER" never issued the weight fragment
                // there); for CT = 4 (NM = 16, PER = 8) this is j = m / 2
                for (int j = 0; j < PER; ++j)
                    if (j == rd && j * NM < (m + 1) * PER) { load_one(step + 2, (step + 2) % 3, j); ++rd; }
            }
            const int pg = m / CT, ct = m % CT;
            acc[pg][ct] = mfma16x16x32(wf[cur][ct], pf[cur][pg], acc[pg][ct]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- staging into LDS (whole 512-thread workgroup; the caller's barrier publishes it) ----
// The NTAPS weight slabs of one cout tile, [tap][CT * 16 rows][64] bf16 in HBM -> swizzled 128-B rows.
template <int CT, int NTAPS>
TUP_DEVICE void stage_weights(char* w_lds, const bf16_t* wsrc) {
    for (int idx = threadIdx.x; idx < NTAPS * CT * 16 * 8; idx += 512) {
        const int row = idx >> 3, c = idx & 7;             // row = tap * WROWS + n_local
        *reinterpret_cast<u32x4*>(w_lds + swz128(row, c)) = *reinterpret_cast<const u32x4*>(wsrc + (size_t)idx * 8);
    }
}
// The bias of cout tile nt in the order the lanes read it, [g][ct][e]: channel 64 nt + 16 g + 4 ct + e (the NHWC packing), or with
// THIN channel 16 ct + 4 g + e < cout_valid (the planar packing, one cout tile).  bias may be null (zeros).
template <int CT, bool THIN>
TUP_DEVICE void stage_bias(float* bias_lds, const float* bias, int nt, int cout_valid) {
    if (threadIdx.x < 16 * CT) {
        const int gg = threadIdx.x / (4 * CT), ct = (threadIdx.x / 4) % CT, e = threadIdx.x & 3;
        float bval = 0.f;
        if (bias) {
            if constexpr (!THIN) bval = bias[nt * 64 + gg * 16 + ct * 4 + e];
            else { const int co = 16 * ct + 4 * gg + e; bval = co < cout_valid ? bias[co] : 0.f; }
        }
        bias_lds[threadIdx.x] = bval;
    }
}

}  // namespace
