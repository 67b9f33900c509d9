// Inference: conv1 (3->64, +bias, ReLU) and conv2 (64->64, +bias, ReLU) without the 64-channel map between them ever reaching
// HBM (reference models/FastTransformer/model.py:202-204,251-252).
//
// conv1_compact_kernel   fp32 planar [B][3][H][W] -> bf16 [B][Hp][Wp][4] (channel 3 = 0), the image at (+2, +2) inside a
//                        zero border, Hp = 8 tilesY + 4, Wp = 32 tilesX + 4: every conv2 tile's 12 x 36 input halo is in range
//                        and conv1's zero padding is already in the data.  8 B per pixel; each value is the bf16 conv1 stages
//                        (f32_to_bf16 in conv_thin.hip).
// conv12_fused_kernel    the persistent ping-pong conv of conv_pingpong.h: tile walk, K loop and weight staging are the ones
//                        conv_c64_persistent_kernel<4,0,3> uses, the store phase is that kernel's with ReLU.  What this kernel adds
//                        is its phase loop: the idle wave group does not DMA-fetch its next 10 x 34 feat1 halo image but
//                        computes it:
//   * the halo is cut into 22 runs of 16 pixels in image order (q = 16 G + p, G = wave + 4 j): 6 runs for waves 0 / 1, 5 for 2 / 3;
//   * lane (g, p) needs conv1's k = 8 g .. 8 g + 7, k = (dy 3 + dx) 3 + c.  It loads five words of four pixels of the compact
//     copy (S0.hi, S1, S2, S3, S4.lo; which pixel each slot is depends on g only, a table in LDS) and forms the four
//     fragment words as v_perm_b32(S_{i+1}.lo, S_i.hi, sel_i(g)) -- a word of conv1's B operand is always either two channels
//     of one pixel or channel 2 of one pixel and channel 0 of the next, and the pad channel / selector 0x0c supply k >= 27;
//   * 4 x mfma16x16x32 with conv1's packed weights and the bias as the accumulator input (as conv3x3_c3_persistent_kernel), ReLU
//     and bf16 as v_cvt_pk_bf16_f32 + v_pk_max_i16 (bit-identical to fmaxf + pack for every non-NaN value), zero for halo pixels
//     outside the image (conv2's padding, not ReLU(bias)), two ds_write_b128 into the swizzled slots of the image;
//   * the compact-copy loads (and conv1's A fragments) are issued BEFORE the finished tile's stores: vmcnt retires in order, so
//     loads issued behind the stores would wait for the stores' write latency.
// Every run reads only what its own wave loads, so no wave of the group waits for another before the phase barrier.
#include "conv_pingpong.h"

namespace {

constexpr int TH = 8, TW = 32, HALO_W = TW + 2, HALO_H = TH + 2, NPIX_HALO = HALO_H * HALO_W;
constexpr int IN_BYTES = NPIX_HALO * 128;
constexpr int WROWS = 64, WSLAB = WROWS * 128;
constexpr int NRUNS = (NPIX_HALO + 15) / 16;                 // 22 runs of 16 halo pixels
constexpr int RUNS_PER_WAVE = (NRUNS + 3) / 4;               // 6
// [9 taps][64 rows][128 B] conv2 weights | 2 x halo image | conv2 bias [64] | conv1 bias [64] | per-g slot table [4][16] words
constexpr size_t C12_LDS = (size_t)9 * WSLAB + 2 * (size_t)IN_BYTES + 256 + 256 + 256;
static_assert(C12_LDS <= 163840, "LDS budget");

__global__ __launch_bounds__(256) void conv1_compact_kernel(const float* __restrict__ x, u32x2* __restrict__ xc, int H, int W,
                                                            int Hp, int Wp)
{
    const int xp = blockIdx.y * 256 + threadIdx.x;
    if (xp >= Wp) return;
    const int row = blockIdx.x, b = row / Hp, yp = row - b * Hp;        // row = b * Hp + yp
    const int iy = yp - 2, ix = xp - 2;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const size_t plane = (size_t)H * W;
        const float* s = x + (size_t)b * 3 * plane + (size_t)iy * W + ix;
        v0 = s[0]; v1 = s[plane]; v2 = s[2 * plane];
    }
    xc[(size_t)row * Wp + xp] = u32x2{pack_bf16x2(v0, v1), pack_bf16x2(v2, 0.f)};
}

__global__ __launch_bounds__(512, 2) void conv12_fused_kernel(
    const bf16_t* __restrict__ xc, const bf16_t* __restrict__ w1, const float* __restrict__ b1,
    const bf16_t* __restrict__ wp, const float* __restrict__ bias, bf16_t* __restrict__ out,
    int B, int H, int W, int Wp, int img_bytes, int tilesX, int tilesY)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* w_lds = smem;                              // [9][64 rows][128 B]
    char* in_lds = smem + 9 * WSLAB;                 // [2 groups][IN_BYTES]

    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int g = lane >> 4, p = lane & 15;
    const int total_tiles = tilesX * tilesY * B;
    char* my_in = in_lds + grp * IN_BYTES;
    float* bias_lds = reinterpret_cast<float*>(in_lds + 2 * IN_BYTES);      // conv2 bias, then conv1 bias
    uint32_t* tab_lds = reinterpret_cast<uint32_t*>(in_lds + 2 * IN_BYTES + 512);

    // ---- conv2's fragment addresses (its K loop: k_loop<4, 9>) ----
    uint32_t poff[9][2];
    pixel_frag_offsets<3, HALO_W>(poff, my_in, wave, g, p);
    const uint32_t wbase0 = weight_frag_base(w_lds, g, p);

    f32x4 acc[4][4];
    const uint32_t bias_addr = lds_addr(bias_lds) + (uint32_t)(g * 64);

    // ---- store phase: as conv_c64_persistent_kernel<4,0,3> with relu (8 stores per wave, out-of-image lanes to the sink) ----
    auto store_tile = [&](const TC& c) {
#pragma unroll
        for (int pg = 0; pg < 4; ++pg) {
            const int oy = c.ty * TH + 2 * wave + (pg >> 1);
            const int ox = c.tx * TW + (pg & 1) * 16 + p;
            const bool ok = oy < H && ox < W;
            const size_t eoff = (((size_t)c.b * H + oy) * W + ox) * 64 + g * 16;
            uint32_t pk[8];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                pk[ct * 2 + 0] = relu_pack_bf16x2(acc[pg][ct][0], acc[pg][ct][1]);
                pk[ct * 2 + 1] = relu_pack_bf16x2(acc[pg][ct][2], acc[pg][ct][3]);
            }
            bf16_t* o = ok ? out + eoff : reinterpret_cast<bf16_t*>(tup_store_sink) + lane * 16;
            *reinterpret_cast<u32x4*>(o) = u32x4{pk[0], pk[1], pk[2], pk[3]};
            *reinterpret_cast<u32x4*>(o + 8) = u32x4{pk[4], pk[5], pk[6], pk[7]};
        }
    };

    // ---- the idle group's conv1: loads (issued before the stores), then the runs ----
    // Everything per-lane here is rebuilt from lane_id_fresh() each phase: hoisted out of the phase loop it would stay live
    // across conv2's K loop (which sits near the 256-register limit) and spill.
    struct Conv1In { uint32_t raw[RUNS_PER_WAVE][8]; bf16x8 a[4]; };
    auto issue_conv1_loads = [&](const TC& c, Conv1In& in) {
        const int l = lane_id_fresh(), lg = l >> 4, lp = l & 15;
        // conv1's A fragments: row ct*16 + p, k = 8 g .. 8 g + 7 of the [64][32] image (L2-resident, 4 KB)
        const bf16_t* wrow = w1 + lp * 32 + lg * 8;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) in.a[ct] = *reinterpret_cast<const bf16x8*>(wrow + ct * 512);
        const u32x4 so = *reinterpret_cast<const u32x4*>(tab_lds + lg * 16);      // byte offsets of slots 0..3 (slot 4 below)
        const uint32_t so4 = tab_lds[lg * 16 + 4];
        // descriptor inputs made provably wave-uniform (otherwise hipcc wraps every buffer load in a waterfall loop)
        const int cb = __builtin_amdgcn_readfirstlane(c.b), cty = __builtin_amdgcn_readfirstlane(c.ty);
        const int ctx = __builtin_amdgcn_readfirstlane(c.tx);
        const char* img = reinterpret_cast<const char*>(xc) + (size_t)cb * img_bytes;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)img, 0, img_bytes, 0x00020000);
        const int tbase = (cty * TH * Wp + ctx * TW) * 8;          // the tile's halo origin (padded coordinates = image - 2)
#pragma unroll
        for (int j = 0; j < RUNS_PER_WAVE; ++j) {
            // waves 2, 3 have five runs: their sixth (G = 22, 23) runs on clamped addresses and writes nothing.  No branch around
            // it: with the loads conditional, hipcc's vmcnt bookkeeping merges the paths and waits for the stores as well
            const int G = wave_u + 4 * j;
            const int q = min(16 * G + lp, NPIX_HALO - 1);          // the last run is partial: its spare lanes load in range
            const int hy = (q * 241) >> 13, hx = q - hy * HALO_W;   // q / 34 exactly for q < 352
            const int pix = (hy * Wp + hx) * 8;
            uint32_t* r = in.raw[j];
            r[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, pix + (int)so[0] + 4, tbase, 0);
            const u32x2 s1 = __builtin_amdgcn_raw_buffer_load_b64(rs, pix + (int)so[1], tbase, 0);
            const u32x2 s2 = __builtin_amdgcn_raw_buffer_load_b64(rs, pix + (int)so[2], tbase, 0);
            const u32x2 s3 = __builtin_amdgcn_raw_buffer_load_b64(rs, pix + (int)so[3], tbase, 0);
            r[7] = __builtin_amdgcn_raw_buffer_load_b32(rs, pix + (int)so4, tbase, 0);
            r[1] = s1[0]; r[2] = s1[1]; r[3] = s2[0]; r[4] = s2[1]; r[5] = s3[0]; r[6] = s3[1];
        }
    };
    auto build_conv1 = [&](const TC& c, const Conv1In& in) {
        const int l = lane_id_fresh(), lg = l >> 4, lp = l & 15;
        const u32x4 sel = *reinterpret_cast<const u32x4*>(tab_lds + lg * 16 + 8);
        f32x4 bv[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bv[ct] = *reinterpret_cast<const f32x4*>(bias_lds + 64 + lg * 16 + ct * 4);
        const int ty0 = c.ty * TH, tx0 = c.tx * TW;
        const bool edge = !(ty0 >= 1 && ty0 + TH + 1 <= H && tx0 >= 1 && tx0 + TW + 1 <= W);      // wave-uniform
        const uint32_t img_lds = lds_addr(my_in);
#pragma unroll
        for (int j = 0; j < RUNS_PER_WAVE; ++j) {
            const int G = wave_u + 4 * j;
            const uint32_t* r = in.raw[j];
            const u32x4 bw = {__builtin_amdgcn_perm(r[1], r[0], sel[0]), __builtin_amdgcn_perm(r[3], r[2], sel[1]),
                              __builtin_amdgcn_perm(r[5], r[4], sel[2]), __builtin_amdgcn_perm(r[7], r[6], sel[3])};
            const bf16x8 bfrag = __builtin_bit_cast(bf16x8, bw);
            f32x4 a[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) a[ct] = mfma16x16x32(in.a[ct], bfrag, bv[ct]);
            uint32_t pk[8];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                pk[ct * 2 + 0] = relu_pack_bf16x2(a[ct][0], a[ct][1]);
                pk[ct * 2 + 1] = relu_pack_bf16x2(a[ct][2], a[ct][3]);
            }
            const int q = 16 * G + lp;
            if (edge) {
                const int hy = (q * 241) >> 13, hx = q - hy * HALO_W;
                const bool ok = (unsigned)(ty0 - 1 + hy) < (unsigned)H && (unsigned)(tx0 - 1 + hx) < (unsigned)W;
#pragma unroll
                for (int k = 0; k < 8; ++k) pk[k] = ok ? pk[k] : 0u;
            }
            const uint32_t a0 = img_lds + (uint32_t)swz128(q, 2 * lg), a1 = a0 ^ 16u;     // chunks 2g, 2g + 1 of pixel q
            if (q < NPIX_HALO) {
                *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(a0) = u32x4{pk[0], pk[1], pk[2], pk[3]};
                *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(a1) = u32x4{pk[4], pk[5], pk[6], pk[7]};
            }
            // one run at a time: interleaved by the scheduler, the runs' 16 accumulator registers each pile up beside the
            // loaded words, the stored tile's accumulators and conv2's resident addresses
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    const TileWalk walk(total_tiles, tilesX, tilesY, grp, true);
    const int my_count = walk.my_count, nphases = walk.nphases;
    const TC c_first = walk.first;

    stage_weights<4, 9>(w_lds, wp);
    // both biases in one pass ([g][ct][e] = channel order; stage_bias would be a second load and store for conv1's)
    if (threadIdx.x < 128) bias_lds[threadIdx.x] = threadIdx.x < 64 ? bias[threadIdx.x] : b1[threadIdx.x - 64];
    if (threadIdx.x < 64) {
        // slot table of lane group g: words 0..4 = byte offsets of pixel slots S0..S4 = (dy, dx) below, words 8..11 = the
        // v_perm selectors of fragment words 0..3.  X = {S_i channel 2, S_i+1 channel 0}, Y = {channel 1, channel 2} of one
        // pixel (S_i = S_i+1), Z = channels 0, 1 of S_i+1, F = S_i's (channel 2, pad) word, 0 = zero (k >= 27)
        constexpr uint32_t X = 0x05040100u, Y = 0x01000706u, Z = 0x07060504u, F = 0x03020100u, Zero = 0x0c0c0c0cu;
        constexpr int slot_dydx[4][5] = {{0x00, 0x00, 0x01, 0x01, 0x02}, {0x02, 0x10, 0x10, 0x11, 0x12},
                                         {0x12, 0x12, 0x20, 0x21, 0x21}, {0x22, 0x22, 0x22, 0x22, 0x22}};
        constexpr uint32_t sels[4][4] = {{Z, X, Y, Z}, {X, Y, Z, X}, {Y, Z, X, Y}, {Z, F, Zero, Zero}};
        const int gg = threadIdx.x >> 4, w = threadIdx.x & 15;
        uint32_t v = 0u;
        if (w < 5) v = (uint32_t)((((slot_dydx[gg][w] >> 4) * Wp) + (slot_dydx[gg][w] & 15)) * 8);
        else if (w >= 8 && w < 12) v = sels[gg][w - 8];
        tab_lds[threadIdx.x] = v;
    }
    __syncthreads();
    if (grp == 0 && my_count > 0) {
        Conv1In in;
        issue_conv1_loads(c_first, in);
        build_conv1(c_first, in);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    TC c_done = c_first, c_next = c_first;
    if (grp == 0) walk.advance(c_next);

    // phase ph: group (ph & 1) runs the K loop of its tile ph >> 1; the other group issues its next tile's conv1 loads, stores
    // its previous tile and builds the next tile's halo image in its (now idle) buffer.  One workgroup barrier per phase.
    for (int ph = 0; ph < nphases; ++ph) {
        const int k = ph >> 1;
        if ((ph & 1) == grp) {
            if (k < my_count) k_loop<4, 9>(acc, poff, wbase0, bias_addr);
        } else {
            const int done = grp == 0 ? k : k - 1;
            const int nxt = done + 1;
            const bool store = done >= 0 && done < my_count;
            const bool fetch = nxt < my_count;
            // three separate paths: a store that is conditional between the loads and their first use makes hipcc's vmcnt
            // bookkeeping assume the shorter path and wait for the stores too
            if (fetch && store) {
                Conv1In in;
                issue_conv1_loads(c_next, in);
                __builtin_amdgcn_sched_barrier(0);
                store_tile(c_done);
                __builtin_amdgcn_sched_barrier(0);
                build_conv1(c_next, in);
            } else if (fetch) {
                Conv1In in;
                issue_conv1_loads(c_next, in);
                build_conv1(c_next, in);
            } else if (store) {
                store_tile(c_done);
            }
            c_done = c_next;
            walk.advance(c_next);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

// Compact padded input of the fused conv1 -> conv2: x fp32 [B][3][H][W] -> xc bf16 [B][Hp][Wp][4], Hp = 8 ceil(H / 8) + 4,
// Wp = 32 ceil(W / 32) + 4 (every element written: zero border, channel 3 = 0).
extern "C" int tup_conv1_compact_fwd(const float* x, void* xc, int B, int H, int W, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int Hp = (H + TH - 1) / TH * TH + 4, Wp = (W + TW - 1) / TW * TW + 4;
    if ((long long)B * Hp > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    conv1_compact_kernel<<<dim3((unsigned)(B * Hp), (unsigned)((Wp + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        x, (u32x2*)xc, H, W, Hp, Wp);
    TUP_CHECK_LAUNCH();
    return 0;
}

// conv2(ReLU(conv1(x))) with ReLU: xc from tup_conv1_compact_fwd; w1 bf16 [64][32] + b1 fp32 [64] (tup_conv3x3_c3_fwd's packing);
// w2 bf16 [1][1][9][64][64] + b2 fp32 [1][64] (tup_conv3x3_c64_fwd's out_mode 0 packing); out bf16 NHWC [B][H][W][64].
extern "C" int tup_conv12_fused_fwd(const void* xc, const void* w1, const float* b1, const void* w2, const float* b2, void* out,
                                    int B, int H, int W, void* stream)
{
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    const int Hp = tilesY * TH + 4, Wp = tilesX * TW + 4;
    const long long nt = (long long)tilesX * tilesY * B;
    // buffer-resource byte offsets are 32-bit and per image
    if (nt > 0x7fffffffLL || (long long)Hp * Wp * 8 > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TUP_SET_DYN_LDS(conv12_fused_kernel, C12_LDS);
    const int grid = (int)(nt < 256 ? nt : 256);                 // one workgroup per CU
    conv12_fused_kernel<<<dim3(grid), dim3(512), C12_LDS, s>>>((const bf16_t*)xc, (const bf16_t*)w1, b1, (const bf16_t*)w2, b2,
                                                               (bf16_t*)out, B, H, W, Wp, Hp * Wp * 8, tilesX, tilesY);
    TUP_CHECK_LAUNCH();
    return 0;
}
