// Training samples of a whole batch in one launch: random HR crops with one of the 8 flip / rotate variants and their LR
// counterparts (data.PatchSampler; the reference trains on whole frames only, data_handling/data_class.py:24-75).
//
// Per 32-byte record {frame, H, W, y0, x0, op}, with P the HR and p the LR patch side (P = p * s, square patches):
//   t  = frame[y0:y0+P, x0:x0+P]                                  frame: contiguous uint8 [H][W][3]
//   op & 1: t = t[:, ::-1];  op & 2: t = t[::-1];  op & 4: t = t.transpose(1, 0, 2)     (in that order)
//   hr = ToTensor(t)                                              (float)v / 255.0f, fp32 planar [3][P][P]
//   lr = ToTensor(Image.resize((p, p), BILINEAR)(t))              Pillow's 8-bit two-pass resampler as image_io.hip states it
// bit-exact.  Pillow's horizontal pass runs over the TRANSFORMED image and is rounded to uint8 before the vertical pass, so the
// transpose does not commute with the resize (1 LSB apart at every scale): with op & 4 the rounded first pass runs along the frame's
// vertical axis.  Nothing here special-cases that: the window is staged in LDS in t's own coordinates and both passes run on t.
//
// A workgroup owns one 16 x 16 LR tile of one sample and the (16 s)^2 HR pixels under it:
//   1. stage the source window (the tile's HR square plus the filter halo, at most s (16 + 1) pixels a side) from the frame into
//      LDS through the index map: whole aligned dwords along the frame's rows (a row of a crop starts at any byte), scattered as
//      bytes to their place in t;
//   2. write the HR share (16-byte stores per plane where P and the base allow it) and run the first pass into a uint8 LDS tile
//      -- that intermediate never reaches memory;
//   3. run the second pass and write the LR tile.
// One table serves both passes (square patch).  Every output element has exactly one writer: no atomics, no workspace.
// Bound: HBM and launch latency -- 3 P^2 bytes read, 12 P^2 + 12 p^2 written per sample, ~27 integer multiply-adds per LR value;
// a batch of 64 patches moves a few MB, so one launch replaces what is otherwise several hundred launch-bound ones.
#include "common.h"

struct PatchRec {
    const uint8_t* frame;
    int H, W, y0, x0, op, reserved;
};
static_assert(sizeof(PatchRec) == 32, "patch record = 32 bytes (the host packs it as one int64 and six int32 words)");

namespace {
constexpr int PP_TILE = 16;                       // LR tile side
constexpr int PP_PRECISION_BITS = 32 - 8 - 2;     // Pillow's PRECISION_BITS for 8-bit images
constexpr int PP_MAX_LDS = 64 * 1024;

__device__ __forceinline__ uint32_t pp_clip8(int v) { v >>= PP_PRECISION_BITS; return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// bytes of dynamic LDS for window side wmax: window [wmax][wmax][3] + first-pass tile [wmax][16][3] (both rounded up to dwords),
// then the two tap-table slices int [16][ksize]
__host__ __device__ inline int pp_win_bytes(int wmax) { return (wmax * wmax * 3 + 3) & ~3; }
__host__ __device__ inline int pp_tmp_bytes(int wmax) { return (wmax * PP_TILE * 3 + 3) & ~3; }

__global__ __launch_bounds__(256) void patch_pairs_kernel(const PatchRec* __restrict__ recs, int P, int p, int wmax,
                                                          const int* __restrict__ xmin, const int* __restrict__ xsize,
                                                          const int* __restrict__ kk, int ksize,
                                                          float* __restrict__ hr, float* __restrict__ lr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t pp_lds[];
    uint8_t* win = pp_lds;                                              // [wr][wc][3], t's coordinates
    uint8_t* tmp = pp_lds + pp_win_bytes(wmax);                         // [wr][tw][3], the first pass
    int* kx = reinterpret_cast<int*>(tmp + pp_tmp_bytes(wmax));         // [16][ksize] taps of the tile's columns
    int* ky = kx + PP_TILE * ksize;                                     // ... and of its rows

    const int b = blockIdx.y, tid = threadIdx.x;
    const PatchRec rec = recs[b];
    // a box that leaves its frame is never read (ops.patch_pairs refuses it on the host; this keeps a bad table off the device)
    if (rec.y0 < 0 || rec.x0 < 0 || rec.y0 > rec.H - P || rec.x0 > rec.W - P || (rec.op & ~7)) return;

    const int ntx = (p + PP_TILE - 1) / PP_TILE, s = P / p;
    const int tx0 = (blockIdx.x % ntx) * PP_TILE, ty0 = (blockIdx.x / ntx) * PP_TILE;
    const int tw = min(PP_TILE, p - tx0), th = min(PP_TILE, p - ty0);
    // the window of t: the taps of the tile's outputs, which cover the HR square under it (tables of pil_bilinear_coeffs(P, p))
    const int c_lo = min(max(xmin[tx0], 0), P), r_lo = min(max(xmin[ty0], 0), P);
    const int wc = min(min(max(xmin[tx0 + tw - 1] + xsize[tx0 + tw - 1], s * (tx0 + tw)), P) - c_lo, wmax);
    const int wr = min(min(max(xmin[ty0 + th - 1] + xsize[ty0 + th - 1], s * (ty0 + th)), P) - r_lo, wmax);

    for (int i = tid; i < PP_TILE * ksize; i += 256) {
        const int o = i / ksize, j = i - o * ksize;
        kx[i] = o < tw ? kk[(size_t)(tx0 + o) * ksize + j] : 0;
        ky[i] = o < th ? kk[(size_t)(ty0 + o) * ksize + j] : 0;
    }

    // ---- 1. frame -> LDS.  u = t before the transpose: u[a][b], a rectangle [a0, a0 + na) x [b0, b0 + nb) of the crop ----
    {
        const bool tr = rec.op & 4, fy = rec.op & 2, fx = rec.op & 1;
        const int a0 = tr ? c_lo : r_lo, na = tr ? wc : wr, b0 = tr ? r_lo : c_lo, nb = tr ? wr : wc;
        const int fa0 = fy ? P - a0 - na : a0, fb0 = fx ? P - b0 - nb : b0;          // its lowest frame row / column inside the crop
        const int nbytes = nb * 3, nwords = (nbytes + 6) >> 2;                        // dwords a row can touch at any misalignment
        const size_t pitch = (size_t)rec.W * 3;
        const uint8_t* base = rec.frame + ((size_t)(rec.y0 + fa0) * rec.W + (rec.x0 + fb0)) * 3;
        for (int i = tid; i < na * nwords; i += 256) {
            const int ia = i / nwords, iw = i - ia * nwords;
            const uint8_t* row = base + (size_t)ia * pitch;
            const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
            const int e0 = iw * 4 - mis;                                              // row byte of this dword's byte 0
            if (e0 >= nbytes) continue;
            // an aligned dword that holds at least one byte of the row lies inside the row's page: reading it whole cannot fault
            const uint32_t w = *reinterpret_cast<const uint32_t*>(row + e0);
            const int a = fy ? a0 + na - 1 - ia : a0 + ia;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = e0 + j;
                if (e < 0 || e >= nbytes) continue;
                const int ib = e / 3, ch = e - ib * 3;
                const int bb = fx ? b0 + nb - 1 - ib : b0 + ib;
                const int r = tr ? bb : a, c = tr ? a : bb;
                win[((r - r_lo) * wc + (c - c_lo)) * 3 + ch] = (uint8_t)(w >> (8 * j));
            }
        }
    }
    __syncthreads();

    // ---- 2a. the HR share: rows [s ty0, s (ty0 + th)), columns [s tx0, s (tx0 + tw)) of t, / 255 ----
    {
        const int R0 = s * ty0, C0 = s * tx0, nR = s * th, nC = s * tw;
        const size_t plane = (size_t)P * P;
        float* h = hr + (size_t)b * 3 * plane;
        if ((P & 3) == 0 && (reinterpret_cast<uintptr_t>(hr) & 15) == 0) {            // C0 and nC are multiples of 4 then
            const int nq = nC >> 2;
            for (int i = tid; i < nR * nq; i += 256) {
                const int y = i / nq, q = i - y * nq;
                const uint8_t* sp = win + ((R0 + y - r_lo) * wc + (C0 + 4 * q - c_lo)) * 3;
                f32x4 o0, o1, o2;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o0[j] = (float)sp[3 * j] / 255.0f; o1[j] = (float)sp[3 * j + 1] / 255.0f; o2[j] = (float)sp[3 * j + 2] / 255.0f;
                }
                float* d = h + (size_t)(R0 + y) * P + C0 + 4 * q;
                *reinterpret_cast<f32x4*>(d) = o0;
                *reinterpret_cast<f32x4*>(d + plane) = o1;
                *reinterpret_cast<f32x4*>(d + 2 * plane) = o2;
            }
        } else {
            for (int i = tid; i < nR * nC; i += 256) {
                const int y = i / nC, x = i - y * nC;
                const uint8_t* sp = win + ((R0 + y - r_lo) * wc + (C0 + x - c_lo)) * 3;
                float* d = h + (size_t)(R0 + y) * P + C0 + x;
                d[0] = (float)sp[0] / 255.0f; d[plane] = (float)sp[1] / 255.0f; d[2 * plane] = (float)sp[2] / 255.0f;
            }
        }
    }

    // ---- 2b. Pillow's horizontal pass over the window's rows, rounded to uint8: tmp[r][ox] ----
    for (int i = tid; i < wr * tw; i += 256) {
        const int r = i / tw, ox = i - r * tw;
        const int lo = xmin[tx0 + ox], n = min(xsize[tx0 + ox], ksize);
        const uint8_t* sp = win + (r * wc + (lo - c_lo)) * 3;
        const int* k = kx + ox * ksize;
        int s0 = 1 << (PP_PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int j = 0; j < n; ++j) {
            const int kv = k[j];
            s0 += (int)sp[3 * j] * kv; s1 += (int)sp[3 * j + 1] * kv; s2 += (int)sp[3 * j + 2] * kv;
        }
        uint8_t* d = tmp + (r * tw + ox) * 3;
        d[0] = (uint8_t)pp_clip8(s0); d[1] = (uint8_t)pp_clip8(s1); d[2] = (uint8_t)pp_clip8(s2);
    }
    __syncthreads();

    // ---- 3. the vertical pass and ToTensor: the LR tile ----
    {
        const size_t plane = (size_t)p * p;
        float* l = lr + (size_t)b * 3 * plane;
        for (int i = tid; i < th * tw; i += 256) {
            const int oy = i / tw, ox = i - oy * tw;
            const int lo = xmin[ty0 + oy], n = min(xsize[ty0 + oy], ksize);
            const uint8_t* sp = tmp + ((lo - r_lo) * tw + ox) * 3;
            const int* k = ky + oy * ksize;
            int s0 = 1 << (PP_PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int j = 0; j < n; ++j) {
                const int kv = k[j];
                const uint8_t* q = sp + j * tw * 3;
                s0 += (int)q[0] * kv; s1 += (int)q[1] * kv; s2 += (int)q[2] * kv;
            }
            float* d = l + (size_t)(ty0 + oy) * p + tx0 + ox;
            d[0] = (float)pp_clip8(s0) / 255.0f; d[plane] = (float)pp_clip8(s1) / 255.0f; d[2 * plane] = (float)pp_clip8(s2) / 255.0f;
        }
    }
}
}  // namespace

// recs: device array [B] of 32-byte records {const uint8_t* frame; int H; int W; int y0; int x0; int op; int reserved};
// xmin / xsize int32 [p], k int32 [p][ksize] = resize_taps.pil_bilinear_coeffs(P, p); hr fp32 [B][3][P][P], lr fp32 [B][3][p][p].
extern "C" int tup_patch_pairs(const void* recs, int B, int P, int p, const int* xmin, const int* xsize, const int* k, int ksize,
                               float* hr, float* lr, void* stream)
{
    if (B <= 0) return 0;
    if (B > 65535 || ksize < 1 || P < p || p < 1 || P % p != 0) return (int)hipErrorInvalidValue;
    // the taps of 16 consecutive outputs span at most s * 15 + ksize source pixels (xmin steps by s, xsize <= ksize)
    const long long span = (long long)(P / p) * (PP_TILE - 1) + ksize;
    const long long wmax = span < P ? span : P;
    if (wmax > 1024) return (int)hipErrorInvalidValue;
    const long long lds = (long long)pp_win_bytes((int)wmax) + pp_tmp_bytes((int)wmax) + 2LL * PP_TILE * ksize * (long long)sizeof(int);
    if (lds > PP_MAX_LDS) return (int)hipErrorInvalidValue;                          // scales up to 8 fit (63 KiB at s = 8)
    const int nt = (p + PP_TILE - 1) / PP_TILE;
    if ((long long)nt * nt > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    patch_pairs_kernel<<<dim3((unsigned)(nt * nt), (unsigned)B), dim3(256), (size_t)lds, reinterpret_cast<hipStream_t>(stream)>>>(
        (const PatchRec*)recs, P, p, (int)wmax, xmin, xsize, k, ksize, hr, lr);
    TUP_CHECK_LAUNCH();
    return 0;
}
