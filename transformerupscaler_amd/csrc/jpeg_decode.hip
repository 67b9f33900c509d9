// Baseline sequential JPEG (SOF0) files of a whole batch decoded on the GPU: `ops.jpeg_decode`, DESIGN 7l.  Pixel for pixel what
// Pillow's Image.open(file).convert("RGB") returns (libjpeg's slow integer IDCT, fancy h2v2 upsampling, 16-bit colour conversion);
// tests/_jpeg_decode_ref.py states it in numpy and tests/test_jpeg_decode_cpu.py pins that to Pillow.  The encoder of
// jpeg_encode.hip, mirrored.
//
// The host parses the marker segments (ops.jpeg_parse) and uploads, once, a JdImage record per image (its tables as DQT / DHT carry
// them, where its scan lies) followed by the scans, each at a multiple of 16 bytes.  All images share H, W, the layout (4:4:4, 4:2:0
// or grey) and the restart interval.  Three launches, whatever the batch and the size:
//   1. jpeg_index_kernel    a workgroup per image -> segs int32 [B][S][8], the state a walker needs at the start of each of the S
//                           segments {byte, end byte, the bits already read and their number, three DC predictors, first MCU}, and
//                           status int32 [B].  With a restart interval the segments are the intervals: their starts are found by a
//                           search of the scan for FF D0 .. D7 (byte stuffing makes every such pair a marker), 16 bytes a load, a
//                           workgroup scan of the counts giving every marker its number.  Without one, a lane walks the whole scan
//                           through the Huffman codes alone and records its state at the start of every MCU row: after it the file
//                           looks like one with a restart interval of a row, except that a segment may begin mid-byte.  That walk
//                           (jd_serial_index, jpeg_index.h) has a parallel form, jpeg_sync_index_kernel (jpeg_sync.hip,
//                           tup_jpeg_decode_index_sync, ops.jpeg_decode(index="sync")): the same records by self-synchronising
//                           Huffman decoding, a lane per 132 bytes of the scan; it falls back to this walk on a damaged scan.
//   2. jpeg_blocks_kernel   a workgroup per (segment, image).  A segment is walked in chunks of at most JD_BLOCKS = 96 blocks: the
//                           workgroup stages JD_WINDOW bytes of the scan in LDS; lane 0 walks the codes (jpeg_entropy.h) and puts
//                           the quantised coefficients of whole MCUs into LDS until 96 blocks are full or less than the largest
//                           possible MCU is left of the window; then all lanes dequantise and run the column and the row IDCT
//                           (jpeg_dct.h), and store the samples as bytes into the image's workspace: the Y, Cb and Cr planes, padded
//                           to whole MCUs.  Coefficients never reach memory.
//   3. jpeg_finish_kernel   a lane per pixel: fancy upsampling of the chroma planes where 4:2:0 (it needs the chroma rows of the
//                           MCU rows above and below, which is why the planes pass through the workspace), YCbCr -> RGB, crop, and
//                           either uint8 [B][H][W][3] or fp32 [B][3][H][W] = byte / 255.
// Damaged files: the walker stops at the first bad condition (a code with no entry, a coefficient past 63, a size out of range, a
// marker or the end of the data where bits were needed) and the image's status becomes non-zero; segments the index could not place
// are skipped.  Nothing is read outside the image's scan or written outside its workspace and output; other images are unaffected.
// All integer arithmetic; all global writes are ordinary vector stores (different workgroups may store different non-zero codes into
// one image's status: any of them says "damaged").  Bound: the serial walk of lane 0 (launch 2; launch 1 unless index="sync"); DESIGN 7l has
// the times.
#include "common.h"
#include "jpeg_dct.h"
#include "jpeg_entropy.h"
#include "jpeg_index.h"

static_assert(sizeof(JdImage) == 1488, "image record = 1488 bytes (the host packs it)");

namespace {
constexpr int JD_BLOCKS = 96;                               // blocks per chunk
constexpr int JD_PITCH = 65;                                // words from one block to the next

__global__ __launch_bounds__(JD_THREADS) void jpeg_index_kernel(const JdImage* __restrict__ records, const uint8_t* __restrict__ scans,
                                                                long long scans_bytes, int layout, int interval, int mw, int total, int S,
                                                                int* __restrict__ segs, int* __restrict__ status)
{
    __shared__ JdTables tb;
    __shared__ __attribute__((aligned(16))) uint32_t win[JD_WINDOW / 4];
    __shared__ int scanbuf[2][JD_THREADS];
    __shared__ JdWalk wk;
    const int tid = threadIdx.x, b = blockIdx.x;
    const JdImage* rec = records + b;
    int* seg = segs + (size_t)b * S * JD_SEG;
    const int off = rec->scan_off, len = rec->scan_len;
    const bool tables_ok = jd_load_tables(rec, tb, tid);
    if (!tables_ok || !jd_record_ok(off, len, scans_bytes)) {                       // nothing of this image is walked
        jd_refuse_image(seg, S, status + b, tables_ok, tid);
        return;
    }
    const uint8_t* scan = scans + off;

    if (interval > 0) {
        // ---- restart markers: count, number, place ----
        const int len16 = (len + 15) & ~15;
        const int per = (((len16 + JD_THREADS - 1) / JD_THREADS) + 15) & ~15;
        const int i0 = min(tid * per, len16), i1 = min(i0 + per, len16);
        int found = 0;
        uint32_t prev = i0 > 0 ? scan[i0 - 1] : 0u;
        for (int i = i0; i < i1; i += 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(scan + i);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t cur = (v[j >> 2] >> (8 * (j & 3))) & 255u;
                found += (prev == 0xFFu && cur >= 0xD0u && cur <= 0xD7u && i + j < len) ? 1 : 0;
                prev = cur;
            }
        }
        int markers;
        int k = dg_scan256(found, scanbuf, tid, markers);
        prev = i0 > 0 ? scan[i0 - 1] : 0u;
        for (int i = i0; i < i1; i += 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(scan + i);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t cur = (v[j >> 2] >> (8 * (j & 3))) & 255u;
                if (prev == 0xFFu && cur >= 0xD0u && cur <= 0xD7u && i + j < len) {  // marker k ends segment k and starts segment k + 1
                    if (k < S) seg[(size_t)k * JD_SEG + 1] = i + j - 1;
                    if (k + 1 < S) {
                        int* s1 = seg + (size_t)(k + 1) * JD_SEG;
                        s1[0] = i + j + 1; s1[2] = 0; s1[3] = 0; s1[4] = 0; s1[5] = 0; s1[6] = 0; s1[7] = (k + 1) * interval;
                    }
                    ++k;
                }
                prev = cur;
            }
        }
        if (tid == 0) {
            seg[0] = 0; seg[2] = 0; seg[3] = 0; seg[4] = 0; seg[5] = 0; seg[6] = 0; seg[7] = 0;
            if (markers < S) seg[(size_t)markers * JD_SEG + 1] = len;               // the last segment runs to the end of the scan
            status[b] = markers == S - 1 ? JE_OK : JE_RESTARTS;
        }
        for (int q = markers + 1 + tid; q < S; q += JD_THREADS) jd_store_seg(seg + (size_t)q * JD_SEG, 0, 0, 0, -1, 0, 0, 0, 0);
        return;
    }

    // ---- no restart interval: one walk through the codes, the state at the start of every MCU row recorded ----
    jd_serial_index(scan, len, layout, mw, total, S, seg, status + b, tb, win, wk, tid);
}

struct JdBlocksShared {
    int coef[JD_BLOCKS * JD_PITCH];                         // quantised coefficients, then the column pass's output, by block
    __attribute__((aligned(16))) uint32_t win[JD_WINDOW / 4];
    JdTables tb;
    int qt[3][64];
    JdWalk wk;
};

__global__ __launch_bounds__(JD_THREADS) void jpeg_blocks_kernel(const JdImage* __restrict__ records, const uint8_t* __restrict__ scans,
                                                                 long long scans_bytes, int layout, int interval, int mw, int total, int S,
                                                                 const int* __restrict__ segs, int* __restrict__ status,
                                                                 uint8_t* __restrict__ workspace, long long ws, int yw, int yh, int cw, int ch)
{
    __shared__ JdBlocksShared sh;
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const JdImage* rec = records + b;
    const int* seg = segs + ((size_t)b * S + s) * JD_SEG;
    const int seg_pos = seg[0], seg_end = seg[1], seg_n = seg[3], mcu0 = seg[7];
    const int off = rec->scan_off, len = rec->scan_len;
    // a segment the index did not place, or one whose record it did not make: the image's status says so already
    if (seg_n < 0 || seg_n > 32 || !jd_record_ok(off, len, scans_bytes) || seg_pos < 0 || seg_end > len || seg_pos > seg_end || mcu0 < 0 || mcu0 >= total)
        return;
    if (!jd_load_tables(rec, sh.tb, tid)) return;
    if (tid < 192) sh.qt[tid >> 6][tid & 63] = rec->qt[tid >> 6][tid & 63];
    if (tid == 0) {
        sh.wk.pos = seg_pos; sh.wk.acc = seg[2]; sh.wk.n = seg_n; sh.wk.hit = 0;
        sh.wk.pred[0] = seg[4]; sh.wk.pred[1] = seg[5]; sh.wk.pred[2] = seg[6]; sh.wk.count = 0; sh.wk.err = 0;
    }
    __syncthreads();

    const uint8_t* scan = scans + off;
    const int bpm = je_blocks_per_mcu(layout), mpc = JD_BLOCKS / bpm;
    const int mcus = min(interval > 0 ? interval : mw, total - mcu0);
    uint8_t* planes = workspace + (size_t)b * (size_t)ws;
    const size_t ysize = (size_t)yw * yh, csize = (size_t)cw * ch;

    for (int done = 0; done < mcus;) {
        const int want = min(mpc, mcus - done);
        const int w0 = sh.wk.pos & ~15, wlen = min(JD_WINDOW, seg_end - w0);
        const bool final = w0 + wlen >= seg_end;
        jd_stage(scan, w0, wlen, reinterpret_cast<u32x4*>(sh.win), tid);
        for (int i = tid; i < want * bpm * JD_PITCH; i += JD_THREADS) sh.coef[i] = 0;
        __syncthreads();

        // ---- the walk: whole MCUs, as many as the chunk and the window hold ----
        if (tid == 0) {
            JeBits bits{reinterpret_cast<const uint8_t*>(sh.win), sh.wk.pos - w0, wlen, (uint32_t)sh.wk.acc, sh.wk.n, sh.wk.hit};
            int m = 0, err = 0;
            while (m < want && (final || bits.pos + JE_MCU_BYTES <= wlen)) {
                err = je_mcu(bits, sh.tb.tab, sh.tb.td, sh.tb.ta, layout, sh.wk.pred, sh.coef + m * bpm * JD_PITCH, JD_PITCH, sh.tb.zz);
                if (err) break;
                ++m;
            }
            if (!err && m == 0) err = JE_END;                                       // cannot happen: a window holds an MCU
            sh.wk.pos = w0 + bits.pos; sh.wk.acc = (int)bits.acc; sh.wk.n = bits.n; sh.wk.hit = bits.hit; sh.wk.count = m; sh.wk.err = err;
        }
        __syncthreads();
        const int m = sh.wk.count, err = sh.wk.err, nblk = m * bpm;

        // ---- dequantise and inverse DCT: columns, then rows; the samples go to the planes ----
        for (int i = tid; i < nblk * 8; i += JD_THREADS) {
            const int blk = i >> 3, c = i & 7;
            const int* q = sh.qt[je_component(layout, blk % bpm)] + c;
            int* p = sh.coef + blk * JD_PITCH + c;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k * 8] * q[k * 8];
            dg_idct8<true>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k * 8] = d[k];
        }
        __syncthreads();
        for (int i = tid; i < nblk * 8; i += JD_THREADS) {
            const int blk = i >> 3, r = i & 7, j = blk % bpm;
            const int mcu = mcu0 + done + blk / bpm, my = mcu / mw, mx = mcu - my * mw;
            const int* p = sh.coef + blk * JD_PITCH + r * 8;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[k];
            dg_idct8<false>(d);
            u32x2 o = {0u, 0u};
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k >> 2] |= (uint32_t)dg_clip255(d[k] + 128) << (8 * (k & 3));
            uint8_t* dst;
            if (layout == 2 && j < 4) dst = planes + (size_t)(my * 16 + (j >> 1) * 8 + r) * yw + mx * 16 + (j & 1) * 8;
            else if (layout == 2) dst = planes + ysize + (j - 4) * csize + (size_t)(my * 8 + r) * cw + mx * 8;
            else dst = planes + j * ysize + (size_t)(my * 8 + r) * yw + mx * 8;    // 4:4:4: the three planes have one size; grey: j = 0
            *reinterpret_cast<u32x2*>(dst) = o;
        }
        done += m;
        if (err) {
            if (tid == 0) status[b] = err;
            break;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_finish_kernel(const uint8_t* __restrict__ workspace, long long ws, int H, int W, int layout,
                                                                 int yw, int yh, int cw, int ch, uint8_t* __restrict__ out_u8,
                                                                 float* __restrict__ out_f32)
{
    const long long hw = (long long)H * W;
    const long long i = (long long)blockIdx.x * JD_THREADS + threadIdx.x;
    if (i >= hw) return;
    const int b = blockIdx.y, y = (int)(i / W), x = (int)(i - (long long)y * W);
    const uint8_t* yp = workspace + (size_t)b * (size_t)ws;
    const int Y = yp[(size_t)y * yw + x];
    int R = Y, G = Y, B = Y;
    if (layout != 4) {
        const size_t ysize = (size_t)yw * yh, csize = (size_t)cw * ch;
        const uint8_t* cbp = yp + ysize;
        const uint8_t* crp = cbp + csize;
        int cb, cr;
        if (layout == 0) {
            cb = cbp[(size_t)y * cw + x];
            cr = crp[(size_t)y * cw + x];
        } else {
            // libjpeg's fancy h2v2 upsampling over the real chroma samples, ceil(H / 2) x ceil(W / 2): rows 3 : 1 with the row above
            // (even y) or below (odd y), then columns 3 : 1 with the sample before (even x, + 8) or after (odd x, + 7), >> 4; at the
            // edges a sample is its own neighbour
            const int hc = (H + 1) >> 1, wc = (W + 1) >> 1, cy = y >> 1, cx = x >> 1;
            const int ny = (y & 1) ? min(cy + 1, hc - 1) : max(cy - 1, 0), nx = (x & 1) ? min(cx + 1, wc - 1) : max(cx - 1, 0);
            const int bias = (x & 1) ? 7 : 8;
            const size_t r0 = (size_t)cy * cw, r1 = (size_t)ny * cw;
            cb = (3 * (3 * cbp[r0 + cx] + cbp[r1 + cx]) + (3 * cbp[r0 + nx] + cbp[r1 + nx]) + bias) >> 4;
            cr = (3 * (3 * crp[r0 + cx] + crp[r1 + cx]) + (3 * crp[r0 + nx] + crp[r1 + nx]) + bias) >> 4;
        }
        cb -= 128; cr -= 128;
        R = dg_clip255(Y + ((dg_fix(1.402) * cr + 32768) >> 16));
        G = dg_clip255(Y + ((-dg_fix(.34414) * cb + 32768 - dg_fix(.71414) * cr) >> 16));
        B = dg_clip255(Y + ((dg_fix(1.772) * cb + 32768) >> 16));
    }
    if (out_u8) {
        uint8_t* d = out_u8 + ((size_t)b * (size_t)hw + (size_t)i) * 3;
        d[0] = (uint8_t)R; d[1] = (uint8_t)G; d[2] = (uint8_t)B;
    } else {
        float* d = out_f32 + (size_t)b * 3 * (size_t)hw + (size_t)i;             // tup_u8hwc_to_f32chw's rule
        d[0] = (float)R / 255.0f; d[hw] = (float)G / 255.0f; d[2 * hw] = (float)B / 255.0f;
    }
}
}  // namespace

// The number of segments S of an H x W image (what sizes segs), or -1 for what the decoder refuses: sizes outside 1..65535, a layout
// other than 0 (4:4:4) / 2 (4:2:0) / 4 (grey), a restart interval outside 0..65535 MCUs (0: none, S = the MCU rows).
extern "C" int tup_jpeg_decode_segments(int H, int W, int layout, int restart_interval)
{
    JdGeometry g;
    return jd_geometry(H, W, layout, restart_interval, g) ? g.S : -1;
}

// Launch 1: segs int32 [B][S][8] and status int32 [B] from the records (B x 1488 bytes) and the scan area (scans_bytes bytes).
extern "C" int tup_jpeg_decode_index(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout,
                                     int restart_interval, int S, int* segs, int* status, void* stream)
{
    JdGeometry g;
    if (!jd_geometry(H, W, layout, restart_interval, g) || S != g.S || !records || !scans || !segs || !status || B < 1 || B > 65535 ||
        scans_bytes < 0 || scans_bytes > 0x7fff0000LL || (reinterpret_cast<uintptr_t>(scans) & 15) || (reinterpret_cast<uintptr_t>(records) & 3))
        return (int)hipErrorInvalidValue;
    jpeg_index_kernel<<<dim3((unsigned)B), dim3(JD_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const JdImage*)records, (const uint8_t*)scans, scans_bytes, layout, restart_interval, g.mw, g.total, S, segs, status);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Launch 2: workspace uint8 [B][ws_bytes] <- the sample planes of every segment the index placed; ws_bytes = the planes of one image,
// Y (and Cb, Cr) padded to whole MCUs.
extern "C" int tup_jpeg_decode_blocks(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout,
                                      int restart_interval, int S, const int* segs, int* status, void* workspace, long long ws_bytes, void* stream)
{
    JdGeometry g;
    if (!jd_geometry(H, W, layout, restart_interval, g) || S != g.S || ws_bytes != g.ws || !records || !scans || !segs || !status || !workspace ||
        B < 1 || B > 65535 || scans_bytes < 0 || scans_bytes > 0x7fff0000LL || (reinterpret_cast<uintptr_t>(scans) & 15) ||
        (reinterpret_cast<uintptr_t>(records) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return (int)hipErrorInvalidValue;
    jpeg_blocks_kernel<<<dim3((unsigned)S, (unsigned)B), dim3(JD_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const JdImage*)records, (const uint8_t*)scans, scans_bytes, layout, restart_interval, g.mw, g.total, S, segs, status,
        (uint8_t*)workspace, ws_bytes, g.yw, g.yh, g.cw, g.ch);
    TUP_CHECK_LAUNCH();
    return 0;
}

// Launch 3: exactly one of out_u8 (uint8 [B][H][W][3], RGB) and out_f32 (fp32 [B][3][H][W] = byte / 255) <- the pixels.
extern "C" int tup_jpeg_decode_finish(const void* workspace, long long ws_bytes, int B, int H, int W, int layout, void* out_u8, float* out_f32,
                                      void* stream)
{
    JdGeometry g;
    if (!jd_geometry(H, W, layout, 0, g) || ws_bytes != g.ws || !workspace || (!out_u8) == (!out_f32) || B < 1 || B > 65535)
        return (int)hipErrorInvalidValue;
    const long long groups = ((long long)H * W + JD_THREADS - 1) / JD_THREADS;
    jpeg_finish_kernel<<<dim3((unsigned)groups, (unsigned)B), dim3(JD_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const uint8_t*)workspace, ws_bytes, H, W, layout, g.yw, g.yh, g.cw, g.ch, (uint8_t*)out_u8, out_f32);
    TUP_CHECK_LAUNCH();
    return 0;
}
