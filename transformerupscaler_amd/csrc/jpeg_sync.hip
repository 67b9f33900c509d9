// Launch 1 of `ops.jpeg_decode` for files without restart markers, as a parallel pass: the segment records of
// jpeg_index_kernel's serial walk (jpeg_decode.hip) -- the reader's state, the DC predictors and the MCU number at the start of every
// MCU row -- found by self-synchronising Huffman decoding.  jpeg_sync.h has the algorithm and what one lane does; this file is the
// workgroup around it.
//
// A workgroup per image.  The scan is taken in spans of 256 subsequences of JS_BYTES raw bytes, a lane each, staged in LDS with the few
// bytes past the span that its last symbols reach into.  Per span:
//   pass 1    every lane walks its subsequence from an assumed state; lane 0 from the true one, the span before having left it;
//   rounds    every lane whose left neighbour's exit is not the state it last started from walks again from that exit, until none
//             does.  Exit 0 is exact after pass 1 and every round makes one more exact, so the loop is bounded by the lanes of the
//             span, ends only when nothing changed, and leaves the serial walker's states, whatever the bytes;
//   sums      a lane's last walk started from its true state, so what it counted stands: workgroup prefix sums of the block ends and of
//             each component's DC differences (modulo 2^16, as je_block wraps the predictor) give the MCU number and the predictors at
//             every lane's start;
//   last pass the lanes that pass the start of an MCU row (js_first_row_block) walk once more and store the segment record at each.
// A walk notes its first error and goes on where it can (jpeg_sync.h), so a lane that only assumed its state still falls into step.  Once
// the exits stand, the first lane that still has an error is where the serial walker stops: the block ends before it are all that
// count.  An image whose count stays below its blocks (a damaged or short scan) is then walked by jd_serial_index in this same launch,
// and its segs and status are word for word the serial index's.  One launch whatever the data, no spin-wait, nothing read back; all
// global writes are ordinary vector stores.
#include "common.h"
#include "jpeg_index.h"
#include "jpeg_sync.h"

namespace {
constexpr int JS_SPAN = JD_THREADS * JS_BYTES;              // bytes of the scan a workgroup resolves at a time
static_assert(JS_SPAN * 4 < (1 << 30), "a block takes at least two bits (one-symbol tables), so a span's block ends fit an int with room");
static_assert(JS_SPAN % 16 == 0 && JS_SLACK % 16 == 0 && JS_SPAN + JS_SLACK >= JD_WINDOW, "whole 16-byte loads; the serial walk borrows the window");

// stores the segment record at the start of every MCU row the walk passes
struct JsStoreRows {
    int* seg;
    int w0, len, before, p0, p1, p2, bpm, mw, total;        // before, p0..p2: blocks ended and DC sums ahead of this lane
    __device__ void operator()(const JeBits& b, const JsCount& c) const
    {
        const int mcu = (before + c.blocks) / bpm;
        if (mcu < total && mcu % mw == 0)
            jd_store_seg(seg + (size_t)(mcu / mw) * JD_SEG, w0 + b.pos, len, (int)b.acc, b.n, js_pred(p0 + c.d0), js_pred(p1 + c.d1), js_pred(p2 + c.d2), mcu);
    }
};

__global__ __launch_bounds__(JD_THREADS) void jpeg_sync_index_kernel(const JdImage* __restrict__ records, const uint8_t* __restrict__ scans,
                                                                     long long scans_bytes, int layout, int mw, int total, int S,
                                                                     int* __restrict__ segs, int* __restrict__ status, int* __restrict__ rounds)
{
    __shared__ JdTables tb;
    __shared__ __attribute__((aligned(16))) uint32_t win[(JS_SPAN + JS_SLACK) / 4];
    __shared__ int scanbuf[2][JD_THREADS];
    __shared__ int exit_p[JD_THREADS], exit_q[JD_THREADS];
    __shared__ JdWalk wk;
    const int tid = threadIdx.x, b = blockIdx.x;
    const JdImage* rec = records + b;
    int* seg = segs + (size_t)b * S * JD_SEG;
    const int off = rec->scan_off, len = rec->scan_len;
    const bool tables_ok = jd_load_tables(rec, tb, tid);
    if (!tables_ok || !jd_record_ok(off, len, scans_bytes)) {                       // nothing of this image is walked
        jd_refuse_image(seg, S, status + b, tables_ok, tid);
        if (rounds && tid == 0) rounds[b] = 0;
        return;
    }
    const uint8_t* scan = scans + off;
    const uint8_t* data = reinterpret_cast<const uint8_t*>(win);
    const int bpm = je_blocks_per_mcu(layout), need = total * bpm;

    JsState first{0, 0};                                    // the true state at the span's start, relative to it
    int before = 0, p0 = 0, p1 = 0, p2 = 0, turns = 0;      // blocks ended and DC sums ahead of the span; sync rounds so far
    for (int w0 = 0; w0 < len && first.p >= 0 && before < need; w0 += JS_SPAN) {
        const int wlen = min(JS_SPAN + JS_SLACK, len - w0), lanes = min(JD_THREADS, (len - w0 + JS_BYTES - 1) / JS_BYTES);
        jd_stage(scan, w0, wlen, reinterpret_cast<u32x4*>(win), tid);
        __syncthreads();
        const bool mine = tid < lanes;
        const int stop = min((tid + 1) * JS_BYTES, wlen);
        JsState entry{-1, 0}, exit{-1, 0};
        JsCount cnt{0, 0, 0, 0, 0};
        if (mine) {
            entry = tid == 0 ? first : js_assume(data, tid * JS_BYTES);
            exit = js_walk(data, wlen, stop, entry, tb.tab, tb.td, tb.ta, layout, cnt, JsNoVisit{});
            exit_p[tid] = exit.p; exit_q[tid] = exit.q;
        }
        __syncthreads();
        for (int r = 0; r < lanes; ++r) {                   // at the latest turn `lanes - 1` finds nothing changed
            JsState from = entry;
            if (mine && tid > 0) from = JsState{exit_p[tid - 1], exit_q[tid - 1]};
            const bool again = !js_same(from, entry);
            if (!__syncthreads_or(again ? 1 : 0)) break;    // (the barrier: every exit is read before one is written)
            if (again) {
                entry = from;
                exit = js_walk(data, wlen, stop, entry, tb.tab, tb.td, tb.ta, layout, cnt, JsNoVisit{});
                exit_p[tid] = exit.p; exit_q[tid] = exit.q;
            }
            __syncthreads();
            ++turns;
        }
        // a lane that still has an error marks where the serial walker stops: it counts up to that error, the lanes behind it not at
        // all, so the sum of the blocks is what the chain confirmed (tests/jpeg_sync_main.cpp adds up the same, lane after lane)
        int errs, sum, s0, s1, s2;
        const bool stands = dg_scan256(mine && cnt.err ? 1 : 0, scanbuf, tid, errs) == 0 && mine;
        const int b_before = before + dg_scan256(stands ? cnt.blocks : 0, scanbuf, tid, sum);
        const int d0 = p0 + dg_scan256(mine ? cnt.d0 : 0, scanbuf, tid, s0);
        const int d1 = p1 + dg_scan256(mine ? cnt.d1 : 0, scanbuf, tid, s1);
        const int d2 = p2 + dg_scan256(mine ? cnt.d2 : 0, scanbuf, tid, s2);
        if (stands && js_first_row_block(b_before, cnt.blocks, entry, cnt.err ? JsState{-1, 0} : exit, bpm * mw) >= 0) {
            JsCount again;
            js_walk(data, wlen, stop, entry, tb.tab, tb.td, tb.ta, layout, again, JsStoreRows{seg, w0, len, b_before, d0, d1, d2, bpm, mw, total});
        }
        first = JsState{exit_p[lanes - 1], exit_q[lanes - 1]};
        if (first.p >= 0) first.p -= JS_SPAN;
        if (errs) first.p = -1;                             // the chain ends in this span
        before += sum;
        p0 = (p0 + s0) & 0xFFFF; p1 = (p1 + s1) & 0xFFFF; p2 = (p2 + s2) & 0xFFFF;
        __syncthreads();                                    // the window and the exits are free again
    }
    if (rounds && tid == 0) rounds[b] = turns;
    if (before >= need) {                                   // every MCU was met before any error: every row has its record
        if (tid == 0) status[b] = JE_OK;
        return;
    }
    jd_serial_index(scan, len, layout, mw, total, S, seg, status + b, tb, win, wk, tid);
}
}  // namespace

// Launch 1 for images without a restart interval, as a parallel pass: segs int32 [B][S][8] and status int32 [B] as
// tup_jpeg_decode_index(restart_interval = 0) gives them, except that a good image's records may hold another reader state (byte, bits,
// their number) for the same bit of the scan; rounds int32 [B] (or null) <- the sync rounds each image took.
extern "C" int tup_jpeg_decode_index_sync(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout,
                                          int* segs, int* status, int* rounds, void* stream)
{
    JdGeometry g;
    if (!jd_geometry(H, W, layout, 0, g) || !records || !scans || !segs || !status || B < 1 || B > 65535 || scans_bytes < 0 ||
        scans_bytes > 0x7fff0000LL || (reinterpret_cast<uintptr_t>(scans) & 15) || (reinterpret_cast<uintptr_t>(records) & 3))
        return (int)hipErrorInvalidValue;
    jpeg_sync_index_kernel<<<dim3((unsigned)B), dim3(JD_THREADS), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        (const JdImage*)records, (const uint8_t*)scans, scans_bytes, layout, g.mw, g.total, g.S, segs, status, rounds);
    TUP_CHECK_LAUNCH();
    return 0;
}
