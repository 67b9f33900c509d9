// What 4:2:0 adds to a JPEG round trip, per sample, as libjpeg computes it: the encoder's h2v2 downsample with its padding rules, and
// the decoder's "fancy" (triangle) upsample with its index clamping and the plain replication it falls back to on narrow images.
// One text for the kernel of degrade420.hip and for the host (tests/degrade420_main.cpp runs whole images through it under the address
// and undefined-behaviour sanitizers); tests/_degrade420_ref.py states it in numpy and is pinned to Pillow.
//
// Every index these functions return is inside the plane it addresses: pixel rows in [0, H), pixel columns in [0, W), chroma rows in
// [0, ceil(H/2)), chroma columns in [0, ceil(W/2)), for any cy, cx >= 0 and any pixel (y, x) of the image.
#pragma once

#ifndef TUP_HOST_DEVICE
#if defined(__HIPCC__)
#define TUP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define TUP_HOST_DEVICE inline
#endif
#endif

// ---- the front half: four pixels -> one chroma sample ----
struct J420Src {
    int y0, y1, x0, x1;      // the two pixel rows and the two pixel columns the sample averages
};
// Sample (cy, cx) of the downsampled plane, whose size is a multiple of 8 either way.  Columns are padded in the pixel domain: the
// image's last column is replicated up to the MCU width.  Rows are padded in the pixel domain only from H to H + (H & 1); below
// that the downsampled plane replicates its own last row.  The asymmetry is libjpeg's and shows in the output.
TUP_HOST_DEVICE J420Src j420_down_src(int cy, int cx, int H, int W)
{
    const int real = (H + 1) >> 1, ry = cy < real ? cy : real - 1;
    J420Src s;
    s.y0 = 2 * ry;
    s.y1 = 2 * ry + 1 < H ? 2 * ry + 1 : H - 1;
    s.x0 = 2 * cx < W ? 2 * cx : W - 1;
    s.x1 = 2 * cx + 1 < W ? 2 * cx + 1 : W - 1;
    return s;
}
// the rounding bias alternates 1, 2 with the sample's absolute column, so that the halves do not all round one way
TUP_HOST_DEVICE int j420_down(int p00, int p01, int p10, int p11, int cx) { return (p00 + p01 + p10 + p11 + 1 + (cx & 1)) >> 2; }

// ---- the back half: chroma samples -> one pixel's chroma ----
// libjpeg uses the triangle filter only on components more than 2 samples wide; below that every sample is replicated 2 x 2
TUP_HOST_DEVICE bool j420_narrow(int W) { return ((W + 1) >> 1) <= 2; }

struct J420Taps {
    int cy, ny, cx, nx;      // the pixel's own chroma row and column, and the nearer neighbour row and column, clamped to the real samples
};
TUP_HOST_DEVICE J420Taps j420_up_src(int y, int x, int H, int W)
{
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    J420Taps t;
    t.cy = y >> 1;
    t.cx = x >> 1;
    t.ny = (y & 1) ? (t.cy + 1 < ch ? t.cy + 1 : ch - 1) : (t.cy > 0 ? t.cy - 1 : 0);
    t.nx = (x & 1) ? (t.cx + 1 < cw ? t.cx + 1 : cw - 1) : (t.cx > 0 ? t.cx - 1 : 0);
    return t;
}
// rows 3 : 1 with the nearer row, then columns 3 : 1 with the nearer column; p_<row><col>, o = the pixel's own, n = the neighbour's
TUP_HOST_DEVICE int j420_up(int p_oo, int p_no, int p_on, int p_nn, int x)
{
    const int own = 3 * p_oo + p_no, nb = 3 * p_on + p_nn;
    return (3 * own + nb + ((x & 1) ? 7 : 8)) >> 4;
}
