"""Tap tables of the antialiased bilinear resize (torchvision.transforms.Resize on tensors).

Product-side builder for tup_resize_aa_fwd.  Follows aten's float32 evaluation
(_compute_indices_weights_aa in UpSampleKernel.cpp, PyTorch being a third-party dependency of
the reference: requirements.txt:42) so results agree with the reference's CPU path to rounding.
Vectorised numpy, float32 throughout.
"""
from __future__ import annotations

import functools
import math

import numpy as np


@functools.lru_cache(maxsize=64)
def aa_taps(in_size: int, out_size: int):
    f = np.float32
    scale = f(in_size) / f(out_size)
    support = scale if scale >= 1.0 else f(1.0)
    invscale = f(1.0) / scale if scale >= 1.0 else f(1.0)
    kmax = int(math.ceil(float(support))) * 2 + 1
    i = np.arange(out_size, dtype=np.float32)
    center = (scale * (i + f(0.5))).astype(np.float32)
    lo = np.maximum(0, (center - support + f(0.5)).astype(np.float32).astype(np.int64))
    hi = np.minimum(in_size, (center + support + f(0.5)).astype(np.float32).astype(np.int64))
    n = (hi - lo).astype(np.int32)
    j = np.arange(kmax, dtype=np.int64)[None, :]
    arg = ((j + lo[:, None]).astype(np.float32) - center[:, None] + f(0.5)).astype(np.float32) * invscale
    w = np.maximum(f(0.0), f(1.0) - np.abs(arg)).astype(np.float32)
    w = np.where(j < n[:, None], w, f(0.0)).astype(np.float32)
    tot = np.zeros(out_size, np.float32)
    for k in range(kmax):           # sequential float32 accumulation, as aten does
        tot = (tot + w[:, k]).astype(np.float32)
    w = np.where(tot[:, None] != 0, w / np.where(tot == 0, f(1.0), tot)[:, None], w).astype(np.float32)
    return lo.astype(np.int32), n, np.ascontiguousarray(w), kmax


@functools.lru_cache(maxsize=64)
def aa_inverse_ranges(in_size: int, out_size: int):
    """For every input index the contiguous range [o0, o0+on) of output indices whose taps cover it
    (the transpose of the forward table; used by the resize backward)."""
    lo, n, _, _ = aa_taps(in_size, out_size)
    o0 = np.full(in_size, out_size, np.int32)
    o1 = np.zeros(in_size, np.int32)
    for o in range(out_size):
        a, b = int(lo[o]), int(lo[o] + n[o])
        o0[a:b] = np.minimum(o0[a:b], o)
        o1[a:b] = np.maximum(o1[a:b], o + 1)
    on = np.maximum(o1 - o0, 0).astype(np.int32)
    o0 = np.where(on > 0, o0, 0).astype(np.int32)
    # contiguity check: every output in [o0, o0+on) must really cover the input index
    for i in range(in_size):
        for o in range(int(o0[i]), int(o0[i] + on[i])):
            assert lo[o] <= i < lo[o] + n[o]
    return o0, on


@functools.lru_cache(maxsize=64)
def taps_or_identity(in_size: int, out_size: int):
    """aa_taps, or exact identity tables when the sizes match (transforms.Resize returns its input then)."""
    if in_size == out_size:
        return (np.arange(out_size, dtype=np.int32), np.ones(out_size, np.int32), np.ones((out_size, 1), np.float32), 1)
    return aa_taps(in_size, out_size)


@functools.lru_cache(maxsize=64)
def tile_extent(in_size: int, out_size: int, tile: int) -> int:
    """Largest input window any `tile`-wide run of outputs touches (sizes the fused tail kernel's LDS tiles)."""
    lo, n, _, _ = taps_or_identity(in_size, out_size)
    best = 1
    for o0 in range(0, out_size, tile):
        o1 = min(o0 + tile, out_size) - 1
        best = max(best, int(lo[o1] + n[o1] - lo[o0]))
    return best


@functools.lru_cache(maxsize=64)
def bicubic_taps(in_size: int, out_size: int):
    """F.interpolate(mode='bicubic', align_corners=False) (aten upsample_bicubic2d, A = -0.75): per output index
    four clamped source indices and float32 weights.  Third-party PyTorch semantics (reference
    models/ResidualTransformer/model.py:125,160 call it); vectorised numpy."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    o = np.arange(out_size, dtype=np.float32)
    src = (scale * (o + f(0.5)) - f(0.5)).astype(np.float32)
    fl = np.floor(src)
    t = (src - fl).astype(np.float32)
    A = f(-0.75)
    c1 = lambda x: (((A + f(2)) * x - (A + f(3))) * x * x + f(1)).astype(np.float32)
    c2 = lambda x: (((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A).astype(np.float32)
    w = np.stack([c2(t + f(1)), c1(t), c1(f(1) - t), c2(f(2) - t)], axis=1).astype(np.float32)
    idx = np.clip(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, in_size - 1).astype(np.int32)
    return np.ascontiguousarray(idx), np.ascontiguousarray(w)


def transpose_taps(idx: np.ndarray, w: np.ndarray, in_size: int):
    """Per-output tap lists (idx, w: [out][K]) -> per-source CSR lists for the gather-form backward:
    start int32 [in+1], out_index int32 [nnz], weight float32 [nnz] (taps clamped onto the same source stay separate
    entries, so the backward adds exactly the terms the forward used)."""
    out_size, K = idx.shape
    flat_src = idx.reshape(-1).astype(np.int64)
    flat_out = np.repeat(np.arange(out_size, dtype=np.int64), K)
    order = np.argsort(flat_src, kind="stable")
    counts = np.bincount(flat_src, minlength=in_size)
    start = np.zeros(in_size + 1, dtype=np.int32)
    start[1:] = np.cumsum(counts)
    return start, np.ascontiguousarray(flat_out[order].astype(np.int32)), np.ascontiguousarray(w.reshape(-1)[order].astype(np.float32))


PIL_PRECISION_BITS = 32 - 8 - 2


def _pil_triangle(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _pil_cubic(x: float) -> float:
    """Pillow's bicubic_filter: the Keys kernel with a = -0.5."""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _pil_coeffs(in_size: int, out_size: int, kernel, kernel_support: float):
    """libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc for one axis and one filter."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = kernel_support * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    lo = np.zeros(out_size, np.int32)
    n = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    inv = 1.0 / fscale
    for i in range(out_size):
        center = (i + 0.5) * scale
        a = max(int(center - support + 0.5), 0)
        b = min(int(center + support + 0.5), in_size)
        ww = 0.0
        for x in range(b - a):
            w = kernel((x + a - center + 0.5) * inv)
            kk[i, x] = w
            ww += w
        if ww != 0.0:
            kk[i, :b - a] /= ww
        lo[i], n[i] = a, b - a
    ki = np.where(kk < 0, np.trunc(-0.5 + kk * (1 << PIL_PRECISION_BITS)), np.trunc(0.5 + kk * (1 << PIL_PRECISION_BITS)))
    return lo, n, np.ascontiguousarray(ki.astype(np.int32)), ksize


def pil_bilinear_coeffs(in_size: int, out_size: int):
    """Pillow's coefficient tables for an 8-bit BILINEAR resample of one axis (libImaging/Resample.c precompute_coeffs +
    normalize_coeffs_8bpc; the arithmetic behind transforms.Resize on a PIL image, reference data_handling/data_class.py:61-71):
    (min int32 [out], size int32 [out], k int32 [out][ksize], ksize).  Weights are computed and normalised in double and rounded
    half away from zero to 22 fractional bits, exactly as Pillow does."""
    return _pil_coeffs(in_size, out_size, _pil_triangle, 1.0)


def pil_bicubic_coeffs(in_size: int, out_size: int):
    """The same tables for Pillow's BICUBIC resample (a = -0.5, support 2; the reference's baseline image, inference.py:83): same
    normalisation and rounding, negative lobes included, so the row / column kernels take them as they are."""
    return _pil_coeffs(in_size, out_size, _pil_cubic, 2.0)


def tail_fused_tables(in_h: int, in_w: int, out_h: int, out_w: int, tile_h: int, tile_w: int):
    """Row and column tables of the tiled fused tail (csrc/tail_fused.hip) and the input extent of its output tiles."""
    return taps_or_identity(in_h, out_h) + taps_or_identity(in_w, out_w) + (tile_extent(in_h, out_h, tile_h), tile_extent(in_w, out_w, tile_w))


def tail_stream_plan(B: int, H: int, W: int, Ho: int, Wo: int, workgroups: int):
    """Decomposition of the fused streaming tail + Resize (csrc/tail_stream.hip, RESIZE = true) of B LR maps H x W to Ho x Wo:
    (ylo, yn, yw, ky, xlo, xn, xw, kx, oxb, oyb, strip stride, band height, band extension) with oxb / oyb the output columns /
    rows each strip / band owns.  `workgroups` fills the chip once at the kernel's occupancy.  None when a tap table has more
    than 4 taps or an owned output reads beyond what its strip / band computes (then the Resize runs as its own kernel)."""
    ylo, yn, yw, ky = aa_taps(2 * H, Ho)
    xlo, xn, xw, kx = aa_taps(2 * W, Wo)
    if int(yn.max()) > 4 or int(xn.max()) > 4:
        return None
    sc = 60 - (int(xn.max()) - 1 + 1) // 2
    ext = (int(yn.max()) - 1 + 1) // 2
    nstrip = (W + sc - 1) // sc
    nb = max(1, workgroups // max(1, B * nstrip))
    bh = max(12, ((H + nb - 1) // nb + 2) // 3 * 3)
    nband = (H + bh - 1) // bh
    oxb = np.searchsorted(xlo, 2 * sc * np.arange(nstrip + 1), side="left").astype(np.int32)
    oyb = np.searchsorted(ylo, 2 * bh * np.arange(nband + 1), side="left").astype(np.int32)
    oxb[-1], oyb[-1] = Wo, Ho
    for s in range(nstrip):           # every owned column's taps inside the strip's 120 valid HR columns, <= 128 gathered
        a, b = int(oxb[s]), int(oxb[s + 1])
        if b > a and ((xlo[a:b] + xn[a:b]).max() > 2 * s * sc + 120 or b - a > 128):
            return None
    for k in range(nband):            # every owned row's taps inside the rows the band computes
        a, b = int(oyb[k]), int(oyb[k + 1])
        if b > a and (ylo[a:b] + yn[a:b]).max() > 2 * min(H, (k + 1) * bh + ext):
            return None
    return ylo, yn, yw, ky, xlo, xn, xw, kx, oxb, oyb, sc, bh, ext


def bicubic_taps_transposed(in_size: int, out_size: int):
    """transpose_taps of bicubic_taps: the per-source lists of the gather-form bicubic backward."""
    idx, w = bicubic_taps(in_size, out_size)
    return transpose_taps(idx, w, in_size)


BICUBIC_BAND_ROWS = 16


def bicubic_bands(in_size: int, out_size: int):
    """Band tables of the row pass of the banded bicubic backward: for source rows 16b .. 16b+15 the contiguous range of output
    rows that touch them (first int32 [bands], count int32 [bands]) and the dense weights fp32 [bands][rows][16] (transpose of the
    forward tap matrix), rows = the largest count."""
    yb = BICUBIC_BAND_ROWS
    idx, w = bicubic_taps(in_size, out_size)             # [out][4]
    nb = (in_size + yb - 1) // yb
    lo = np.full(in_size, out_size, dtype=np.int64)
    hi = np.full(in_size, -1, dtype=np.int64)
    rows = np.arange(out_size)
    for k in range(4):
        np.minimum.at(lo, idx[:, k], rows)
        np.maximum.at(hi, idx[:, k], rows)
    r0 = np.array([lo[b * yb:(b + 1) * yb].min() for b in range(nb)], dtype=np.int64)
    r1 = np.array([hi[b * yb:(b + 1) * yb].max() for b in range(nb)], dtype=np.int64)
    n = (r1 - r0 + 1).clip(min=1)
    r0 = np.minimum(r0, out_size - 1)
    nr_max = int(n.max())
    bw = np.zeros((nb, nr_max, yb), dtype=np.float32)
    for k in range(4):
        y = idx[:, k]
        b = y // yb
        np.add.at(bw, (b, rows - r0[b], y - b * yb), w[:, k].astype(np.float32))
    return r0.astype(np.int32), n.astype(np.int32), bw, nr_max


def bicubic_cols(in_size: int, out_size: int):
    """Dense column tables of the banded bicubic backward: (xoT int32 [kmax][in], xwT fp32 [kmax][in], kmax, and per 256-column
    block the first output column int32 [blocks] and the count int32 [blocks] it reads) from the transposed tap lists; None when
    a block's stretch exceeds the kernel's LDS tile of 4096 columns (very large ratios)."""
    xs, xo, xw = bicubic_taps_transposed(in_size, out_size)
    cnt = np.diff(xs)
    kmax = int(cnt.max())
    xoT = np.zeros((kmax, in_size), dtype=np.int32)
    xwT = np.zeros((kmax, in_size), dtype=np.float32)
    for x in range(in_size):
        n = cnt[x]
        xoT[:n, x] = xo[xs[x]:xs[x] + n]
        xwT[:n, x] = xw[xs[x]:xs[x] + n]
        xoT[n:, x] = xo[xs[x]]                                  # padding: in-range index, weight 0
    nblk = (in_size + 255) // 256
    c0 = np.array([xoT[:, j * 256:(j + 1) * 256].min() for j in range(nblk)], dtype=np.int32)
    c1 = np.array([xoT[:, j * 256:(j + 1) * 256].max() for j in range(nblk)], dtype=np.int32)
    nn = (c1 - c0 + 1).astype(np.int32)
    return None if int(nn.max()) > 4096 else (xoT, xwT, kmax, c0, nn)
