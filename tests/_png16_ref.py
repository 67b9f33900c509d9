"""TEST INFRASTRUCTURE ONLY -- the 16-bit PNG file `ops.png_encode(.., bits=16)` writes (csrc/png16_encode.hip, csrc/png_kernels.h; DESIGN
7m), stated in numpy and plain Python.  It is tests/_png_ref.py's file with exactly these changes: IHDR bit depth 16 (colour type 2),
samples big-endian, bpp = 6, a row of 1 + 6 W filtered bytes.  Filters and the adaptive choice work on bytes, with the left neighbour
at x - 6.  Ranges, tokens, code lengths, block forms, IDAT framing, CRC and Adler are _png_ref's, used as they are.  The GPU's files
equal `encode` byte for byte; tests/test_png16_cpu.py checks these files with Pillow, zlib and an independent unfilter."""
import struct

import numpy as np

import _png_ref as P

FILTERS = P.FILTERS
BPP = 6


def quantise16(x):
    """q_16: float32 [3][H][W] (or [B][3][H][W]) -> uint16 [H][W][3] (or [B][H][W][3]).  Four separate fp32 steps: t = x * 65535;
    NaN -> 0; clamp to [0, 65535]; (int)(t + 0.5f)."""
    s = np.float32(65535.0)
    t = np.asarray(x, np.float32) * s
    t = np.where(np.isnan(t), np.float32(0.0), t)
    t = np.minimum(np.maximum(t, np.float32(0.0)), s)
    q = (t + np.float32(0.5)).astype(np.int32).astype(np.uint16)
    return np.ascontiguousarray(np.moveaxis(q, -3, -1))


def row_bytes(img):
    """uint16 [H][W][3] -> uint8 [H][6 W]: every sample high byte first"""
    img = np.asarray(img)
    assert img.dtype == np.uint16 and img.ndim == 3 and img.shape[2] == 3
    return np.ascontiguousarray(img.astype(">u2")).view(np.uint8).reshape(img.shape[0], 6 * img.shape[1])


def _candidates(cur, up):
    """the five filtered forms of one row of bytes, uint8 [5][6 W]"""
    cur = cur.astype(np.int32)
    up = up.astype(np.int32)
    a = np.concatenate([np.zeros(BPP, np.int32), cur[:-BPP]])
    c = np.concatenate([np.zeros(BPP, np.int32), up[:-BPP]])
    p = a + up - c
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    return np.stack([cur, cur - a, cur - up, cur - ((a + up) >> 1), cur - paeth]).astype(np.uint8)


def filter_types(img, filter="adaptive"):
    """uint8 [H]: the filter of every row"""
    rows = row_bytes(img)
    h = rows.shape[0]
    f = FILTERS[filter]
    if f < 5:
        return np.full(h, f, np.uint8)
    out = np.zeros(h, np.uint8)
    for y in range(h):
        cand = _candidates(rows[y], rows[y - 1] if y else np.zeros_like(rows[0]))
        out[y] = int(np.argmin(np.abs(cand.view(np.int8).astype(np.int64)).sum(1)))          # the first of equal sums
    return out


def filtered(img, filter="adaptive"):
    rows = row_bytes(img)
    h, n = rows.shape
    types = filter_types(img, filter)
    out = np.zeros((h, 1 + n), np.uint8)
    for y in range(h):
        out[y, 0] = types[y]
        out[y, 1:] = _candidates(rows[y], rows[y - 1] if y else np.zeros_like(rows[0]))[types[y]]
    return out.tobytes()


def blocks(h, w, block_bytes):
    return -(-(h * (1 + 6 * w)) // block_bytes)


def file_bound(h, w, block_bytes):
    """the length of the file whose blocks are all stored"""
    return 33 + h * (1 + 6 * w) + 2 + (5 + 12) * blocks(h, w, block_bytes) + 16 + 12


def encode(img, block_bytes=32768, filter="adaptive", stats=None):
    img = np.asarray(img)
    assert P.MIN_BLOCK <= block_bytes <= P.MAX_BLOCK
    h, w, _ = img.shape
    stream = filtered(img, filter)
    out = P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
    n = blocks(h, w, block_bytes)
    for i in range(n):
        body = P.deflate_block(stream[i * block_bytes:(i + 1) * block_bytes], i == n - 1, stats)
        out += P.chunk(b"IDAT", (b"\x78\x01" if i == 0 else b"") + body)
    return out + P.chunk(b"IDAT", struct.pack(">I", P.adler32(stream))) + P.chunk(b"IEND", b"")
