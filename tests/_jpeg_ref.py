"""TEST INFRASTRUCTURE ONLY -- the numpy statement of the baseline JPEG encoder (`ops.jpeg_encode`, csrc/jpeg_encode.hip).
`encode(frame, quality, subsampling, restart_rows)` returns the bytes of the file that
``Image.fromarray(frame).save(buf, "JPEG", quality=q, subsampling=s, restart_marker_rows=R)`` writes; tests/test_jpeg_cpu.py pins it
to Pillow byte for byte.  Colour conversion, forward DCT, quantiser tables and quantiser are those of tests/_degrade_ref.py as they
stand.  What this file adds:

  geometry   an MCU is 8 x 8 (4:4:4: Y, Cb, Cr) or 16 x 16 (4:2:0: Y x 4 in raster order, Cb, Cr).  Luma is replicated from its last
             column / row out to whole 8 x 8 blocks.  The luma blocks of an edge MCU beyond those (a 4:2:0 image whose width or height
             in blocks is odd) are not made from pixels: libjpeg codes them as DC = the DC of the block before them in the MCU, AC = 0.
  chroma     4:2:0: Cb and Cr at full resolution, columns replicated out to whole MCUs, then (a + b + c + d + bias) >> 2 with the bias
             1, 2, 1, 2 ... along a row.  Rows: an odd last row is paired with itself; below that, the LAST DOWNSAMPLED ROW is
             replicated (libjpeg pads after downsampling there), which differs from downsampling replicated rows when H is even.
  entropy    zigzag order, DC differences per component in scan order reset at every restart, AC run / size with ZRL and EOB, the
             standard tables K.3 - K.6, bits MSB first, 1-padding before every RSTm (m = 0 .. 7 cycling) and before EOI, 0xFF -> 0xFF 0x00.
  file       SOI, APP0 (JFIF 1.01, density 1:1, no unit), DQT luma, DQT chroma, SOF0, DHT x 4 (DC0, AC0, DC1, AC1), DRI, SOS, scan, EOI.
"""
import numpy as np

import _degrade_ref as D

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.3 - K.6: the number of codes of each length 1 .. 16, then the symbols in code order
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
            0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
            0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
            0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
            0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
            0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
            0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
              0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
              0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
              0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
              0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
              0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
              0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def huffman_codes(spec):
    """Annex C: symbol -> (code, length) from the (counts, symbols) form of a table."""
    counts, symbols = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
AC_CODES = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]


def subsampling_code(s):
    if s in (0, "4:4:4"):
        return 0
    if s in (2, "4:2:0"):
        return 2
    raise ValueError(f"subsampling {s!r}")


def _fdct_quant(planes, table):
    """planes int [n][8k][8l] (0 .. 255) -> quantised coefficients int [n][k][l][64] in natural order."""
    n, h, w = planes.shape
    blk = (planes - 128).reshape(n, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4)
    c = D._fdct_pass(blk, True)
    c = D._fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
    q = np.sign(c) * ((np.abs(c) + (8 * table >> 1)) // (8 * table))
    return q.reshape(n, h // 8, w // 8, 64)


def coefficients(frame, quality, sub):
    """frame uint8 [H][W][3] -> (blocks int [MCU rows][MCUs per row][blocks per MCU][64] in natural order, component index of each
    block of an MCU).  The luma blocks libjpeg does not make from pixels are already in their coded form."""
    u = np.asarray(frame).astype(np.int64)
    H, W, _ = u.shape
    R, G, B = u[..., 0], u[..., 1], u[..., 2]
    FIX = D.FIX
    Y = (FIX(.299) * R + FIX(.587) * G + FIX(.114) * B + 32768) >> 16
    Cb = (-FIX(.16874) * R - FIX(.33126) * G + FIX(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (FIX(.5) * R - FIX(.41869) * G - FIX(.08131) * B + (128 << 16) + 32767) >> 16
    tl, tc = D.quant_table(D.LUMA, quality), D.quant_table(D.CHROMA, quality)
    m = 16 if sub == 2 else 8
    mh, mw = (H + m - 1) // m, (W + m - 1) // m
    pad = lambda p, h, w: np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")
    qy = _fdct_quant(pad(Y, mh * m, mw * m)[None], tl)[0]                          # [mh * m / 8][mw * m / 8][64]
    if sub == 0:
        qc = _fdct_quant(np.stack([pad(Cb, mh * 8, mw * 8), pad(Cr, mh * 8, mw * 8)]), tc)
        return np.stack([qy, qc[0], qc[1]], axis=2), (0, 1, 2)
    hb, wb = (H + 7) // 8, (W + 7) // 8                                             # luma blocks that exist
    ch = []
    for p in (Cb, Cr):
        p = pad(p, H + (H & 1), mw * 16)
        bias = 1 + (np.arange(mw * 8) & 1)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        ch.append(pad(d, mh * 8, mw * 8))
    qc = _fdct_quant(np.stack(ch), tc)
    out = np.zeros((mh, mw, 6, 64), dtype=np.int64)
    for my in range(mh):
        for mx in range(mw):
            for j in range(4):
                by, bx = 2 * my + (j >> 1), 2 * mx + (j & 1)
                if by < hb and bx < wb:
                    out[my, mx, j] = qy[by, bx]
                else:
                    out[my, mx, j, 0] = out[my, mx, j - 1, 0]                       # j >= 1 here: block 0 of an MCU always exists
            out[my, mx, 4], out[my, mx, 5] = qc[0, my, mx], qc[1, my, mx]
    return out, (0, 0, 0, 0, 1, 2)


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.stuffed = 0

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(int(v))).bit_length()


def encode_block(bw, blk, pred, dc, ac, stats=None):
    """One block of 64 natural-order coefficients; returns its DC value (the next predictor of its component)."""
    diff = int(blk[0]) - pred
    s = _size(diff)
    bw.put(*dc[s])
    if s:
        bw.put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
    if stats is not None:
        stats["dc_size"] = max(stats.get("dc_size", 0), s)
    zz = blk[ZIGZAG]
    run = 0
    nonzero = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        nonzero += 1
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
            if stats is not None:
                stats["zrl"] = stats.get("zrl", 0) + 1
        s = _size(v)
        bw.put(*ac[(run << 4) | s])
        bw.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        run = 0
    if run:
        bw.put(*ac[0])
        if stats is not None and nonzero:
            stats["eob_after_run"] = stats.get("eob_after_run", 0) + 1
    if stats is not None:
        if nonzero == 63:
            stats["full_blocks"] = stats.get("full_blocks", 0) + 1
        if nonzero == 0:
            stats["dc_only_blocks"] = stats.get("dc_only_blocks", 0) + 1
        stats["blocks"] = stats.get("blocks", 0) + 1
    return int(blk[0])


def scan(frame, quality, sub, restart_rows, stats=None):
    """The entropy-coded segment between SOS and EOI, restart markers included."""
    blocks, comps = coefficients(frame, quality, sub)
    mh, mw = blocks.shape[:2]
    interval = restart_rows * mw
    out = bytearray()
    bw = BitWriter()
    pred = [0, 0, 0]
    stuffed = 0
    for i in range(mh * mw):
        if i and i % interval == 0:
            bw.flush()
            out += bw.out + bytes([0xFF, 0xD0 + ((i // interval - 1) & 7)])
            stuffed += bw.stuffed
            bw = BitWriter()
            pred = [0, 0, 0]
        for j, c in enumerate(comps):
            pred[c] = encode_block(bw, blocks[i // mw, i % mw, j], pred[c], DC_CODES[c > 0], AC_CODES[c > 0], stats)
    bw.flush()
    if stats is not None:
        stats["stuffed"] = stuffed + bw.stuffed
    return bytes(out + bw.out)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, quality, sub, restart_rows):
    """Everything before the scan: SOI .. SOS, from the parameters alone."""
    m = 16 if sub == 2 else 8
    interval = restart_rows * ((W + m - 1) // m)
    assert 1 <= H <= 65535 and 1 <= W <= 65535 and 1 <= interval <= 65535
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, base in enumerate((D.LUMA, D.CHROMA)):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in D.quant_table(base, quality).reshape(64)[ZIGZAG]))
    samp = 0x22 if sub == 2 else 0x11
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, samp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([cls]) + bytes(spec[0]) + bytes(spec[1]))
    out += _segment(0xDD, interval.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(frame, quality=75, subsampling="4:2:0", restart_rows=1, stats=None):
    """frame uint8 [H][W][3] RGB -> the bytes of the JPEG file."""
    sub = subsampling_code(subsampling)
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and 1 <= quality <= 100 and restart_rows >= 1
    H, W, _ = frame.shape
    return header(H, W, quality, sub, restart_rows) + scan(frame, quality, sub, restart_rows, stats) + b"\xff\xd9"


def split(data):
    """(marker segments before and including SOS, scan without the EOI)."""
    i = 2
    while True:
        assert data[i] == 0xFF
        length = int.from_bytes(data[i + 2:i + 4], "big")
        done = data[i + 1] == 0xDA
        i += 2 + length
        if done:
            break
    assert data[-2:] == b"\xff\xd9"
    return data[:i], data[i:-2]
