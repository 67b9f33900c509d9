"""TEST INFRASTRUCTURE ONLY -- the numpy statement of the baseline JPEG decoder (`ops.jpeg_decode`, csrc/jpeg_decode.hip and
csrc/jpeg_entropy.h).  `decode(data)` returns the pixels ``np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))`` gives
and a status (0, or one of the JE_* codes of jpeg_entropy.h for a scan that does not decode completely); tests/test_jpeg_decode_cpu.py
pins it to Pillow pixel for pixel.  Dequantisation tables, the inverse DCT and the colour conversion are those of
tests/_degrade_ref.py as they stand, zigzag order that of tests/_jpeg_ref.py.  What this file adds:

  parse      the marker segments: SOF0 only, DQT / DHT with any number of tables a segment, DRI, SOS; APPn and COM skipped.
  tables     Annex C: the codes of a DHT table in order of length, as a map from a code's bits to its symbol.
  walker     bit by bit: DC category and difference, AC run / size with ZRL (15, 0) and EOB (0, 0), 0xFF 0x00 read as 0xFF, the DC
             predictors reset at every restart marker.  A segment is the bytes between two restart markers (or the whole scan) and
             holds `restart interval` MCUs (the last one what is left).  It stops at a code with no entry, a coefficient past index
             63, a DC category above 11 or an AC size above 10, a marker inside the segment or the end of the data.
  back half  dequantise; jidctint's column and row pass, + 128, clip; 4:2:0: libjpeg's fancy h2v2 upsampling over the real chroma
             samples, ceil(H / 2) x ceil(W / 2): rows 3 : 1 with the row above (upper output row) or below (lower), then columns
             (3 s[i] + s[i - 1] + 8) >> 4 for the even and (3 s[i] + s[i + 1] + 7) >> 4 for the odd output, a sample at the edge being
             its own neighbour; YCbCr -> RGB, clip; crop to H x W.  One component: R = G = B = Y.
"""
import numpy as np

import _degrade_ref as D
import _jpeg_ref as REF

OK, BAD_CODE, BAD_INDEX, BAD_SIZE, MARKER, END, RESTARTS, BAD_TABLE = range(8)


def parse(data):
    """The twin of ops.jpeg_parse for the files the decoder takes; everything else is a ValueError."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    i, quant, huff, frame, interval = 2, {}, {}, None, 0
    jfif, adobe = False, None
    while True:
        if i + 4 > len(data) or data[i] != 0xFF or data[i + 1] == 0xD9:
            raise ValueError("the file ends before SOS")
        m, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if i + 2 + length > len(data):
            raise ValueError("the file ends before SOS")
        p = data[i + 4:i + 2 + length]
        i += 2 + length
        if 0xC1 <= m <= 0xCF and m != 0xC4:
            raise ValueError(f"SOF{m - 0xC0}")
        if m == 0xC0:
            if p[0] != 8 or p[5] not in (1, 3):
                raise ValueError("precision or component count")
            frame = (int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big"), [tuple(p[6 + 3 * c:9 + 3 * c]) for c in range(p[5])])
        elif m == 0xDB:
            for k in range(0, len(p), 65):
                if p[k] >> 4:
                    raise ValueError("16-bit quantisation table")
                t = np.zeros(64, dtype=np.int64)
                t[REF.ZIGZAG] = list(p[k + 1:k + 65])
                quant[p[k] & 15] = tuple(int(v) for v in t)
        elif m == 0xC4:
            k = 0
            while k < len(p):
                counts = tuple(p[k + 1:k + 17])
                if huffman_map((counts, ())) is None:
                    raise ValueError("not a valid prefix code")
                huff[(p[k] >> 4, p[k] & 15)] = (counts, tuple(p[k + 17:k + 17 + sum(counts)]))
                k += 17 + sum(counts)
        elif m == 0xDD:
            interval = int.from_bytes(p, "big")
        elif m == 0xE0 and p[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and p[:5] == b"Adobe":
            adobe = p[11]
        elif m == 0xDA:
            break
    H, W, comps = frame
    ns = p[0]
    if ns != len(comps) or tuple(p[1 + 2 * ns:]) != (0, 63, 0):
        raise ValueError("more than one scan, or a scan that is not 0 .. 63")
    samp = tuple(c[1] for c in comps)
    if len(comps) == 1:
        sub = "grey"
    elif samp in ((0x11, 0x11, 0x11), (0x22, 0x11, 0x11)) and adobe in (None, 1) and (jfif or adobe or tuple(c[0] for c in comps) != (0x52, 0x47, 0x42)):
        sub = "4:4:4" if samp[0] == 0x11 else "4:2:0"
    else:
        raise ValueError("sampling or colour space")
    end = data.rfind(b"\xff\xd9", i)
    return {"H": H, "W": W, "components": len(comps), "subsampling": sub, "quant_tables": quant, "huffman_tables": huff,
            "component_ids": tuple(c[0] for c in comps), "quant_selectors": tuple(c[2] for c in comps),
            "dc_selectors": tuple(p[2 + 2 * c] >> 4 for c in range(ns)), "ac_selectors": tuple(p[2 + 2 * c] & 15 for c in range(ns)),
            "restart_interval": interval, "scan": (i, end if end >= 0 else len(data))}


def huffman_map(spec):
    """Annex C: {the code as a string of bits: symbol}, or None where the counts are no prefix code."""
    counts, symbols = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        if code + counts[length - 1] > (1 << length):
            return None
        for _ in range(counts[length - 1]):
            if k < len(symbols):
                out[format(code, f"0{length}b")] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Stop(Exception):
    pass


class _Bits:
    """The bits of one segment, 0xFF 0x00 read as 0xFF; a marker or the end of the bytes ends them, and says which."""

    def __init__(self, seg, stats):
        out, i, self.hit = bytearray(), 0, END
        while i < len(seg):
            if seg[i] == 0xFF:
                if i + 1 >= len(seg):
                    break
                if seg[i + 1] != 0:
                    self.hit = MARKER
                    break
                stats["stuffed"] = stats.get("stuffed", 0) + 1
                out.append(0xFF)
                i += 2
                continue
            out.append(seg[i])
            i += 1
        self.bits = "".join(format(v, "08b") for v in out)
        self.pos = 0

    def symbol(self, table):
        for length in range(1, 17):
            code = self.bits[self.pos:self.pos + length]
            if len(code) < length:
                # the reader shows the walker zeros where the bytes have run out: a code made of them reaches past the data
                code = code + "0" * (length - len(code))
                if code in table:
                    raise _Stop(self.hit)
                continue
            if code in table:
                self.pos += length
                return table[code]
        raise _Stop(BAD_CODE)

    def receive(self, s):
        if self.pos + s > len(self.bits):
            raise _Stop(self.hit)
        v = int(self.bits[self.pos:self.pos + s], 2)
        self.pos += s
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _block(bits, dc, ac, pred, stats):
    """One block -> (64 coefficients in natural order, its DC)."""
    out = np.zeros(64, dtype=np.int64)
    s = bits.symbol(dc)
    if s > 11:
        raise _Stop(BAD_SIZE)
    stats["dc_size"] = max(stats.get("dc_size", 0), s)
    if s:
        pred = (pred + bits.receive(s) + 32768) % 65536 - 32768
    out[0] = pred
    k, nonzero = 1, 0
    while k < 64:
        rs = bits.symbol(ac)
        r, size = rs >> 4, rs & 15
        if size == 0:
            if r != 15:
                stats["eob_after_run" if nonzero else "eob_first"] = stats.get("eob_after_run" if nonzero else "eob_first", 0) + 1
                break
            stats["zrl"] = stats.get("zrl", 0) + 1
            k += 16
            continue
        if size > 10:
            raise _Stop(BAD_SIZE)
        k += r
        if k > 63:
            raise _Stop(BAD_INDEX)
        out[REF.ZIGZAG[k]] = bits.receive(size)
        nonzero += 1
        k += 1
    stats["full_blocks"] = stats.get("full_blocks", 0) + (nonzero == 63)
    stats["blocks"] = stats.get("blocks", 0) + 1
    return out, pred


def geometry(info):
    sub = info["subsampling"]
    m = 16 if sub == "4:2:0" else 8
    comps = {"4:4:4": (0, 1, 2), "4:2:0": (0, 0, 0, 0, 1, 2), "grey": (0,)}[sub]
    return m, (info["H"] + m - 1) // m, (info["W"] + m - 1) // m, comps


def segments(scan, interval):
    """The scan cut at its restart markers (every FF D0 .. D7: byte stuffing leaves no other such pair)."""
    if not interval:
        return [scan]
    out, start, i = [], 0, 0
    while i + 1 < len(scan):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            out.append(scan[start:i])
            start = i = i + 2
        else:
            i += 1
    return out + [scan[start:]]


def walk(data, info=None, stats=None):
    """-> (blocks int [MCU rows][MCUs a row][blocks per MCU][64] in natural order, zeros where the walk did not come; status)."""
    info = info or parse(data)
    stats = {} if stats is None else stats
    _, mh, mw, comps = geometry(info)
    tables = {k: huffman_map(v) for k, v in info["huffman_tables"].items()}
    blocks = np.zeros((mh * mw, len(comps), 64), dtype=np.int64)
    if any(t is None for t in tables.values()):
        return blocks.reshape(mh, mw, len(comps), 64), BAD_TABLE
    interval = info["restart_interval"]
    segs = segments(data[info["scan"][0]:info["scan"][1]], interval)
    count = (mh * mw + interval - 1) // interval if interval else 1
    status = OK if len(segs) == count else RESTARTS
    for s, seg in enumerate(segs[:count]):
        bits, pred = _Bits(seg, stats), [0, 0, 0]
        first = s * interval
        try:
            for mcu in range(first, min(first + interval, mh * mw) if interval else mh * mw):
                for j, c in enumerate(comps):
                    blocks[mcu, j], pred[c] = _block(bits, tables[(0, info["dc_selectors"][c])], tables[(1, info["ac_selectors"][c])], pred[c], stats)
        except _Stop as e:
            status = status or e.args[0]
    return blocks.reshape(mh, mw, len(comps), 64), status


def checksum(blocks):
    """Of the coefficients in scan order, as tests/jpeg_entropy_main.cpp prints it."""
    h = 0
    for v in np.asarray(blocks).reshape(-1):
        h = (h * 1000003 + (int(v) & 0xFFFF)) & 0xFFFFFFFF
    return h


def _idct(q, t):
    c = q.reshape(q.shape[:-1] + (8, 8)) * np.asarray(t, dtype=np.int64).reshape(8, 8)
    w = D._idct_pass(c.swapaxes(-1, -2), True).swapaxes(-1, -2)
    return np.clip(D._idct_pass(w, False) + 128, 0, 255)


def _plane(b):
    r, c = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(r * 8, c * 8)


def fancy_upsample(p):
    """p int [h][w], the real chroma samples -> [2 h][2 w]."""
    h, w = p.shape
    out = np.zeros((2 * h, 2 * w), dtype=np.int64)
    for v, nb in ((0, np.vstack([p[:1], p[:-1]])), (1, np.vstack([p[1:], p[-1:]]))):
        s = 3 * p + nb
        before, after = np.hstack([s[:, :1], s[:, :-1]]), np.hstack([s[:, 1:], s[:, -1:]])
        out[v::2, 0::2] = (3 * s + before + 8) >> 4
        out[v::2, 1::2] = (3 * s + after + 7) >> 4
    return out


def pixels(blocks, info):
    """The back half: quantised coefficients -> uint8 [H][W][3]."""
    H, W, sub = info["H"], info["W"], info["subsampling"]
    qt = [info["quant_tables"][t] for t in info["quant_selectors"]]
    if sub == "grey":
        Y = _plane(_idct(blocks[:, :, 0], qt[0]))[:H, :W]
        return np.stack([Y, Y, Y], -1).astype(np.uint8)
    if sub == "4:4:4":
        Y, Cb, Cr = (_plane(_idct(blocks[:, :, i], qt[i]))[:H, :W] for i in range(3))
    else:
        mh, mw = blocks.shape[:2]
        yb = np.zeros((mh * 2, mw * 2, 64), dtype=np.int64)
        for j in range(4):
            yb[(j >> 1)::2, (j & 1)::2] = blocks[:, :, j]
        Y = _plane(_idct(yb, qt[0]))[:H, :W]
        ch, cw = (H + 1) // 2, (W + 1) // 2
        Cb = fancy_upsample(_plane(_idct(blocks[:, :, 4], qt[1]))[:ch, :cw])[:H, :W]
        Cr = fancy_upsample(_plane(_idct(blocks[:, :, 5], qt[2]))[:ch, :cw])[:H, :W]
    FIX = D.FIX
    cb, cr = Cb - 128, Cr - 128
    rgb = np.stack([Y + ((FIX(1.402) * cr + 32768) >> 16), Y + ((-FIX(.34414) * cb + 32768 - FIX(.71414) * cr) >> 16),
                    Y + ((FIX(1.772) * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def decode(data, stats=None):
    """file bytes -> (uint8 [H][W][3] RGB, status)."""
    info = parse(data)
    blocks, status = walk(data, info, stats)
    return pixels(blocks, info), status
