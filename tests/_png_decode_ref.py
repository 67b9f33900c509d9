"""The PNG decoder's definition in plain Python (ops.png_decode, csrc/png_decode.hip, csrc/png_inflate.h): inflate with the
kernels' status codes, unfilter, conversion to RGB.  It mirrors png_inflate.h rule for rule, so that a damaged stream ends with the
same status everywhere: 64 stream bits are read from any bit position with zeros past the end; a token is decoded from them first
and tested against the end of the stream after."""
import struct
import zlib

import numpy as np

OK, BAD_BLOCK_TYPE, BAD_STORED_LEN, BAD_CODE, NO_SYMBOL, BAD_DISTANCE, INPUT_EXHAUSTED, OUTPUT_LONG, OUTPUT_SHORT, BAD_FILTER, BAD_ADLER = range(11)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LIT, DIST, CL = 0, 1, 2
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class Failed(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def build(lens, kind):
    """Code lengths -> {(length, code read first bit first): symbol}, under RFC 1951's rules (zlib's): never over-subscribed; complete,
    but for a literal or distance code that is one code of one bit; the code-length code is complete and not empty."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left, coded = 1, sum(count[1:])
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            raise Failed(BAD_CODE)
    if left > 0 and coded > 0 and (kind == CL or not (coded == 1 and count[1] == 1)):
        raise Failed(BAD_CODE)
    if coded == 0 and kind == CL:
        raise Failed(BAD_CODE)
    table, code = {}, 0
    for l in range(1, 16):
        for s, m in enumerate(lens):
            if m == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def symbol(table, w):
    """(symbol or -1, bits of its code; 15 where the bits are no code)"""
    code = 0
    for l in range(1, 16):
        code = (code << 1) | ((w >> (l - 1)) & 1)
        if (l, code) in table:
            return table[(l, code)], l
    return -1, 15


class Reader:
    def __init__(self, data):
        self.data, self.nbits, self.pos = data, 8 * len(data), 0

    def peek(self, pos=None):
        p = self.pos if pos is None else pos
        return (int.from_bytes(self.data[p >> 3:(p >> 3) + 9], "little") >> (p & 7)) & (2 ** 64 - 1)

    def need(self, bits):
        if self.pos + bits > self.nbits:
            raise Failed(INPUT_EXHAUSTED)


def token(lit, dist, w, avail):
    """-> (err, kind, used, value, len, dist): kind 0 literal, 1 match, 2 end of block"""
    sym, used = symbol(lit, w)
    err = kind = value = length = distance = 0
    if sym < 0 or sym >= 286:
        err = NO_SYMBOL
    elif sym < 256:
        value = sym
    elif sym == 256:
        kind = 2
    else:
        kind = 1
        eb = LENGTH_EXTRA[sym - 257]
        length = LENGTH_BASE[sym - 257] + ((w >> used) & ((1 << eb) - 1))
        used += eb
        ds, l = symbol(dist, w >> used)
        used += l
        if ds < 0 or ds >= 30:
            err = NO_SYMBOL
        else:
            db = DIST_EXTRA[ds]
            distance = DIST_BASE[ds] + ((w >> used) & ((1 << db) - 1))
            used += db
    if used > avail:
        err = INPUT_EXHAUSTED
    return err, kind, used, value, length, distance


def dynamic_tables(r):
    r.need(14)
    w = r.peek()
    nlen, nd, ncl = 257 + (w & 31), 1 + ((w >> 5) & 31), 4 + ((w >> 10) & 15)
    r.pos += 14
    if nlen > 286 or nd > 30:
        raise Failed(BAD_CODE)
    r.need(3 * ncl)
    w = r.peek()
    cl = [0] * 19
    for k in range(ncl):
        cl[CL_ORDER[k]] = (w >> (3 * k)) & 7
    r.pos += 3 * ncl
    table = build(cl, CL)
    lens = []
    while len(lens) < nlen + nd:
        w = r.peek()
        sym, l = symbol(table, w)
        used = l + (0 if sym < 0 else {16: 2, 17: 3, 18: 7}.get(sym, 0))
        r.need(used)
        if sym < 0:
            raise Failed(NO_SYMBOL)
        n, v = 1, sym
        if sym == 16:
            if not lens:
                raise Failed(BAD_CODE)
            v, n = lens[-1], 3 + ((w >> l) & 3)
        elif sym == 17:
            v, n = 0, 3 + ((w >> l) & 7)
        elif sym == 18:
            v, n = 0, 11 + ((w >> l) & 127)
        if len(lens) + n > nlen + nd:
            raise Failed(BAD_CODE)
        lens += [v] * n
        r.pos += used
    if lens[256] == 0:
        raise Failed(BAD_CODE)
    return build(lens[:nlen], LIT), build(lens[nlen:], DIST)


FIXED = None


def fixed_tables():
    global FIXED
    if FIXED is None:
        FIXED = (build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, LIT), build([5] * 32, DIST))
    return FIXED


def inflate(stream, total):
    """A zlib stream (two header bytes, blocks, Adler-32) that must inflate to exactly `total` bytes -> (bytes so far, status)."""
    r = Reader(bytes(stream))
    r.pos = 16
    out = bytearray()
    try:
        while True:
            r.need(3)
            head = r.peek() & 7
            r.pos += 3
            if head >> 1 == 3:
                raise Failed(BAD_BLOCK_TYPE)
            if head >> 1 == 0:
                r.pos = (r.pos + 7) & ~7
                r.need(32)
                w = r.peek()
                n = w & 0xffff
                if n != (~(w >> 16) & 0xffff):
                    raise Failed(BAD_STORED_LEN)
                r.pos += 32
                r.need(8 * n)
                if n > total - len(out):
                    raise Failed(OUTPUT_LONG)
                out += r.data[r.pos >> 3:(r.pos >> 3) + n]
                r.pos += 8 * n
            else:
                lit, dist = fixed_tables() if head >> 1 == 1 else dynamic_tables(r)
                while True:
                    err, kind, used, value, length, distance = token(lit, dist, r.peek(), r.nbits - r.pos)
                    if err:
                        raise Failed(err)
                    r.pos += used
                    if kind == 2:
                        break
                    if kind == 0:
                        if len(out) >= total:
                            raise Failed(OUTPUT_LONG)
                        out.append(value)
                    else:
                        if distance > len(out):
                            raise Failed(BAD_DISTANCE)
                        if length > total - len(out):
                            raise Failed(OUTPUT_LONG)
                        piece = bytes(out[len(out) - distance:len(out) - distance + length])
                        out += (piece * (length // len(piece) + 1))[:length]
            if head & 1:
                break
        if len(out) != total:
            raise Failed(OUTPUT_SHORT)
        r.pos = (r.pos + 7) & ~7
        r.need(32)
        want = struct.unpack(">I", r.data[r.pos >> 3:(r.pos >> 3) + 4])[0]
        if zlib.adler32(bytes(out)) != want:
            raise Failed(BAD_ADLER)
    except Failed as e:
        return bytes(out), e.status
    return bytes(out), OK


def unfilter(raw, H, W, bpp):
    """The filtered stream -> (uint8 [H][W * bpp], whether a filter byte was above 4: such a row is read as filter 0).  Row 0 lies
    under a row of zeros."""
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * bpp)
    out = np.zeros((H, W * bpp), np.uint8)
    bad = False
    prev = np.zeros(W * bpp, np.int32)
    for y in range(H):
        ft, x = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft > 4:
            bad, ft = True, 0
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        elif ft == 1:
            cur = (np.cumsum(x.reshape(W, bpp), axis=0) & 255).reshape(-1)
        else:
            cur = np.zeros(W * bpp, np.int32)
            xs, ps, cs = x.tolist(), prev.tolist(), [0] * (W * bpp)
            for i in range(W * bpp):
                a = cs[i - bpp] if i >= bpp else 0
                b = ps[i]
                c = ps[i - bpp] if i >= bpp else 0
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cs[i] = (xs[i] + pred) & 255
            cur = np.asarray(cs, np.int32)
        out[y] = cur
        prev = cur
    return out, bad


def to_rgb(samples, H, W, color_type, palette):
    """uint8 [H][W * channels] -> uint8 [H][W][3]: grey R = G = B, alpha dropped, palette looked up (an index past PLTE is black)."""
    s = samples.reshape(H, W, CHANNELS[color_type])
    if color_type in (2, 6):
        return np.ascontiguousarray(s[:, :, :3])
    if color_type == 3:
        pal = np.zeros((256, 3), np.uint8)
        p = np.frombuffer(bytes(palette), np.uint8).reshape(-1, 3)
        pal[:len(p)] = p
        return pal[s[:, :, 0]]
    return np.repeat(s[:, :, :1], 3, axis=2)


def chunks(data):
    """[(type, payload)] of a file whose framing is sound"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, found = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        found.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
    return found


def split(data):
    """-> (H, W, colour type, PLTE payload, the zlib stream)"""
    cs = chunks(data)
    W, H, depth, ct, _, _, lace = struct.unpack(">IIBBBBB", cs[0][1])
    assert depth == 8 and lace == 0
    return H, W, ct, b"".join(p for k, p in cs if k == b"PLTE"), b"".join(p for k, p in cs if k == b"IDAT")


def decode(data):
    """A file -> (RGB uint8 [H][W][3] or None where the stream did not inflate, status)."""
    H, W, ct, palette, stream = split(data)
    bpp = CHANNELS[ct]
    raw, status = inflate(stream, H * (1 + bpp * W))
    if status not in (OK, BAD_ADLER) or len(raw) != H * (1 + bpp * W):
        return None, status
    samples, bad = unfilter(raw, H, W, bpp)
    return to_rgb(samples, H, W, ct, palette), BAD_FILTER if bad else status
