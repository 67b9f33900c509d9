"""TEST INFRASTRUCTURE ONLY -- the PNG file `ops.png_encode` writes (csrc/png_encode.hip, csrc/png_deflate.h), stated in numpy
and plain Python.  The GPU's files equal `encode` byte for byte; tests/test_png_cpu.py checks these files with Pillow and zlib.

The file: signature, IHDR (8-bit RGB, no interlace), one IDAT per deflate block, an IDAT of four bytes with the Adler-32, IEND.
The filtered stream, H * (1 + 3 W) bytes, is cut into ranges of `block_bytes` bytes that ignore row boundaries; a range is one deflate
block.  Rules fixed here, each stated once:

* tokens: a maximal run of r equal bytes inside a range is one literal, then with m = r - 1: m // 258 matches (length 258, distance 1),
  then, with t = m % 258, one match of length t when t >= 3, else t literals.  (So runs of up to three bytes are literals.)
* code lengths: symbols with a count, sorted by (count, symbol); Moffat-Katajainen's in-place minimum-redundancy lengths on that order;
  lengths above the limit (15; 7 for the code-length alphabet) are clamped and the Kraft sum is repaired by moving codes down from the
  limit; the longest lengths go to the first symbols of the order.  One symbol alone gets length 1.
* dynamic header: BFINAL, BTYPE = 2, HLIT = 1 + the last used literal/length symbol (>= 257), HDIST = 1 + the last used distance symbol
  (>= 1; distance 1 is symbol 0, so HDIST is always 1), HCLEN = 1 + the last position of the permuted order with a length (>= 4).
  The HLIT + HDIST lengths are one sequence; a run of c zeros is 18 (up to 138 at a time) while c >= 11, then 17 when c >= 3, then single
  zeros; a run of c equal lengths v is v, then 16 (up to 6 at a time) while c >= 3, then single v.
* the form of a block: bits_fixed = 3 + tokens + 7, bits_dynamic = 3 + 14 + 3 HCLEN + header tokens + tokens + end-of-block.  The
  Huffman form is the fixed one unless the dynamic one has fewer bits.  Its bytes are ceil((bits + 3) / 8) + 4 with the empty stored
  block that follows every block but the last, ceil(bits / 8) for the last.  The block is stored (5 + n bytes) unless the Huffman form
  has fewer bytes.
"""
import struct
import zlib

import numpy as np

FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
MIN_BLOCK, MAX_BLOCK = 256, 32768


# ---- filters ----
def _candidates(cur, up):
    """the five filtered forms of one row, uint8 [5][3 W]"""
    cur = cur.astype(np.int32)
    up = up.astype(np.int32)
    a = np.concatenate([np.zeros(3, np.int32), cur[:-3]])
    c = np.concatenate([np.zeros(3, np.int32), up[:-3]])
    p = a + up - c
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    return np.stack([cur, cur - a, cur - up, cur - ((a + up) >> 1), cur - paeth]).astype(np.uint8)


def filter_types(img, filter="adaptive"):
    """uint8 [H]: the filter of every row"""
    img = np.asarray(img)
    h, w, _ = img.shape
    f = FILTERS[filter]
    if f < 5:
        return np.full(h, f, np.uint8)
    rows = img.reshape(h, 3 * w)
    out = np.zeros(h, np.uint8)
    for y in range(h):
        cand = _candidates(rows[y], rows[y - 1] if y else np.zeros(3 * w, np.uint8))
        sums = np.abs(cand.view(np.int8).astype(np.int64)).sum(1)
        out[y] = int(np.argmin(sums))                                  # the first of equal sums
    return out


def filtered(img, filter="adaptive"):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w, _ = img.shape
    rows = img.reshape(h, 3 * w)
    types = filter_types(img, filter)
    out = np.zeros((h, 1 + 3 * w), np.uint8)
    for y in range(h):
        out[y, 0] = types[y]
        out[y, 1:] = _candidates(rows[y], rows[y - 1] if y else np.zeros(3 * w, np.uint8))[types[y]]
    return out.tobytes()


# ---- Huffman code lengths ----
def _minimum_redundancy(a):
    """Moffat & Katajainen, in place: counts in ascending order -> code lengths (longest first)"""
    n = len(a)
    if n == 1:
        a[0] = 0
        return
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avail, used, depth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avail > 0:
        while root >= 0 and a[root] == depth:
            used += 1
            root -= 1
        while avail > used:
            a[nxt] = depth
            nxt -= 1
            avail -= 1
        avail, used, depth = 2 * used, 0, depth + 1


def code_lengths(freq, limit):
    """lengths, one per symbol (0: unused)"""
    order = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    lens = [0] * len(freq)
    if not order:
        return lens
    if len(order) == 1:
        lens[order[0][1]] = 1
        return lens
    a = [f for f, _ in order]
    _minimum_redundancy(a)
    count = [0] * (limit + 1)
    for l in a:
        count[min(l, limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    i = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lens[order[i][1]] = l
            i += 1
    return lens


def canonical(lens):
    """by symbol: the code with its bits reversed, as deflate sends it"""
    next_code, code = {}, 0
    for l in range(1, 16):
        code = (code + sum(1 for v in lens if v == l - 1 and l > 1)) << 1
        next_code[l] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(next_code[l], f"0{l}b")[::-1], 2)
            next_code[l] += 1
    return out


def length_symbol(n):
    """match length 3..258 -> (symbol, extra bits, their value)"""
    if n == 258:
        return 285, 0, 0
    v = n - 3
    if v < 8:
        return 257 + v, 0, 0
    eb = v.bit_length() - 3
    return 261 + 4 * eb + ((v >> eb) & 3), eb, v & ((1 << eb) - 1)


def run_length_code(seq):
    """the code-length sequence -> [(symbol, extra bits, their value)]"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        c = j - i
        i = j
        if v == 0:
            while c >= 11:
                k = min(c, 138)
                out.append((18, 7, k - 11))
                c -= k
            if c >= 3:
                out.append((17, 3, c - 3))
                c = 0
        else:
            out.append((v, 0, 0))
            c -= 1
            while c >= 3:
                k = min(c, 6)
                out.append((16, 2, k - 3))
                c -= k
        out += [(v, 0, 0)] * c
    return out


# ---- one deflate block ----
def tokens(block):
    """[(byte, run length)] of the maximal runs, and the tokens: ('L', byte) / ('M', length)"""
    d = np.frombuffer(block, np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    ends = np.concatenate([starts[1:], [len(d)]])
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v, m = int(d[s]), e - s - 1
        out.append(("L", v))
        out += [("M", 258)] * (m // 258)
        t = m % 258
        out += [("M", t)] if t >= 3 else [("L", v)] * t
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, val, n):
        self.acc |= val << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def block_plan(block):
    """what decides a block's form: the tokens, both histograms, the dynamic code and the exact bit counts"""
    toks = tokens(block)
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for kind, v in toks:
        if kind == "L":
            lit[v] += 1
        else:
            lit[length_symbol(v)[0]] += 1
            dist[0] += 1
    ll, dl = code_lengths(lit, 15), code_lengths(dist, 15)
    hlit = max(s for s in range(286) if lit[s]) + 1
    hdist = max([s for s in range(30) if dist[s]] + [0]) + 1
    cl_tokens = run_length_code(ll[:hlit] + dl[:hdist])
    cl_freq = [0] * 19
    for s, _, _ in cl_tokens:
        cl_freq[s] += 1
    cl = code_lengths(cl_freq, 7)
    hclen = max(max(i for i in range(19) if cl[CL_ORDER[i]]) + 1, 4)
    extra = lambda s: (s - 261) // 4 if 265 <= s < 285 else 0           # extra bits of a length symbol
    body_fixed = sum(lit[s] * (FIXED_LENGTHS[s] + extra(s)) for s in range(286)) + 5 * dist[0]
    body_dyn = sum(lit[s] * (ll[s] + extra(s)) for s in range(286)) + dl[0] * dist[0]
    bits_fixed = 3 + body_fixed
    bits_dyn = 3 + 14 + 3 * hclen + sum(cl[s] + e for s, e, _ in cl_tokens) + body_dyn
    return dict(tokens=toks, ll=ll, dl=dl, cl=cl, hlit=hlit, hdist=hdist, hclen=hclen, cl_tokens=cl_tokens, bits_fixed=bits_fixed, bits_dyn=bits_dyn)


def deflate_block(block, last, stats=None):
    """the bytes of one range: a deflate block that starts and ends on a byte boundary"""
    n = len(block)
    p = block_plan(block)
    dynamic = p["bits_dyn"] < p["bits_fixed"]
    bits = p["bits_dyn"] if dynamic else p["bits_fixed"]
    nbytes = (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4
    form = "stored" if 5 + n <= nbytes else ("dynamic" if dynamic else "fixed")
    if stats is not None:
        stats.setdefault("forms", []).append(form)
        stats.setdefault("plans", []).append(p)
    if form == "stored":
        return bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(block)
    w = _Bits()
    w.put(1 if last else 0, 1)
    if dynamic:
        w.put(2, 2)
        w.put(p["hlit"] - 257, 5)
        w.put(p["hdist"] - 1, 5)
        w.put(p["hclen"] - 4, 4)
        for i in range(p["hclen"]):
            w.put(p["cl"][CL_ORDER[i]], 3)
        cl_codes = canonical(p["cl"])
        for s, e, v in p["cl_tokens"]:
            w.put(cl_codes[s], p["cl"][s])
            w.put(v, e)
        ll, dl = p["ll"], p["dl"]
    else:
        w.put(1, 2)
        ll, dl = FIXED_LENGTHS, [5] * 30
    lc, dc = canonical(ll), canonical(dl)
    for kind, v in p["tokens"]:
        if kind == "L":
            w.put(lc[v], ll[v])
        else:
            s, e, x = length_symbol(v)
            w.put(lc[s], ll[s])
            w.put(x, e)
            w.put(dc[0], dl[0])
    w.put(lc[256], ll[256])
    assert len(w.out) * 8 + w.n == bits
    if not last:
        w.put(0, 3)
    w.align()
    if not last:
        w.out += b"\x00\x00\xff\xff"
    assert len(w.out) == nbytes
    return bytes(w.out)


# ---- the file ----
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def adler32(data):
    """by the definition, not by zlib"""
    d = np.frombuffer(data, np.uint8).astype(np.int64)
    a = (1 + int(d.sum())) % 65521
    b = (len(d) + int((d * np.arange(len(d), 0, -1)).sum())) % 65521
    return (b << 16) | a


def blocks(h, w, block_bytes):
    return -(-(h * (1 + 3 * w)) // block_bytes)


def file_bound(h, w, block_bytes):
    """the length of the file whose blocks are all stored"""
    return 33 + h * (1 + 3 * w) + 2 + (5 + 12) * blocks(h, w, block_bytes) + 16 + 12


def encode(img, block_bytes=32768, filter="adaptive", stats=None):
    img = np.asarray(img)
    assert MIN_BLOCK <= block_bytes <= MAX_BLOCK
    h, w, _ = img.shape
    stream = filtered(img, filter)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    n = blocks(h, w, block_bytes)
    for i in range(n):
        body = deflate_block(stream[i * block_bytes:(i + 1) * block_bytes], i == n - 1, stats)
        out += chunk(b"IDAT", (b"\x78\x01" if i == 0 else b"") + body)
    return out + chunk(b"IDAT", struct.pack(">I", adler32(stream))) + chunk(b"IEND", b"")
