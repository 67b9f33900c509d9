"""Case files of the PNG decoder (ops.png_decode), built at test time: files by Pillow, by zlib's strategies, by the project's own
encoder (tests/_png_ref.py), hand-written deflate streams for what no encoder here emits, re-chunked IDATs, and damaged streams."""
import collections
import functools
import io
import struct
import zlib

import numpy as np

import _png_decode_ref as R
import _png_ref as ENC

Case = collections.namedtuple("Case", "name data")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MODES = {"L": 0, "RGB": 2, "P": 3, "LA": 4, "RGBA": 6}


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def png(H, W, color_type, stream, palette=None, idat=None, depth=8, interlace=0, before=(), between=False):
    """A file around a zlib stream; idat: the bytes per IDAT chunk (None: one chunk); before: chunks ahead of the first IDAT."""
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, interlace))
    for kind, payload in before:
        out += chunk(kind, payload)
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    step = idat or max(len(stream), 1)
    pieces = [stream[i:i + step] for i in range(0, len(stream), step)] or [b""]
    for n, piece in enumerate(pieces):
        out += chunk(b"IDAT", piece)
        if between and n == 0:
            out += chunk(b"tEXt", b"k\0v")
    return out + chunk(b"IEND", b"")


def content(H, W, channels, seed=0):
    """noise on a gradient: every filter is some row's best, and nothing is a long flat run"""
    rng = np.random.default_rng(seed + 131 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    base = (3 * x + 5 * y)[:, :, None] + 40 * np.arange(channels)[None, None, :]
    return ((base + rng.integers(0, 24, (H, W, channels))) & 255).astype(np.uint8)


def filter_rows(samples, bpp, types):
    """uint8 [H][W * bpp] -> the filtered stream with row y under filter types[y % len(types)]"""
    H = samples.shape[0]
    s = samples.astype(np.int32)
    out = bytearray()
    for y in range(H):
        ft = types[y % len(types)]
        cur, up = s[y], s[y - 1] if y else np.zeros_like(s[0])
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        else:
            p = a + up - c
            pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        out += bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def palette_of(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8).tobytes()


def own(H, W, color_type, types, seed=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, entries=256, **kw):
    """A file of this module's own filtering, compressed by zlib"""
    bpp = R.CHANNELS[color_type]
    s = content(H, W, bpp, seed)
    if color_type == 3:
        s = (s.astype(np.int32) % entries).astype(np.uint8)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    raw = filter_rows(s.reshape(H, W * bpp), bpp, types)
    return png(H, W, color_type, co.compress(raw) + co.flush(), palette_of(entries) if color_type == 3 else None, **kw)


# ---- a token-level deflate writer ----
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, table, sym):
        l, c = table[sym]
        self.put(int(format(c, f"0{l}b")[::-1], 2), l)          # a code goes first bit first

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def codes(lens):
    """{symbol: (length, canonical code)}"""
    table, code = {}, 0
    for l in range(1, 16):
        for s, m in enumerate(lens):
            if m == l:
                table[s] = (l, code)
                code += 1
        code <<= 1
    return table


FIXED_LIT = codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = codes([5] * 32)


class Deflate:
    """Blocks written token by token: ("lit", byte), ("match", length, distance); the output they stand for is tracked in .raw"""

    def __init__(self):
        self.b, self.raw = Bits(), bytearray()
        self.b.put(0x78, 8)
        self.b.put(0x01, 8)

    def _tokens(self, tokens, lit, dist):
        for t in tokens:
            if t[0] == "lit":
                self.b.code(lit, t[1])
                self.raw.append(t[1])
            else:
                _, n, d = t
                i = R.LENGTH_BASE.index(max(v for v in R.LENGTH_BASE if v <= n)) if n < 258 else 28
                self.b.code(lit, 257 + i)
                self.b.put(n - R.LENGTH_BASE[i], R.LENGTH_EXTRA[i])
                j = max(k for k in range(30) if R.DIST_BASE[k] <= d)
                self.b.code(dist, j)
                self.b.put(d - R.DIST_BASE[j], R.DIST_EXTRA[j])
                for _ in range(n):
                    self.raw.append(self.raw[-d] if d <= len(self.raw) else 0)      # a damaged case may reach before the start
        self.b.code(lit, 256)

    def fixed(self, tokens, final=False):
        self.b.put(final | 2, 3)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST)

    def dynamic(self, tokens, lit_lens, dist_lens, final=False):
        """every code length is sent as itself under a code-length code of sixteen 4-bit codes"""
        self.b.put(final | 4, 3)
        self.b.put(len(lit_lens) - 257, 5)
        self.b.put(len(dist_lens) - 1, 5)
        self.b.put(19 - 4, 4)
        for s in R.CL_ORDER:
            self.b.put(4 if s < 16 else 0, 3)
        cl = codes([4] * 16 + [0] * 3)
        for l in list(lit_lens) + list(dist_lens):
            self.b.code(cl, l)
        self._tokens(tokens, codes(lit_lens), codes(dist_lens))

    def stored(self, data, final=False):
        self.b.put(final | 0, 3)
        self.b.align()
        self.b.put(len(data), 16)
        self.b.put(len(data) ^ 0xffff, 16)
        for v in data:
            self.b.put(v, 8)
        self.raw += data

    def finish(self, adler=None):
        self.b.align()
        self.b.out += struct.pack(">I", zlib.adler32(bytes(self.raw)) if adler is None else adler)
        return bytes(self.b.out)


def tokenize(raw, forced):
    """literals, but for the forced matches [(position, length, distance)] in ascending order"""
    tokens, at = [], 0
    for pos, n, d in forced:
        assert pos >= at and raw[pos:pos + n] == bytes(raw[pos - d + (k % d)] for k in range(n)), (pos, n, d)
        tokens += [("lit", v) for v in raw[at:pos]] + [("match", n, d)]
        at = pos + n
    return tokens + [("lit", v) for v in raw[at:]]


def grey_rows(H, row):
    """filter byte 0 and row(y) for every row"""
    return b"".join(b"\0" + bytes(row(y)) for y in range(H))


@functools.lru_cache(maxsize=None)
def handwritten():
    """[(name, H, W (grey), stream)], each checked against zlib by the CPU tests"""
    out = []
    rng = np.random.default_rng(11)
    # length 258 at distances 1, 2, 3, 63, 64, 65: a row per distance, periodic with it
    dists = (1, 2, 3, 63, 64, 65)
    pats = [rng.integers(0, 256, d).astype(np.uint8).tobytes() for d in dists]
    raw = grey_rows(len(dists), lambda y: (pats[y] * 400)[:399])
    d = Deflate()
    d.fixed(tokenize(raw, [(400 * y + 1 + dist, 258, dist) for y, dist in enumerate(dists)]), final=True)
    out.append(("len258_short_distances", len(dists), 399, d.finish()))
    # rows that repeat every 4 (1024 bytes): matches at distance 32768 (zlib stops at 32506), across the first flush of 32 KB and
    # across the wrap of a 64 KB ring; the one stream of more than 64 KB
    rows = [rng.integers(0, 256, 255).astype(np.uint8).tobytes() for _ in range(4)]
    raw = grey_rows(300, lambda y: rows[y % 4])
    forced = [(32768 - 100, 258, 1024), (32768 + 300, 258, 32768), (65536 - 100, 258, 32768), (65536 + 200, 258, 3072),
              (70000, 258, 32768), (76800 - 258, 258, 2048)]
    d = Deflate()
    d.fixed(tokenize(raw, forced), final=True)
    out.append(("distance_32768_ring_wrap", 300, 255, d.finish()))
    # a 15-bit code: lengths 1, 2, .., 14, 15, 15 over sixteen symbols; a one-symbol distance code (distance 1, an incomplete code)
    lits = [0, 7, 19, 33, 60, 90, 120, 150, 180, 200, 220, 240, 250]
    lit_lens = [0] * 286
    for l, s in enumerate([0, 256, 285] + lits[1:] + [258], start=1):
        lit_lens[s] = min(l, 15)
    raw = grey_rows(3, lambda y: [lits[(y + k) % 13] for k in range(40)] + [lits[y + 1]] * 300)
    d = Deflate()
    d.dynamic(tokenize(raw, [(341 * y + 42, 258, 1) for y in range(3)] + [(341 * 2 + 300, 4, 1)])[:], lit_lens, [1], final=True)
    out.append(("code_of_15_bits_one_distance", 3, 340, d.finish()))
    # HLIT = 257: no length symbols at all, and an empty distance code
    raw = grey_rows(2, lambda y: range(10 * y, 10 * y + 31))
    d = Deflate()
    d.dynamic(tokenize(raw, []), [8] * 255 + [9] * 2, [0], final=True)
    out.append(("hlit_257", 2, 31, d.finish()))
    # a Huffman block that ends at each of the eight bit phases, followed by a stored block; then empty blocks, the final one empty
    raw = grey_rows(4, lambda y: range(140 + y, 155 + y))            # literals of 8 and of 9 bits
    for phase in range(8):
        for n in range(1, 16):
            d = Deflate()
            d.fixed(tokenize(raw[:n], []))
            if d.b.n == phase:
                break
        assert d.b.n == phase, phase
        d.stored(raw[n:40])
        d.stored(b"")
        d.fixed(tokenize(raw[40:], []))
        d.fixed([], final=True) if phase & 1 else d.stored(b"", final=True)
        out.append((f"stored_after_bit_{(phase + 7) % 8}_final_empty", 4, 15, d.finish()))
    return out


@functools.lru_cache(maxsize=None)
def files():
    """every sound file: [Case]"""
    from PIL import Image
    out = []
    add = lambda name, data: out.append(Case(name, data))
    for (H, W) in ((1, 1), (1, 70), (70, 1)):
        for ct in MODES.values():
            add(f"own_{H}x{W}_ct{ct}", own(H, W, ct, (4, 3, 1, 2, 0), entries=200))
    for ct in MODES.values():
        for ft in range(5):
            add(f"own_5x3_ct{ct}_filter{ft}", own(5, 3, ct, (ft,), seed=ft))
        add(f"own_5x3_ct{ct}_adaptive", own(5, 3, ct, (1, 4, 2, 0, 3)))
        add(f"own_65x67_ct{ct}", own(65, 67, ct, (4, 3, 1, 2, 0, 4, 4, 3), seed=ct))
    # ancillary chunks before and a palette shorter than the indices (index past PLTE is black: not claimed against Pillow)
    add("own_5x3_ct3_short_palette~", own(5, 3, 3, (0, 1), entries=256)[:0] + _short_palette())
    add("own_65x67_ct2_ancillary", own(65, 67, 2, (4,), before=((b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Comment\0x"))))
    # Pillow's writer
    for mode in MODES:
        img = content(65, 67, {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "P": 1}[mode], seed=3)
        im = Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img, "P" if mode == "P" else None)
        if mode == "P":
            im.putpalette(palette_of(256, 9))
        for level, optimize in ((0, False), (1, False), (6, False), (9, False), (6, True)):
            buf = io.BytesIO()
            im.save(buf, "PNG", compress_level=level, optimize=optimize)
            add(f"pillow_{mode}_l{level}{'_opt' if optimize else ''}", buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(content(150, 150, 3, seed=1)).save(buf, "PNG", compress_level=6)
    add("pillow_150x150_rgb_l6", buf.getvalue())
    # zlib's strategies
    for name, strategy in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        add(f"zlib_{name}_150x150", own(150, 150, 2, (1, 4), strategy=strategy))
    # the project's own encoder: a block a chunk, empty stored blocks between them
    for bb, filt in ((256, "adaptive"), (32768, "paeth")):
        add(f"encoder_40x72_{bb}_{filt}", ENC.encode(content(40, 72, 3, seed=2), bb, filt))
    # one stream cut into IDAT chunks of 1, 2, 7 and 65536 bytes
    for n in (1, 2, 7, 65536):
        add(f"rechunk_{n}", own(65, 67, 2, (4, 1, 3), idat=n, between=False))
    for name, H, W, stream in handwritten():
        add("hand_" + name, png(H, W, 0, stream))
    return out


def _short_palette():
    s = content(5, 3, 1, 8)
    s[0, 0, 0], s[4, 2, 0] = 250, 40
    s[1:4] %= 32
    raw = filter_rows(s.reshape(5, 3), 1, (0, 1))
    return png(5, 3, 3, zlib.compress(raw), palette_of(41))


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def claimed(case):
    """whether the pixels are claimed against Pillow"""
    return not case.name.endswith("~")


# ---- damaged streams: small, so that the host program runs every one of them ----
@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, H, W (grey), stream)]: every stream must end with the reference's non-zero status, whatever it is"""
    out = []
    H, W = 4, 15
    raw = grey_rows(H, lambda y: [3 * (y % 2) + 2 * k for k in range(15)])         # rows 2 and 3 repeat rows 0 and 1
    total = len(raw)
    d = Deflate()
    d.fixed(tokenize(raw, []), final=True)
    fixed = d.finish()
    d = Deflate()                                            # a dynamic block (zlib codes so short a stream with the fixed code)
    d.dynamic(tokenize(raw, [(32, 16, 32)]), [8] * 226 + [9] * 60, [4] * 2 + [5] * 28, final=True)
    dyn = d.finish()
    for name, stream in (("fixed", fixed), ("dynamic", dyn)):
        for n in range(2, len(stream)):                      # cut at every byte after the zlib header (png_parse wants that whole)
            out.append((f"{name}_cut_{n}", H, W, stream[:n]))
        rng = np.random.default_rng(2024)
        for i in range(120):                                 # substitutions, but those the stream does not notice (padding bits)
            at, v = int(rng.integers(2, len(stream))), int(rng.integers(0, 256))
            changed = stream[:at] + bytes([v]) + stream[at + 1:]
            if R.inflate(changed, total)[1] != R.OK:
                out.append((f"{name}_byte_{at}_{v}", H, W, changed))
    d = Deflate()
    d.fixed([("lit", 0), ("lit", 1), ("match", 10, 3)] + tokenize(raw[12:], []), final=True)
    out.append(("distance_before_start", H, W, d.finish()))
    d = Deflate()
    d.stored(raw[:20])
    d.stored(raw[20:], final=True)
    s = bytearray(d.finish())
    out.append(("stored_overruns_input", H, W, bytes(s[:2 + 1]) + struct.pack("<HH", 500, 500 ^ 0xffff) + bytes(s[2 + 5:])))
    out.append(("stored_nlen", H, W, bytes(s[:2 + 1]) + struct.pack("<HH", 20, 20) + bytes(s[2 + 5:])))
    d = Deflate()
    d.stored(raw + b"\1\2\3", final=True)
    out.append(("stored_overruns_output", H, W, d.finish()))
    for name, lit_lens in (("oversubscribed", [1] * 4 + [8] * 253), ("incomplete", [9] * 257), ("no_end_of_block", [8] * 256 + [0])):
        d = Deflate()
        d.b.put(5, 3)
        d.b.put(0, 5), d.b.put(0, 5), d.b.put(15, 4)
        for sym in R.CL_ORDER:
            d.b.put(4 if sym < 16 else 0, 3)
        cl = codes([4] * 16 + [0] * 3)
        for l in lit_lens + [0]:
            d.b.code(cl, l)
        d.b.put(0, 64)
        out.append((name, H, W, d.finish(0)))
    d = Deflate()
    d.b.put(7, 3)
    out.append(("block_type_3", H, W, d.finish(0)))
    d = Deflate()
    d.fixed(tokenize(raw[:-3], []), final=True)
    out.append(("output_short", H, W, d.finish()))
    d = Deflate()
    d.fixed(tokenize(raw + b"\0", []), final=True)
    out.append(("output_long", H, W, d.finish()))
    d = Deflate()
    d.fixed(tokenize(raw, [(32, 16, 32)]), final=True)
    out.append(("adler", H, W, d.finish(12345)))
    d = Deflate()
    bad = bytearray(raw)
    bad[16] = 5
    d.fixed(tokenize(bytes(bad), []), final=True)
    out.append(("filter_byte_5", H, W, d.finish()))
    d = Deflate()
    d.fixed([("lit", 0)] * 3 + [("match", 258, 1)], final=True)
    out.append(("match_overruns_output", H, W, d.finish()))
    assert total == H * (1 + W)
    return out
