"""TEST INFRASTRUCTURE ONLY -- the Python statement of the self-synchronising index of a JPEG scan without restart markers
(csrc/jpeg_sync.h and jpeg_sync.hip, `ops.jpeg_scan_index(index="sync")`), on top of the bit-by-bit walker of
tests/_jpeg_decode_ref.py, with the lanes emulated one after another.

A position is the logical bit: 8 x (payload bytes before it, stuffed zeros not counted) + the bit in the byte.  `serial_rows` is the
serial walk's record at the start of every MCU row, `sync_rows` the parallel algorithm's; both give {row: (logical bit, mcu0, pred0,
pred1, pred2)} and a status.  `record_bit` turns a segment record of the GPU (pos, acc, n) into the logical bit it denotes."""
import _jpeg_decode_ref as R


def raw_starts(scan):
    """raw index of every payload byte, in order; and the payload bytes as a string of bits"""
    starts, out, i, hit = [], bytearray(), 0, R.END
    while i < len(scan):
        if scan[i] == 0xFF:
            if i + 1 >= len(scan):
                break
            if scan[i + 1] != 0:
                hit = R.MARKER
                break
            starts.append(i)
            out.append(0xFF)
            i += 2
            continue
        starts.append(i)
        out.append(scan[i])
        i += 1
    return starts, "".join(format(v, "08b") for v in out), hit


def record_bit(scan, pos, n):
    """8 x (payload bytes before raw byte `pos`) - n"""
    payload, i = 0, 0
    while i < pos:
        i += 2 if scan[i] == 0xFF else 1
        payload += 1
    return 8 * payload - n


class _Reader(R._Bits):
    """tests/_jpeg_decode_ref._Bits over the readable part of the scan, placed at any bit"""

    def __init__(self, bits, hit, pos):
        self.bits, self.hit, self.pos = bits, hit, pos


def _tables(info):
    tables = {k: R.huffman_map(v) for k, v in info["huffman_tables"].items()}
    return None if any(t is None for t in tables.values()) else tables


def _symbol(rd, tables, info, comps, j, k, sums, go_on=False):
    """One symbol (a code with its value bits) from state (j, k) -> (j, k, blocks ended, error).  go_on=False: an error raises R._Stop as
    the walker does.  go_on=True (csrc/jpeg_sync.h): a bad size or index is returned as the error and the walk goes on behind the code, a
    bad code behind one skipped bit; only bits that are not there still raise.  sums=None: nothing is summed."""
    c, err = comps[j], 0

    def fail(code):
        if not go_on:
            raise R._Stop(code)
        return code
    try:
        if k == 0:
            s = rd.symbol(tables[(0, info["dc_selectors"][c])])
            if s > 11:
                err = fail(R.BAD_SIZE)
            elif s:
                diff = rd.receive(s)
                if sums is not None:
                    sums[c] = (sums[c] + diff) % 65536
            k = 1
        else:
            rs = rd.symbol(tables[(1, info["ac_selectors"][c])])
            r, size = rs >> 4, rs & 15
            if size == 0:
                k = k + 16 if r == 15 else 64
            elif size > 10:
                err = fail(R.BAD_SIZE)
                k += r + 1
            else:
                k += r
                if k > 63:
                    err, k = fail(R.BAD_INDEX), 64
                else:
                    rd.receive(size)
                    k += 1
    except R._Stop as e:
        if not go_on or e.args[0] != R.BAD_CODE or rd.pos >= len(rd.bits):
            raise
        err = R.BAD_CODE
        rd.pos += 1
    if k >= 64:
        return (j + 1) % len(comps), 0, 1, err
    return j, k, 0, err


def _pred(v):
    return (v + 32768) % 65536 - 32768


def serial_rows(scan, info):
    """The serial walk: ({row: (bit, mcu0, p0, p1, p2)}, status), rows as far as their start was reached."""
    _, mh, mw, comps = R.geometry(info)
    tables = _tables(info)
    if tables is None:
        return {}, R.BAD_TABLE
    _, bits, hit = raw_starts(scan)
    rd, rows, sums = _Reader(bits, hit, 0), {}, [0, 0, 0]
    try:
        for mcu in range(mh * mw):
            if mcu % mw == 0:
                rows[mcu // mw] = (rd.pos, mcu) + tuple(_pred(v) for v in sums)
            j, k = 0, 0
            while True:
                j, k, ended, _ = _symbol(rd, tables, info, comps, j, k, sums)
                if ended and j == 0:
                    break
    except R._Stop as e:
        return rows, e.args[0]
    return rows, R.OK


def walk(bits, hit, starts, readable, stop_raw, state, tables, info, comps, visit=None):
    """From state (bit, j, k) to the first symbol that begins in a raw byte >= stop_raw: (exit or None, blocks, [three DC sums], first
    error).  starts: the raw index of every payload byte; readable: the raw index behind the last of them.  visit(bit, blocks so far,
    sums so far) at every MCU start passed.  Blocks, sums and visits end at the walk's first error; the walk goes on where it can."""
    if state is None:
        return None, 0, [0, 0, 0], 0
    pos, j, k = state
    rd, blocks, sums, first = _Reader(bits, hit, pos), 0, [0, 0, 0], 0
    while True:
        byte = rd.pos // 8
        if (starts[byte] if byte < len(starts) else readable) >= stop_raw:
            return (rd.pos, j, k), blocks, sums, first
        if j == 0 and k == 0 and visit is not None and not first:
            visit(rd.pos, blocks, list(sums))
        try:
            j, k, ended, err = _symbol(rd, tables, info, comps, j, k, None if first else sums, go_on=True)
        except R._Stop as e:
            return None, blocks, sums, first or e.args[0]
        first = first or err
        blocks += ended and not first


def sync_rows(scan, info, T, lanes_per_span=256):
    """The parallel index, lanes one after another: ({row: (bit, mcu0, p0, p1, p2)}, status, rounds, subsequences).  A scan whose
    confirmed chain does not reach every MCU gives the serial walk's answer, as the kernel's fallback does."""
    _, mh, mw, comps = R.geometry(info)
    tables = _tables(info)
    if tables is None:
        return {}, R.BAD_TABLE, 0, 0
    starts, bits, hit = raw_starts(scan)
    n = len(scan)
    nsub = (n + T - 1) // T
    raw_to_payload = {s: i for i, s in enumerate(starts)}
    readable = starts[-1] + (2 if scan[starts[-1]] == 0xFF else 1) if starts else 0

    def assume(at):
        at += 1 if scan[at - 1] == 0xFF and scan[at] == 0 else 0
        # a subsequence past the readable bytes (behind a marker) is walked by no confirmed chain; any state does for it
        return (8 * raw_to_payload[at], 0, 0) if at in raw_to_payload else None

    bpm, need, rows = len(comps), mh * mw * len(comps), {}
    first, before, pre, rounds = (0, 0, 0), 0, [0, 0, 0], 0
    for s0 in range(0, nsub, lanes_per_span):
        if first is None or before >= need:
            break
        lanes = min(lanes_per_span, nsub - s0)
        stop = [min((s0 + i + 1) * T, n) for i in range(lanes)]
        entry = [first if i == 0 else assume((s0 + i) * T) for i in range(lanes)]
        res = [walk(bits, hit, starts, readable, stop[i], entry[i], tables, info, comps) for i in range(lanes)]
        for _ in range(lanes):
            new = [entry[0]] + [res[i - 1][0] for i in range(1, lanes)]
            again = [i for i in range(lanes) if new[i] != entry[i]]
            if not again:
                break
            for i in again:
                entry[i] = new[i]
            for i in again:
                res[i] = walk(bits, hit, starts, readable, stop[i], entry[i], tables, info, comps)
            rounds += 1
        else:
            raise AssertionError("the rounds did not settle within the number of lanes")
        for i in range(lanes):
            if first is None:                                       # a lane before this one still has an error: the chain ended there
                break
            def visit(bit, blocks, sums, base=before, dc=list(pre)):
                mcu = (base + blocks) // bpm
                if mcu < mh * mw and mcu % mw == 0:
                    assert (base + blocks) % bpm == 0 and mcu // mw not in rows
                    rows[mcu // mw] = (bit, mcu) + tuple(_pred(dc[c] + sums[c]) for c in range(3))
            walk(bits, hit, starts, readable, stop[i], entry[i], tables, info, comps, visit)
            before += res[i][1]
            pre = [(pre[c] + res[i][2][c]) % 65536 for c in range(3)]
            first = None if res[i][3] else res[i][0]
    if before >= need:
        return rows, R.OK, rounds, nsub
    rows, status = serial_rows(scan, info)
    return rows, status, rounds, nsub


# ---- the files tests/test_jpeg_sync_cpu.py and tests/test_hip_jpeg_sync.py share: all of them without restart markers ----
def _save(a, **kw):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _noise(hw, seed, channels=3):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, hw + (channels,) if channels > 1 else hw, dtype=np.uint8)


NOISE_SEED = 0                          # found by search: with it a boundary of the 256 x 256 scan falls on the 00 of an FF 00 pair
LENGTH_SEEDS = {-1: 207, 0: 341, 1: 729}   # found by search: 24 x 40 noise whose scan is k T - 1, k T and k T + 1 bytes (T = 132)
_cache = {}


def cases():
    """(name, file bytes), made once.  H x W: 8 x 8 grey (less than a subsequence); 16 x 16 4:2:0 and 17 x 9 / 9 x 17 4:4:4 (cropped MCUs);
    flat grey 8 wide and flat 4:2:0 16 wide, many rows (a row start every byte or two) and the same lying down; 256 x 256 noise at
    quality 95, 4:4:4 (more than 256 subsequences: a second span, stuffed bytes, a boundary on a stuffed zero); a gradient with noise
    and optimised tables; scans of k T - 1, k T and k T + 1 bytes; 4096 x 4096 flat grey with optimised tables: one-symbol DC and AC
    tables, one bit a code, two bits a block, the most block ends a span of 256 subsequences can hold (four a byte)."""
    if "cases" in _cache:
        return _cache["cases"]
    import numpy as np
    y, x = np.mgrid[0:72, 0:104].astype(np.float32)
    grad = np.stack([x * 2.4, 128 + 100 * np.sin(x / 17.0 + y / 11.0), y * 3.5], -1) + np.random.default_rng(5).normal(0, 6, (72, 104, 3))
    out = [("grey-8x8", _save(_noise((8, 8), 1, 1), quality=75)),
           ("420-16x16", _save(_noise((16, 16), 2), quality=75, subsampling=2)),
           ("444-17x9", _save(_noise((17, 9), 3), quality=75, subsampling=0)),
           ("444-9x17", _save(_noise((9, 17), 3), quality=75, subsampling=0)),
           ("flat-grey-2048x8", _save(np.full((2048, 8), 128, np.uint8), quality=75)),
           ("flat-grey-8x2048", _save(np.full((8, 2048), 128, np.uint8), quality=75)),
           ("flat-420-1024x16", _save(np.full((1024, 16, 3), 90, np.uint8), quality=75, subsampling=2)),
           ("flat-420-16x1024", _save(np.full((16, 1024, 3), 90, np.uint8), quality=75, subsampling=2)),
           ("noise-256x256-q95", _save(_noise((256, 256), NOISE_SEED), quality=95, subsampling=0)),
           ("flat-grey-optimize-4096x4096", _save(np.full((4096, 4096), 128, np.uint8), quality=75, optimize=True)),
           ("gradient-optimize", _save(np.clip(grad, 0, 255).astype(np.uint8), quality=85, subsampling=2, optimize=True))]
    out += [(f"length-kT{d:+d}", _save(_noise((24, 40), seed), quality=75, subsampling=2)) for d, seed in LENGTH_SEEDS.items()]
    _cache["cases"] = tuple(out)
    return _cache["cases"]


def damaged_batch():
    """Four files of one geometry (40 x 72, 4:2:0): good, truncated mid-scan, good, a byte in the middle replaced by FF D9."""
    if "batch" not in _cache:
        good = [_save(_noise((40, 72), s), quality=75, subsampling=2) for s in (11, 12)]
        f = _save(_noise((40, 72), 13), quality=75, subsampling=2)
        cut = f[:f.index(b"\xff\xda") + 14 + (len(f) - f.index(b"\xff\xda")) // 2] + b"\xff\xd9"
        g = _save(_noise((40, 72), 14), quality=75, subsampling=2)
        mid = (g.index(b"\xff\xda") + len(g)) // 2
        _cache["batch"] = (good[0], cut, good[1], g[:mid] + b"\xff\xd9" + g[mid + 1:])
    return _cache["batch"]
