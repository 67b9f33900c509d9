"""TEST INFRASTRUCTURE ONLY -- the numpy statement of the training degradations (`ops.degrade`, csrc/degrade.hip): blur,
noise and a JPEG round trip on bytes, all in integers.  tests/test_degrade_cpu.py pins `jpeg_roundtrip` to Pillow's 4:4:4 round trip
bit for bit.  A record is (taps, noise_amp, noise_seed, quality, flags); every stage has an "off" value that is an exact identity.
Integers are held in int64 here and asserted to fit in 32 bits, which is what the kernel computes in."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2                     # Pillow's, for 8-bit images
TAPS_OFF = (1 << PRECISION_BITS, 0, 0, 0)
NOISE_UNIT = 147.80054                          # sqrt(4 * (256^2 - 1) / 12): the standard deviation of a sum of four uniform bytes
FLAG_GREY_NOISE = 1
RECORD_OFF = (TAPS_OFF, 0, 0, 0, 0)

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                  + [99] * 32, dtype=np.int64).reshape(8, 8)

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _fits(*arrays):
    for a in arrays:
        assert np.abs(a).max(initial=0) < 2 ** 31, "an intermediate leaves 32 bits"


def FIX(x):
    return int(x * 65536 + .5)


def quantise(x):
    """fp32 in [0, 1] -> bytes: clip(floor(v * 255.0f + 0.5f), 0, 255), every operation rounded to fp32."""
    v = np.asarray(x, dtype=np.float32) * np.float32(255.0)
    v = np.floor(v + np.float32(0.5))
    return np.clip(v, 0, 255).astype(np.int64)


def drop_hash(seed, idx):
    """csrc/common.h drop_hash."""
    idx = np.asarray(idx, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (idx * np.uint64(0x9E3779B1) + np.uint64(seed)) & m
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def blur_taps(sigma):
    """(k0, k1, k2, k3): a Gaussian truncated at radius 3, normalised, in 22-bit fixed point; the rounding residue goes to k0."""
    if sigma <= 0:
        return TAPS_OFF
    g = np.exp(-0.5 * (np.arange(4, dtype=np.float64) / float(sigma)) ** 2)
    g /= g[0] + 2.0 * g[1:].sum()
    k = [int(round(float(v) * (1 << PRECISION_BITS))) for v in g]
    k[0] += (1 << PRECISION_BITS) - (k[0] + 2 * sum(k[1:]))
    return tuple(k)


def noise_amp(sigma):
    return int(round(float(sigma) * 65536 / NOISE_UNIT))


def blur(u, taps):
    """u int [3][H][W]: the horizontal pass, then the vertical pass, each rounded to bytes; indices clamped to the image."""
    k = [int(v) for v in taps]
    assert len(k) == 4 and min(k) >= 0 and k[0] + 2 * sum(k[1:]) == 1 << PRECISION_BITS
    for axis in (2, 1):
        n = u.shape[axis]
        acc = np.full(u.shape, 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for j in range(-3, 4):
            acc += k[abs(j)] * np.take(u, np.clip(np.arange(n) + j, 0, n - 1), axis=axis)
        _fits(acc)
        u = np.clip(acc >> PRECISION_BITS, 0, 255)
    return u


def noise_values(seed, H, W, grey):
    """n int [3][H][W]: sums of the four bytes of one hash per element, centred."""
    y, x = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    pix = y * np.uint64(W) + x
    e = np.stack([pix] * 3) if grey else np.stack([pix * np.uint64(3) + np.uint64(c) for c in range(3)])
    h = drop_hash(seed, e & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return (h & 255) + (h >> 8 & 255) + (h >> 16 & 255) + (h >> 24) - 510


def noise(u, amp, seed, grey):
    n = noise_values(seed, u.shape[1], u.shape[2], grey)
    _fits(n * int(amp))
    return np.clip(u + ((n * int(amp) + (1 << 15)) >> 16), 0, 255)


def quant_table(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of the slow integer forward DCT along the last axis of d[..., 8]."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    _fits(t4, t5, t6, t7, z1, z2, z3, z4, z5)
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _idct_pass(d, first):
    """One pass of the slow integer inverse DCT along the last axis of d[..., 8]."""
    d = [d[..., i] for i in range(8)]
    n = 11 if first else 18
    z1 = (d[2] + d[6]) * F_0_541
    t2, t3 = z1 - d[6] * F_1_847, z1 + d[2] * F_0_765
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    _fits(t10, t11, t12, t13, t0, t1, t2, t3, z5, t10 + t3, t10 - t3, t11 + t2, t11 - t2, t12 + t1, t12 - t1, t13 + t0, t13 - t0)
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def jpeg_roundtrip(u, quality):
    """u int [3][H][W] (RGB bytes) -> what baseline JPEG at 4:4:4 with the Annex K tables scaled to `quality` decodes to."""
    assert 1 <= quality <= 100
    _, H, W = u.shape
    H8, W8 = (H + 7) & ~7, (W + 7) & ~7
    u = np.pad(np.asarray(u, dtype=np.int64), ((0, 0), (0, H8 - H), (0, W8 - W)), mode="edge")
    R, G, B = u
    ycc = np.stack([
        (FIX(.299) * R + FIX(.587) * G + FIX(.114) * B + 32768) >> 16,
        (-FIX(.16874) * R - FIX(.33126) * G + FIX(.5) * B + (128 << 16) + 32767) >> 16,
        (FIX(.5) * R - FIX(.41869) * G - FIX(.08131) * B + (128 << 16) + 32767) >> 16])
    # blocks [3][H8/8][W8/8][row][col]
    blk = (ycc - 128).reshape(3, H8 // 8, 8, W8 // 8, 8).transpose(0, 1, 3, 2, 4)
    c = _fdct_pass(blk, True)                                           # rows
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)          # columns
    t = np.stack([quant_table(LUMA, quality), quant_table(CHROMA, quality), quant_table(CHROMA, quality)])[:, None, None]
    q = np.sign(c) * ((np.abs(c) + (8 * t >> 1)) // (8 * t))
    c = q * t
    w = _idct_pass(c.swapaxes(-1, -2), True).swapaxes(-1, -2)           # columns
    px = np.clip(_idct_pass(w, False) + 128, 0, 255)                    # rows
    Y, Cb, Cr = px.transpose(0, 1, 3, 2, 4).reshape(3, H8, W8)
    cb, cr = Cb - 128, Cr - 128
    rgb = np.stack([Y + ((FIX(1.402) * cr + 32768) >> 16),
                    Y + ((-FIX(.34414) * cb + 32768 - FIX(.71414) * cr) >> 16),
                    Y + ((FIX(1.772) * cb + 32768) >> 16)])
    return np.clip(rgb, 0, 255)[:, :H, :W]


def degrade_bytes(u, record):
    """u int [3][H][W] bytes -> bytes after the stages the record switches on."""
    taps, amp, seed, quality, flags = record
    assert 0 <= quality <= 100 and not flags & ~FLAG_GREY_NOISE
    u = blur(np.asarray(u, dtype=np.int64), taps)
    if amp:
        u = noise(u, amp, seed, bool(flags & FLAG_GREY_NOISE))
    if quality:
        u = jpeg_roundtrip(u, quality)
    return u


def degrade(x, records):
    """x float32 [B][3][H][W] in [0, 1], one record per sample -> float32 [B][3][H][W] = (float)byte / 255.0f."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 4 and x.shape[1] == 3 and len(records) == x.shape[0]
    out = [degrade_bytes(quantise(x[b]), rec).astype(np.float32) / np.float32(255) for b, rec in enumerate(records)]
    return np.stack(out) if out else np.zeros(x.shape, np.float32)
