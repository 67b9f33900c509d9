"""TEST INFRASTRUCTURE ONLY -- the numpy statement of the 4:2:0 JPEG round trip of the training degradations (`ops.degrade` with
`flags & ops.DEGRADE_JPEG_420`, csrc/degrade420.hip).  The front half is `_jpeg_ref.coefficients(frame, quality, 2)`'s, the
back half `_jpeg_decode_ref.fancy_upsample`'s plus libjpeg's rule for images at most 4 pixels wide; tests/test_degrade420_cpu.py pins
`jpeg_roundtrip_420` to Pillow bit for bit.  Blur, noise, the DCT passes, the tables and the quantiser are _degrade_ref's."""
import numpy as np

import _degrade_ref as D

FLAG_JPEG_420 = 4
FIX = D.FIX


def _edge(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def rgb_to_ycc(u):
    R, G, B = np.asarray(u, dtype=np.int64)
    return ((FIX(.299) * R + FIX(.587) * G + FIX(.114) * B + 32768) >> 16,
            (-FIX(.16874) * R - FIX(.33126) * G + FIX(.5) * B + (128 << 16) + 32767) >> 16,
            (FIX(.5) * R - FIX(.41869) * G - FIX(.08131) * B + (128 << 16) + 32767) >> 16)


def downsample(p):
    """p int [H][W], a chroma plane at full size -> [8 mh][8 mw], mh x mw the 16 x 16 MCUs.  Columns are padded in the pixel domain
    up to the MCU width, rows only from H to H + (H & 1); the downsampled plane is then padded downwards by its last row: libjpeg's
    asymmetry, visible in the output."""
    H, W = p.shape
    mh, mw = (H + 15) // 16, (W + 15) // 16
    p = _edge(np.asarray(p, dtype=np.int64), H + (H & 1), mw * 16)
    bias = 1 + (np.arange(mw * 8) & 1)
    d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _edge(d, mh * 8, mw * 8)


def upsample(p, H, W):
    """p int [ceil(H/2)][ceil(W/2)], the real chroma samples -> [H][W]: the triangle filter, or plain replication where libjpeg
    does not use it (at most 2 samples across, W <= 4)."""
    p = np.asarray(p, dtype=np.int64)
    assert p.shape == ((H + 1) // 2, (W + 1) // 2)
    if p.shape[1] <= 2:
        return p.repeat(2, axis=0).repeat(2, axis=1)[:H, :W]
    out = np.zeros((2 * p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    for v, nb in ((0, np.vstack([p[:1], p[:-1]])), (1, np.vstack([p[1:], p[-1:]]))):
        s = 3 * p + nb
        before, after = np.hstack([s[:, :1], s[:, :-1]]), np.hstack([s[:, 1:], s[:, -1:]])
        out[v::2, 0::2] = (3 * s + before + 8) >> 4
        out[v::2, 1::2] = (3 * s + after + 7) >> 4
    return out[:H, :W]


def _codec(plane, table):
    """plane int [8 k][8 l] in 0..255 -> the same after forward DCT, quantiser, dequantiser and inverse DCT."""
    h, w = plane.shape
    blk = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    c = D._fdct_pass(blk, True)
    c = D._fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
    c = np.sign(c) * ((np.abs(c) + (8 * table >> 1)) // (8 * table)) * table
    v = D._idct_pass(c.swapaxes(-1, -2), True).swapaxes(-1, -2)
    px = np.clip(D._idct_pass(v, False) + 128, 0, 255)
    return px.transpose(0, 2, 1, 3).reshape(h, w)


def decoded_planes(u, quality):
    """u int [3][H][W] -> (Y [H][W], Cb, Cr [ceil(H/2)][ceil(W/2)]) as the decoder holds them before it upsamples."""
    assert 1 <= quality <= 100
    _, H, W = u.shape
    Y, Cb, Cr = rgb_to_ycc(u)
    tl, tc = D.quant_table(D.LUMA, quality), D.quant_table(D.CHROMA, quality)
    y = _codec(_edge(Y, (H + 7) & ~7, (W + 7) & ~7), tl)[:H, :W]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return y, _codec(downsample(Cb), tc)[:ch, :cw], _codec(downsample(Cr), tc)[:ch, :cw]


def ycc_to_rgb(Y, Cb, Cr):
    cb, cr = Cb - 128, Cr - 128
    rgb = np.stack([Y + ((FIX(1.402) * cr + 32768) >> 16),
                    Y + ((-FIX(.34414) * cb + 32768 - FIX(.71414) * cr) >> 16),
                    Y + ((FIX(1.772) * cb + 32768) >> 16)])
    return np.clip(rgb, 0, 255)


def jpeg_roundtrip_420(u, quality):
    """u int [3][H][W] (RGB bytes) -> what baseline JPEG at 4:2:0 with the Annex K tables scaled to `quality` decodes to: Pillow's
    ``save(format="JPEG", quality=quality, subsampling=2)`` then ``open().convert("RGB")``."""
    u = np.asarray(u, dtype=np.int64)
    _, H, W = u.shape
    y, cb, cr = decoded_planes(u, quality)
    return ycc_to_rgb(y, upsample(cb, H, W), upsample(cr, H, W))


def degrade_bytes(u, record):
    """u int [3][H][W] bytes -> bytes after the stages the record switches on; flags & 4 selects the 4:2:0 round trip."""
    taps, amp, seed, quality, flags = record
    assert 0 <= quality <= 100 and not flags & ~(D.FLAG_GREY_NOISE | FLAG_JPEG_420) and (quality or not flags & FLAG_JPEG_420)
    u = D.blur(np.asarray(u, dtype=np.int64), taps)
    if amp:
        u = D.noise(u, amp, seed, bool(flags & D.FLAG_GREY_NOISE))
    if quality:
        u = jpeg_roundtrip_420(u, quality) if flags & FLAG_JPEG_420 else D.jpeg_roundtrip(u, quality)
    return u


def degrade(x, records):
    """x float32 [B][3][H][W], one record per sample -> float32 [B][3][H][W] = (float)byte / 255.0f."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 4 and x.shape[1] == 3 and len(records) == x.shape[0]
    out = [degrade_bytes(D.quantise(x[b]), rec).astype(np.float32) / np.float32(255) for b, rec in enumerate(records)]
    return np.stack(out) if out else np.zeros(x.shape, np.float32)
