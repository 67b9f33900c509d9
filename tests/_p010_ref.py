"""Numpy restatement of the P010 <-> RGB definition ("P010 frames") and of the n-bit quantiser q_n, the reference the HIP
kernels are held to bit for bit.  It is the NV12 definition of tests/_yuv_ref.py carried to 10 bits: integer arithmetic on 10-bit
codes throughout, `>>` floors, the same chroma upsampler.  Checked on its own by tests/test_p010_cpu.py.

Layout: y uint16 [B][H][W]; uv uint16 [B][H/2][W/2][2] = (Cb, Cr); a sample holds its 10-bit code in the high bits (code =
sample >> 6, the low six bits are ignored by a reader and written as zero); chroma sited "left" as for NV12."""
import numpy as np

from _yuv_ref import _round, upsample_c8

K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}          # (Kr, Kb); Kg = 1 - Kr - Kb
COMBOS = [(m, fr) for m in ("bt601", "bt709", "bt2020") for fr in (False, True)]
YS, CS = 1023.0 / 876.0, 1023.0 / 896.0         # limited range: Y 64..940, chroma 64..960


def decode_coeffs(matrix="bt709", full_range=False):
    """(yoff, cy, rv, bu, gu, gv): 16 fractional bits on Y, 13 on the chroma terms (which arrive eight-fold)."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (YS, CS)
    return (0 if full_range else 64, _round(65536 * ys), _round(8192 * 2 * (1 - kr) * cs), _round(8192 * 2 * (1 - kb) * cs),
            -_round(8192 * 2 * kb * (1 - kb) / kg * cs), -_round(8192 * 2 * kr * (1 - kr) / kg * cs))


def encode_coeffs(matrix="bt709", full_range=False):
    """(yoff, ry, gy, by, ur, ug, ub, vr, vg, vb): gy, ug and vg are derived so that white maps to exactly 940 / 1023 and every
    grey to chroma exactly (512, 512)."""
    kr, kb = K[matrix]
    ys, cs = (1.0, 1.0) if full_range else (1.0 / YS, 1.0 / CS)
    ry, by = _round(65536 * kr * ys), _round(65536 * kb * ys)
    gy = _round(65536 * ys) - ry - by
    ub = vr = _round(65536 * 0.5 * cs)
    ur = -_round(65536 * kr / (2 * (1 - kb)) * cs)
    vb = -_round(65536 * kb / (2 * (1 - kr)) * cs)
    return (0 if full_range else 64, ry, gy, by, ur, -(ur + ub), ub, vr, -(vr + vb), vb)


def quantise_n(x, bits):
    """q_n: float32 array -> int32 codes 0..2^n - 1.  Four separate fp32 steps: t = x * S; NaN -> 0; clamp to [0, S];
    (int)(t + 0.5f).  Rounds to nearest (the 8-bit rule of the frame path truncates; this one does not)."""
    s = np.float32((1 << bits) - 1)
    t = np.asarray(x, np.float32) * s
    t = np.where(np.isnan(t), np.float32(0.0), t)
    t = np.minimum(np.maximum(t, np.float32(0.0)), s)
    return (t + np.float32(0.5)).astype(np.int32)


def _clip10(v):
    return np.clip(v, 0, 1023).astype(np.int32)


def codes(samples):
    """uint16 samples -> int32 10-bit codes (the low six bits dropped)."""
    return np.asarray(samples).astype(np.int32) >> 6


def samples(code):
    """10-bit codes -> uint16 samples with zero low bits."""
    return (np.asarray(code).astype(np.int32) << 6).astype(np.uint16)


def p010_to_rgb10(y, uv, matrix="bt709", full_range=False):
    """y [B][H][W], uv [B][H/2][W/2][2] uint16 samples -> RGB codes int32 [B][H][W][3] in 0..1023."""
    yoff, cy, rv, bu, gu, gv = decode_coeffs(matrix, full_range)
    c = codes(uv)
    cb = upsample_c8(c[..., 0]) - 4096
    cr = upsample_c8(c[..., 1]) - 4096
    base = cy * (codes(y) - yoff) + 32768
    return np.stack([_clip10((base + rv * cr) >> 16), _clip10((base + gu * cb + gv * cr) >> 16), _clip10((base + bu * cb) >> 16)], axis=-1)


def p010_to_tensor(y, uv, matrix="bt709", full_range=False):
    """... -> float32 [B][3][H][W] = code / 1023 (the IEEE fp32 quotient; never through 8 bits)."""
    rgb = p010_to_rgb10(y, uv, matrix, full_range)
    return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(1023.0)


def rgb10_to_p010(rgb, matrix="bt709", full_range=False):
    """RGB codes [B][H][W][3] in 0..1023 (H, W even) -> (y uint16 [B][H][W], uv uint16 [B][H/2][W/2][2]) samples."""
    yoff, ry, gy, by, ur, ug, ub, vr, vg, vb = encode_coeffs(matrix, full_range)
    p = np.asarray(rgb).astype(np.int32)
    B, H, W, _ = p.shape
    assert H % 2 == 0 and W % 2 == 0
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = _clip10((ry * r + gy * g + by * b + (yoff << 16) + 32768) >> 16)
    x = np.arange(0, W, 2)
    row = p[:, :, np.maximum(x - 1, 0)] + 2 * p[:, :, x] + p[:, :, np.minimum(x + 1, W - 1)]      # [B][H][W/2][3]
    s = row[:, 0::2] + row[:, 1::2]                                                              # eight times the filtered value
    half = (512 << 19) + (1 << 18)
    cb = _clip10((ur * s[..., 0] + ug * s[..., 1] + ub * s[..., 2] + half) >> 19)
    cr = _clip10((vr * s[..., 0] + vg * s[..., 1] + vb * s[..., 2] + half) >> 19)
    return samples(y), samples(np.stack([cb, cr], axis=-1))


def quantise10(x):
    """float32 [B][3][H][W] -> RGB codes int32 [B][H][W][3] = q_10(x)."""
    return np.ascontiguousarray(quantise_n(x, 10).transpose(0, 2, 3, 1))


def tensor_to_p010(x, matrix="bt709", full_range=False):
    return rgb10_to_p010(quantise10(x), matrix, full_range)


def decode_float64(y, uv, matrix="bt709", full_range=False):
    """The real-valued conversion on the same upsampled chroma c8 / 8, unrounded and unclipped: float64 [B][H][W][3] in codes."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yoff = (1.0, 1.0, 0.0) if full_range else (YS, CS, 64.0)
    c = codes(uv)
    cb = (upsample_c8(c[..., 0]) / 8.0 - 512.0) * cs
    cr = (upsample_c8(c[..., 1]) / 8.0 - 512.0) * cs
    yy = (codes(y).astype(np.float64) - yoff) * ys
    return np.stack([yy + 2 * (1 - kr) * cr, yy - 2 * kb * (1 - kb) / kg * cb - 2 * kr * (1 - kr) / kg * cr, yy + 2 * (1 - kb) * cb], axis=-1)
