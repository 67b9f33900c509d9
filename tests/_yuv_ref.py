"""Numpy restatement of the NV12 <-> RGB definition ("NV12 frames"), the reference the HIP kernels are held to bit for
bit.  Integer arithmetic on bytes throughout; `>>` floors.  Checked on its own by tests/test_yuv_cpu.py.

Layout: y uint8 [B][H][W]; uv uint8 [B][H/2][W/2][2] = (Cb, Cr); chroma sited "left": sample (j, i) at luma column 2i, halfway
between luma rows 2j and 2j + 1."""
import math

import numpy as np

K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb); Kg = 1 - Kr - Kb
COMBOS = [(m, fr) for m in ("bt601", "bt709") for fr in (False, True)]


def _round(v):
    """Round half away from zero."""
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def decode_coeffs(matrix="bt709", full_range=False):
    """(yoff, cy, rv, bu, gu, gv): 16 fractional bits on Y, 13 on the chroma terms (which arrive eight-fold)."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full_range else 16, _round(65536 * ys), _round(8192 * 2 * (1 - kr) * cs), _round(8192 * 2 * (1 - kb) * cs),
            -_round(8192 * 2 * kb * (1 - kb) / kg * cs), -_round(8192 * 2 * kr * (1 - kr) / kg * cs))


def encode_coeffs(matrix="bt709", full_range=False):
    """(yoff, ry, gy, by, ur, ug, ub, vr, vg, vb): gy, ug and vg are derived so that white maps to exactly 235 / 255 and every
    grey to chroma exactly (128, 128)."""
    kr, kb = K[matrix]
    ys, cs = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    ry, by = _round(65536 * kr * ys), _round(65536 * kb * ys)
    gy = _round(65536 * ys) - ry - by
    ub = vr = _round(65536 * 0.5 * cs)
    ur = -_round(65536 * kr / (2 * (1 - kb)) * cs)
    vb = -_round(65536 * kb / (2 * (1 - kr)) * cs)
    return (0 if full_range else 16, ry, gy, by, ur, -(ur + ub), ub, vr, -(vr + vb), vb)


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def upsample_c8(c):
    """One chroma plane [..][h][w] -> eight times its value at every luma position, int32 [..][2h][2w]; no intermediate rounding,
    indices clamped to the plane."""
    c = c.astype(np.int32)
    h, w = c.shape[-2:]
    up = c[..., np.maximum(np.arange(h) - 1, 0), :]
    dn = c[..., np.minimum(np.arange(h) + 1, h - 1), :]
    v = np.empty(c.shape[:-2] + (2 * h, w), np.int32)
    v[..., 0::2, :] = up + 3 * c                                  # luma row 2j
    v[..., 1::2, :] = 3 * c + dn                                  # luma row 2j + 1
    nx = v[..., np.minimum(np.arange(w) + 1, w - 1)]
    out = np.empty(c.shape[:-2] + (2 * h, 2 * w), np.int32)
    out[..., 0::2] = 2 * v                                        # luma column 2i
    out[..., 1::2] = v + nx                                       # luma column 2i + 1
    return out


def nv12_to_rgb8(y, uv, matrix="bt709", full_range=False):
    """y [B][H][W], uv [B][H/2][W/2][2] -> RGB24 uint8 [B][H][W][3]."""
    yoff, cy, rv, bu, gu, gv = decode_coeffs(matrix, full_range)
    cb = upsample_c8(uv[..., 0]) - 1024
    cr = upsample_c8(uv[..., 1]) - 1024
    base = cy * (y.astype(np.int32) - yoff) + 32768
    return np.stack([_clip8((base + rv * cr) >> 16), _clip8((base + gu * cb + gv * cr) >> 16), _clip8((base + bu * cb) >> 16)], axis=-1)


def nv12_to_tensor(y, uv, matrix="bt709", full_range=False):
    """... -> float32 [B][3][H][W] = RGB24 / 255 (ToTensor)."""
    rgb = nv12_to_rgb8(y, uv, matrix, full_range)
    return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


def rgb8_to_nv12(rgb, matrix="bt709", full_range=False):
    """RGB24 uint8 [B][H][W][3] (H, W even) -> (y uint8 [B][H][W], uv uint8 [B][H/2][W/2][2])."""
    yoff, ry, gy, by, ur, ug, ub, vr, vg, vb = encode_coeffs(matrix, full_range)
    p = rgb.astype(np.int32)
    B, H, W, _ = p.shape
    assert H % 2 == 0 and W % 2 == 0
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = _clip8((ry * r + gy * g + by * b + (yoff << 16) + 32768) >> 16)
    x = np.arange(0, W, 2)
    row = p[:, :, np.maximum(x - 1, 0)] + 2 * p[:, :, x] + p[:, :, np.minimum(x + 1, W - 1)]      # [B][H][W/2][3]
    s = row[:, 0::2] + row[:, 1::2]                                                              # eight times the filtered value
    half = (128 << 19) + (1 << 18)
    cb = _clip8((ur * s[..., 0] + ug * s[..., 1] + ub * s[..., 2] + half) >> 19)
    cr = _clip8((vr * s[..., 0] + vg * s[..., 1] + vb * s[..., 2] + half) >> 19)
    return y, np.stack([cb, cr], axis=-1)


def quantise(x):
    """float32 [B][3][H][W] -> RGB24 uint8 [B][H][W][3] = trunc(clamp(x * 255, 0, 255)), NaN -> 0 (what tensor_to_frames writes)."""
    v = x.astype(np.float32) * np.float32(255.0)
    v = np.clip(np.where(np.isnan(v), np.float32(0.0), v), np.float32(0.0), np.float32(255.0))
    return np.ascontiguousarray(v.astype(np.uint8).transpose(0, 2, 3, 1))


def tensor_to_nv12(x, matrix="bt709", full_range=False):
    return rgb8_to_nv12(quantise(x), matrix, full_range)


def decode_float64(y, uv, matrix="bt709", full_range=False):
    """The real-valued conversion on the same upsampled chroma c8 / 8, unrounded and unclipped: float64 [B][H][W][3]."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yoff = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    cb = (upsample_c8(uv[..., 0]) / 8.0 - 128.0) * cs
    cr = (upsample_c8(uv[..., 1]) / 8.0 - 128.0) * cs
    yy = (y.astype(np.float64) - yoff) * ys
    return np.stack([yy + 2 * (1 - kr) * cr, yy - 2 * kb * (1 - kb) / kg * cb - 2 * kr * (1 - kr) / kg * cr, yy + 2 * (1 - kb) * cb], axis=-1)
