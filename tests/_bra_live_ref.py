"""Shared by test_bra_live_taps_cpu.py and test_hip_bra_live_taps.py: the support of the composed branch-A conv
(packing.compose_branch_a) restated in closed form, the dead-tap masks that follow from it, and an fp64 application of the
bf16 composed weights.

Composition: Conv3x3(64 -> 64 r^2) -> PixelShuffle(r) -> Conv3x3(64 -> 3).  HR output row r*y + si reads HR rows r*y + si + d - 1
for the second conv's taps d in [dlo, dhi] (rowmode 1 drops d = 0, rowmode 2 drops d = 2); HR row r*y + s' is LR row
y + floor(s' / r), whose first-conv taps cover LR offsets -1..1 around it, i.e. tap rows floor(s' / r) + 1 .. + 3 of the 5 x 5.
Columns alike.  This is the formula csrc/conv3x3_c64.hip's conv5x5_border_fix_kernel evaluates per ring pixel.
"""
import torch
import torch.nn.functional as F


def support(r, s, mode):
    """Inclusive tap range [lo, hi] of sub-position s along one axis under border mode 0 / 1 (first) / 2 (last)."""
    dlo, dhi = (1 if mode == 1 else 0), (1 if mode == 2 else 2)
    return (s + dlo - 1) // r + 1, (s + dhi - 1) // r + 3


def live_rect(r, si, sj, rowmode, colmode, y, x, H, W):
    """(ty0, ny, tx0, nx): the live in-image taps of HR pixel (r*y + si, r*x + sj) of an H x W LR map."""
    ylo, yhi = support(r, si, rowmode)
    xlo, xhi = support(r, sj, colmode)
    ty0, tx0 = max(ylo, 2 - y), max(xlo, 2 - x)
    return ty0, min(yhi, H + 1 - y) - ty0 + 1, tx0, min(xhi, W + 1 - x) - tx0 + 1


def modes(Y, X, Hs, Ws):
    return (1 if Y == 0 else (2 if Y == Hs - 1 else 0)), (1 if X == 0 else (2 if X == Ws - 1 else 0))


def ring_pixels(Hs, Ws):
    return [(Y, X) for Y in range(Hs) for X in range(Ws) if Y in (0, Hs - 1) or X in (0, Ws - 1)]


def live_mask_variants(r):
    """bool [9][3 r^2][5][5]: taps inside the support of output n = c r^2 + si r + sj under variant rowmode*3 + colmode."""
    m = torch.zeros((9, 3, r, r, 5, 5), dtype=torch.bool)
    for rowmode in range(3):
        for colmode in range(3):
            for si in range(r):
                for sj in range(r):
                    (ylo, yhi), (xlo, xhi) = support(r, si, rowmode), support(r, sj, colmode)
                    m[rowmode * 3 + colmode, :, si, sj, ylo:yhi + 1, xlo:xhi + 1] = True
    return m.reshape(9, 3 * r * r, 5, 5)


def poison_dead_taps(wp, wv, r=2, value=3.0e4):
    """Copies of (wp [1][1][25][rows][64], wv [9][n][25][64]) with every tap outside the support set to +-value."""
    live = live_mask_variants(r)
    n = 3 * r * r
    wp2, wv2 = wp.clone(), wv.clone()
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0).to(wp.dtype).to(wp.device) * value
    dead_p = (~live[0]).reshape(n, 25).t().to(wp.device)                      # [25][n]
    wp2[0, 0, :, :n][dead_p] = sign
    wv2[(~live).reshape(9, n, 25).to(wv.device)] = sign
    return wp2, wv2


def apply_fp64(x_nhwc, wp, bias, wv, bv, r, relu):
    """fp64 application of the bf16 composed weights: interior from wp / bias, the outermost HR ring from variant wv / bv.
    x_nhwc bf16 [B][H][W][64] (CPU) -> float64 [B][3][H r][W r]."""
    n = 3 * r * r
    x = x_nhwc.double().permute(0, 3, 1, 2)
    B, _, H, W = x.shape
    Hs, Ws = H * r, W * r

    def conv(w_n25c, b_n):                    # [n][25][64], [n]
        w = w_n25c.double().reshape(n, 5, 5, 64).permute(0, 3, 1, 2)
        return F.pixel_shuffle(F.conv2d(x, w, b_n.double(), padding=2), r)

    out = conv(wp[0, 0, :, :n].permute(1, 0, 2), bias)
    yy = torch.arange(Hs).reshape(Hs, 1).expand(Hs, Ws)
    xx = torch.arange(Ws).reshape(1, Ws).expand(Hs, Ws)
    rowmode = (yy == 0).long() + 2 * ((yy == Hs - 1) & (yy != 0)).long()
    colmode = (xx == 0).long() + 2 * ((xx == Ws - 1) & (xx != 0)).long()
    var = rowmode * 3 + colmode
    for v in range(1, 9):
        sel = var == v
        if bool(sel.any()):
            out[:, :, sel] = conv(wv[v], bv[v])[:, :, sel]
    return out.clamp_min(0) if relu else out
