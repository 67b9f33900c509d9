"""CPU check of the scatter form of decoder_conv2 (csrc/decoder_fused.hip, tup_decoder_fused_fwd): packing.pack_dec2_scatter's
permuted columns are read back in the K order of decoder_conv1's epilogue registers (lane group g, K-step s, element j <-> input
channel 16g + 8s + j), the 27 projections per dec pixel are summed the way the kernel splits them (dx inside a 32-column tile,
dy inside a wave's two rows, the rest through the row seam plane and the tile-edge column buffer, added by the finishing pass in
its fixed order) -- against F.conv2d.  The only rounding is the bf16 of the packed weight.  No GPU, no library."""
import torch
import torch.nn.functional as F

from transformerupscaler_amd import packing as P


def _scatter_decoder(dec, wz, bias):
    """dec [B][H][W][64] fp64 (NHWC, as the epilogue holds it); wz the packed [48][64] image -> residual [B][3][H][W]."""
    B, H, W, _ = dec.shape
    A = wz.double().reshape(3, 4, 4, 2, 4, 8)                          # [dy][c][dx][s][g][j]: column kk = 32 s + 8 g + j
    frag = dec.reshape(B, H, W, 4, 2, 8)                               # channel 16 g + 8 s + j = [g][s][j] of the pixel
    Z = torch.einsum("ycxsgj,bhwgsj->bhwycx", A, frag)[..., :3, :3]    # [B][H][W][dy][c][dx]
    tile = torch.arange(W) // 32
    zp = F.pad(Z, (0, 0, 0, 0, 0, 0, 1, 1))                           # zero columns -1 and W
    same_l = torch.cat([torch.tensor([False]), tile[1:] == tile[:-1]])  # column x - 1 is in x's tile
    same_r = torch.cat([tile[:-1] == tile[1:], torch.tensor([False])])  # column x + 1 is in x's tile
    # H[b][y][x][dy][c] = sum_dx Z_{dy,dx}(y, x + dx - 1) inside the tile
    Hs = zp[:, :, 1:-1, :, :, 1] + zp[:, :, :-2, :, :, 0] * same_l.view(1, 1, W, 1, 1).double() \
        + zp[:, :, 2:, :, :, 2] * same_r.view(1, 1, W, 1, 1).double()
    zero = torch.zeros_like(Hs[:, :1])
    Hn = torch.cat([Hs[:, 1:], zero], 1)                               # H of row y + 1 (zero past the image)
    Hp = torch.cat([zero, Hs[:, :-1]], 1)                              # H of row y - 1
    even = (torch.arange(H) % 2 == 0).view(1, H, 1, 1)
    part = torch.where(even, Hs[..., 1, :] + Hn[..., 2, :], Hp[..., 0, :] + Hs[..., 1, :])
    seam = torch.where(even, Hp[..., 0, :], Hn[..., 2, :])
    res = bias.double().view(1, 1, 1, 3) + part + seam                 # [B][H][W][3]
    # tile-edge columns: raw Z of a tile's first column (dx = 2, to x - 1) and last column (dx = 0, to x + 1)
    for x in range(W):
        src, dx = (x + 1, 2) if x % 32 == 31 and x + 1 < W else ((x - 1, 0) if x % 32 == 0 and x > 0 else (None, None))
        if src is None:
            continue
        for dy in range(3):
            ys = torch.arange(H) + dy - 1
            ok = (ys >= 0) & (ys < H)
            res[:, ok, x, :] += Z[:, ys[ok], src, dy, :, dx]
    return res.permute(0, 3, 1, 2)


def test_dec2_scatter_permutation_and_gather():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(3, 64, 3, 3, generator=g) / 24
    b = torch.randn(3, generator=g)
    wz = P.pack_dec2_scatter(w)
    assert wz.shape == (48, 64) and wz.dtype == torch.bfloat16
    wr = w.to(torch.bfloat16).double()
    for B, H, W in ((1, 13, 45), (2, 8, 32), (1, 5, 20), (1, 17, 97)):
        dec = torch.relu(torch.randn(B, H, W, 64, generator=g)).double()
        ref = F.conv2d(dec.permute(0, 3, 1, 2), wr, b.double(), padding=1)
        got = _scatter_decoder(dec, wz, b)
        assert (got - ref).abs().max().item() < 1e-10, (B, H, W)


def test_dec2_scatter_padding_rows_are_zero():
    wz = P.pack_dec2_scatter(torch.randn(3, 64, 3, 3)).float().reshape(3, 4, 4, 64)
    assert wz[:, 3].abs().max() == 0 and wz[:, :, 3].abs().max() == 0
