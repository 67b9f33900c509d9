"""The contract the r = 2 branch-A kernels rely on (csrc/conv3x3_c64.hip: bra_rows_persistent_kernel, conv5x5_border_fix_kernel):
packing.compose_branch_a puts every output's 5 x 5 kernel on a block of at most 4 x 4 taps, the same rows and columns for every
weight draw, and a ring pixel never has more than 8 live in-image taps.  No GPU needed."""
import pytest
import torch

import _bra_live_ref as L          # tests/ is on sys.path (rootdir-less test modules)
from transformerupscaler_amd import packing


def _weights(r, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((64 * r * r, 64, 3, 3), generator=g) * 0.04, torch.randn((64 * r * r,), generator=g) * 0.1,
            torch.randn((3, 64, 3, 3), generator=g) * 0.04)


@pytest.fixture(scope="module")
def packs():
    return {r: packing.pack_branch_a(*_weights(r, 11 + r), r) for r in (2, 3, 6)}


def test_wp_dead_rows_and_columns(packs):
    """r = 2: wp is exactly zero (also after the bf16 cast) on tap row 4 for si = 0, row 0 for si = 1, column 4 for sj = 0 and
    column 0 for sj = 1, and non-zero on each of the other 16 taps of every output."""
    wp = packs[2][0]
    assert wp.dtype == torch.bfloat16 and tuple(wp.shape) == (1, 1, 25, 16, 64)
    w = wp[0, 0].float().reshape(5, 5, 16, 64)
    assert not bool(w[:, :, 12:].any()), "padding rows"
    for c in range(3):
        for si in range(2):
            for sj in range(2):
                k = w[:, :, c * 4 + si * 2 + sj]                                  # [5][5][64]
                live = torch.ones((5, 5), dtype=torch.bool)
                live[4 if si == 0 else 0, :] = False
                live[:, 4 if sj == 0 else 0] = False
                assert int(live.sum()) == 16
                assert not bool(k[~live].any()), (c, si, sj)
                assert bool((k[live].abs().amax(-1) > 0).all()), (c, si, sj)
                assert torch.equal(live, L.live_mask_variants(2)[0, c * 4 + si * 2 + sj])


@pytest.mark.parametrize("r", [2, 3, 6])
def test_variant_support_is_the_closed_form(packs, r):
    """All 9 variants, every output: the non-zero taps of wv are exactly the closed-form support rectangle."""
    wv = packs[r][2].float().reshape(9, 3 * r * r, 5, 5, 64)
    nz = wv.abs().amax(-1) > 0
    assert torch.equal(nz, L.live_mask_variants(r))


@pytest.mark.parametrize("r,H,W", [(2, 16, 16), (2, 1, 1), (2, 1, 3), (2, 2, 5), (3, 6, 7), (3, 1, 2), (6, 4, 5), (6, 1, 1)])
def test_ring_pixels_have_at_most_8_live_taps(packs, r, H, W):
    """Every ring pixel of an H x W map (16 x 16 at r = 2: all 9 variants occur): the live in-image taps read off the weights are
    the closed-form rectangle, at most 8 of them -- 2 x <= 4 on the first / last row, <= 4 x 2 on the side columns."""
    nz = packs[r][2].float().reshape(9, 3 * r * r, 5, 5, 64).abs().amax(-1) > 0
    Hs, Ws = H * r, W * r
    seen = set()
    for Y, X in L.ring_pixels(Hs, Ws):
        rowmode, colmode = L.modes(Y, X, Hs, Ws)
        v = rowmode * 3 + colmode
        seen.add(v)
        y, si, x, sj = Y // r, Y % r, X // r, X % r
        inimg = torch.zeros((5, 5), dtype=torch.bool)
        for ty in range(5):
            for tx in range(5):
                inimg[ty, tx] = 0 <= y + ty - 2 < H and 0 <= x + tx - 2 < W
        ty0, ny, tx0, nx = L.live_rect(r, si, sj, rowmode, colmode, y, x, H, W)
        assert ny >= 1 and nx >= 1 and ny * nx <= 8, (Y, X, ny, nx)
        assert (ny <= 2 and nx <= 4) if rowmode else (ny <= 4 and nx <= 2), (Y, X, ny, nx)
        rect = torch.zeros((5, 5), dtype=torch.bool)
        rect[ty0:ty0 + ny, tx0:tx0 + nx] = True
        for c in range(3):
            assert torch.equal(nz[v, c * r * r + si * r + sj] & inimg, rect), (Y, X, c)
    if (H, W) == (16, 16):
        assert seen == set(range(1, 9))
