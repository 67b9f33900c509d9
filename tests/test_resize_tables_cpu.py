"""CPU checks of the host-built tables of the banded bicubic backward and of the streaming-tail plan (resize_taps.py; ops.py only
uploads them): the band and column tables are the transpose of the forward tap matrix, and a plan's strips / bands compute every
tap their owned outputs read."""
import numpy as np
import pytest

from transformerupscaler_amd import resize_taps as R

SIZES = [(1, 1), (5, 17), (16, 16), (17, 33), (45, 720), (90, 1080), (33, 20), (257, 300), (1280, 7680)]
_FORWARD = {}


def _forward_matrix(n_in, n_out):
    """The forward tap matrix [out][in] of bicubic_taps, accumulated in float64 (computed once per size pair, never modified)."""
    if (n_in, n_out) not in _FORWARD:
        idx, w = R.bicubic_taps(n_in, n_out)
        m = np.zeros((n_out, n_in), dtype=np.float64)
        np.add.at(m, (np.repeat(np.arange(n_out), 4), idx.reshape(-1)), w.reshape(-1).astype(np.float64))
        m.setflags(write=False)
        _FORWARD[(n_in, n_out)] = m
    return _FORWARD[(n_in, n_out)]


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_bicubic_bands_are_the_transposed_forward_matrix(n_in, n_out):
    r0, n, bw, nr_max = R.bicubic_bands(n_in, n_out)
    yb = R.BICUBIC_BAND_ROWS
    nb = (n_in + yb - 1) // yb
    assert r0.dtype == n.dtype == np.int32 and bw.dtype == np.float32
    assert r0.shape == n.shape == (nb,) and bw.shape == (nb, nr_max, yb) and nr_max == int(n.max())
    assert (r0 >= 0).all() and (n >= 1).all() and (r0 + n <= n_out).all()
    got = np.zeros((n_out, n_in), dtype=np.float64)
    for b in range(nb):
        cols = min(yb, n_in - b * yb)
        got[r0[b]:r0[b] + n[b], b * yb:b * yb + cols] += bw[b, :n[b], :cols]
        assert not bw[b, n[b]:].any(), b                  # nothing at or beyond the band's row count
        assert not bw[b, :, cols:].any(), b               # ... or beyond the last source row
    err = np.abs(got - _forward_matrix(n_in, n_out)).max()
    print(f"bands {n_in} -> {n_out}: max |scattered - forward| = {err:.1e}")
    # the forward weights are fp32 and at most four are added per entry (measured: 6e-8)
    assert err <= 1e-6


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_bicubic_cols_are_the_transposed_forward_matrix(n_in, n_out):
    cols = R.bicubic_cols(n_in, n_out)
    assert cols is not None
    xoT, xwT, kmax, c0, cn = cols
    assert xoT.dtype == c0.dtype == cn.dtype == np.int32 and xwT.dtype == np.float32 and isinstance(kmax, int)
    assert xoT.shape == xwT.shape == (kmax, n_in)
    assert (xoT >= 0).all() and (xoT < n_out).all()
    # padded slots: weight 0 (the index is in range by the line above)
    cnt = np.diff(R.bicubic_taps_transposed(n_in, n_out)[0])
    pad = np.arange(kmax)[:, None] >= cnt[None, :]
    assert not xwT[pad].any()
    # scattering xwT by xoT gives the forward matrix again, exactly: the slots hold the forward's own fp32 weights, and where taps
    # clamped onto one source share an (output, source) pair both sides add the same terms in float64
    got = np.zeros((n_out, n_in), dtype=np.float64)
    np.add.at(got, (xoT.reshape(-1), np.tile(np.arange(n_in), kmax)), xwT.reshape(-1).astype(np.float64))
    err = np.abs(got - _forward_matrix(n_in, n_out)).max()
    print(f"cols {n_in} -> {n_out}: max |scattered - forward| = {err:.1e}")
    assert err == 0.0
    # every 256-column block reads output columns [c0, c0 + n) only
    nblk = (n_in + 255) // 256
    assert c0.shape == cn.shape == (nblk,)
    for j in range(nblk):
        blk = xoT[:, j * 256:(j + 1) * 256]
        assert blk.min() >= c0[j] and blk.max() < c0[j] + cn[j], j
    assert int(cn.max()) <= 4096


WORKGROUPS = 256 * 4 * 3          # the chip-filling constant ops._tail_stream_plan passes (3 workgroup waves per SIMD)


@pytest.mark.parametrize("shape", [(2, 40, 72, 44, 50), (4, 540, 960, 2160, 3840)])
def test_tail_stream_plan_refuses_more_than_four_taps(shape):
    assert R.tail_stream_plan(*shape, WORKGROUPS) is None


@pytest.mark.parametrize("shape,band", [((1, 12, 60, 24, 120), 12), ((1, 36, 48, 54, 72), 12), ((1, 20, 28, 33, 47), 12),
                                        ((8, 720, 1280, 1080, 1920), 45)])
def test_tail_stream_plan_covers_every_owned_output(shape, band):
    B, H, W, Ho, Wo = shape
    plan = R.tail_stream_plan(*shape, WORKGROUPS)
    assert plan is not None
    ylo, yn, yw, ky, xlo, xn, xw, kx, oxb, oyb, sc, bh, ext = plan
    assert (sc, bh, ext) == (59, band, 1)
    assert all(isinstance(v, int) for v in (ky, kx, sc, bh, ext))
    assert int(yn.max()) <= 4 and int(xn.max()) <= 4
    nstrip, nband = (W + sc - 1) // sc, (H + bh - 1) // bh
    assert oxb.dtype == oyb.dtype == np.int32 and oxb.shape == (nstrip + 1,) and oyb.shape == (nband + 1,)
    for bounds, last in ((oxb, Wo), (oyb, Ho)):
        assert bounds[0] == 0 and bounds[-1] == last and (np.diff(bounds) >= 0).all()
    # a strip starts at LR column s * sc and computes 120 valid HR columns; it gathers at most 128 output columns
    for s in range(nstrip):
        a, b = int(oxb[s]), int(oxb[s + 1])
        assert b - a <= 128, s
        for o in range(a, b):
            assert 2 * s * sc <= xlo[o] and xlo[o] + xn[o] <= 2 * s * sc + 120, (s, o)
    # a band computes the HR rows of LR rows [k * bh, min(H, (k + 1) * bh + ext))
    for k in range(nband):
        for o in range(int(oyb[k]), int(oyb[k + 1])):
            assert 2 * k * bh <= ylo[o] and ylo[o] + yn[o] <= 2 * min(H, (k + 1) * bh + ext), (k, o)
