"""The numpy definition of the P010 <-> RGB conversions and of the n-bit quantiser q_n (tests/_p010_ref.py, DESIGN 3 "P010 frames")
checked on its own: the coefficient tables, the exact anchors (white, black, greys), the facts that make rounding the right rule at
10 and 16 bits, the distance from the real-valued formula, round trips, the chroma edge clamps by hand, the flags frame_speed.py
takes for it and the refusals of the C entries and of the ops wrappers.  No GPU."""
import numpy as np
import pytest

import _p010_ref as R

DECODE_TABLE = {            # (yoff, cy, rv, bu, gu, gv)
    ("bt601", False): (64, 76533, 13113, 16574, -3219, -6679),
    ("bt601", True): (0, 65536, 11485, 14516, -2819, -5850),
    ("bt709", False): (64, 76533, 14729, 17356, -1752, -4378),
    ("bt709", True): (0, 65536, 12901, 15201, -1535, -3835),
    ("bt2020", False): (64, 76533, 13792, 17597, -1539, -5344),
    ("bt2020", True): (0, 65536, 12080, 15412, -1348, -4681),
}
ENCODE_TABLE = {            # (ry, gy, by, ur, ug, ub, vr, vg, vb)
    ("bt601", False): (16780, 32941, 6398, -9685, -19015, 28700, 28700, -24033, -4667),
    ("bt601", True): (19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329),
    ("bt709", False): (11931, 40136, 4052, -6576, -22124, 28700, 28700, -26068, -2632),
    ("bt709", True): (13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005),
    ("bt2020", False): (14742, 38049, 3328, -8015, -20685, 28700, 28700, -26392, -2308),
    ("bt2020", True): (17216, 44434, 3886, -9151, -23617, 32768, 32768, -30133, -2635),
}


def flat(colours, h=2, w=2):
    """One flat-colour frame per row of `colours`: int32 codes [N][h][w][3]."""
    c = np.asarray(colours, np.int32)
    return np.ascontiguousarray(np.broadcast_to(c[:, None, None, :], (len(c), h, w, 3)))


def colours():
    rng = np.random.default_rng(0)
    corners = [[r, g, b] for r in (0, 1023) for g in (0, 1023) for b in (0, 1023)]
    return np.concatenate([rng.integers(0, 1024, (1 << 20, 3)), np.array(corners + [[512, 512, 512]])]).astype(np.int32)


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_coefficient_rows_equal_the_tables(matrix, full):
    assert R.decode_coeffs(matrix, full) == DECODE_TABLE[matrix, full]
    enc = R.encode_coeffs(matrix, full)
    assert enc[0] == (0 if full else 64) and enc[1:] == ENCODE_TABLE[matrix, full]
    assert all(isinstance(v, int) for v in R.decode_coeffs(matrix, full) + enc)
    assert all(abs(v) < 2 ** 23 for v in R.decode_coeffs(matrix, full) + enc)          # 24-bit signed multiplier operands


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_white_black_and_greys_are_exact(matrix, full):
    y, uv = R.rgb10_to_p010(flat([[1023, 1023, 1023], [0, 0, 0]]), matrix, full)
    assert (R.codes(y[0]) == (1023 if full else 940)).all() and (R.codes(y[1]) == (0 if full else 64)).all()
    greys = np.arange(1024, dtype=np.int32)[:, None].repeat(3, axis=1)
    y, uv = R.rgb10_to_p010(flat(greys), matrix, full)
    assert (R.codes(uv) == 512).all()
    assert (np.diff(R.codes(y)[:, 0, 0]) >= 0).all()
    assert y.dtype == uv.dtype == np.uint16 and not (y & 63).any() and not (uv & 63).any()


@pytest.mark.parametrize("bits", [10, 16])
def test_quantiser_inverts_the_division_for_every_code(bits):
    s = (1 << bits) - 1
    p = np.arange(s + 1, dtype=np.int32)
    assert np.array_equal(R.quantise_n(p.astype(np.float32) / np.float32(s), bits), p)


def test_quantiser_widens_bytes_consistently():
    v = np.arange(256, dtype=np.int32)
    x = v.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(R.quantise_n(x, 16), 257 * v)
    assert np.array_equal(R.quantise_n(x, 10), np.floor(v * 1023 / 255 + 0.5).astype(np.int32))


@pytest.mark.parametrize("bits", [10, 16])
def test_quantiser_special_values(bits):
    s = (1 << bits) - 1
    x = np.array([0.0, 1.0, 0.5, 1.0 / s, (s - 0.001) / s, 2.0, -1.0, np.nan], np.float32)
    # 0.5 S + 0.5 = (S + 1) / 2 exactly; 1 / S comes back as 1 +- an ulp, far from 1.5; S - 0.001 rounds up to S
    assert R.quantise_n(x, bits).tolist() == [0, s, (s + 1) // 2, 1, s, s, 0, 0]
    assert R.quantise_n(x, bits).dtype == np.int32


@pytest.mark.parametrize("matrix,full", R.COMBOS)
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 6, 8), (1, 16, 24)])
def test_decode_is_close_to_the_real_formula(matrix, full, shape):
    """|integer result - float64 formula| <= 0.5 (the final rounding) + the rounded coefficients: 0.5 / 65536 on Y times at most 959
    codes, 0.5 / 65536 on each of at most two eight-fold chroma terms of at most 4096, wherever the float64 value is inside 0..1023."""
    rng = np.random.default_rng(sum(shape))
    B, H, W = shape
    y = R.samples(rng.integers(0, 1024, (B, H, W)))
    uv = R.samples(rng.integers(0, 1024, (B, H // 2, W // 2, 2)))
    y.reshape(-1)[:2] = (0, 1023 << 6)
    uv.reshape(-1)[:2] = (1023 << 6, 0)
    got = R.p010_to_rgb10(y, uv, matrix, full).astype(np.float64)
    ref = np.clip(R.decode_float64(y, uv, matrix, full), 0.0, 1023.0)
    err = np.abs(got - ref).max()
    assert err <= 0.5 + (0.5 * 959 + 2 * 0.5 * 4096) / 65536, err


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_flat_colour_round_trip(matrix, full):
    rgb = flat(colours())
    back = R.p010_to_rgb10(*R.rgb10_to_p010(rgb, matrix, full), matrix, full)
    err = np.abs(back - rgb).max()
    assert err <= (1 if full else 2), err


def test_low_six_bits_are_ignored_on_decode():
    rng = np.random.default_rng(3)
    y = R.samples(rng.integers(0, 1024, (2, 6, 8)))
    uv = R.samples(rng.integers(0, 1024, (2, 3, 4, 2)))
    yn = y | rng.integers(0, 64, y.shape).astype(np.uint16)
    uvn = uv | rng.integers(0, 64, uv.shape).astype(np.uint16)
    assert (yn != y).any() and (uvn != uv).any()
    for matrix, full in R.COMBOS:
        assert np.array_equal(R.p010_to_tensor(yn, uvn, matrix, full), R.p010_to_tensor(y, uv, matrix, full))
    t = R.p010_to_tensor(y, uv)
    assert t.dtype == np.float32 and t.shape == (2, 3, 6, 8)
    assert np.array_equal(t, R.p010_to_rgb10(y, uv).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(1023.0))


def test_chroma_edge_clamps_by_hand():
    from _yuv_ref import upsample_c8
    # 2 x 2: one chroma sample; every neighbour clamps onto it, so all four pixels see 8 x that sample
    uv = R.samples(np.array([[[[360, 800]]]]))
    assert np.array_equal(upsample_c8(R.codes(uv)[..., 0]), np.full((1, 2, 2), 2880))
    assert np.array_equal(upsample_c8(R.codes(uv)[..., 1]), np.full((1, 2, 2), 6400))
    y = R.samples(np.array([[[64, 940], [400, 720]]]))
    # bt709 limited by hand: cb = 2880 - 4096 = -1216, cr = 6400 - 4096 = 2304; base = 76533 * (Y - 64) + 32768
    exp = np.zeros((1, 2, 2, 3), np.int32)
    for (r, c), yy in np.ndenumerate(R.codes(y)[0]):
        base = 76533 * (int(yy) - 64) + 32768
        exp[0, r, c] = [min(1023, max(0, (base + 14729 * 2304) >> 16)),
                        min(1023, max(0, (base - 1752 * -1216 - 4378 * 2304) >> 16)),
                        min(1023, max(0, (base + 17356 * -1216) >> 16))]
    assert np.array_equal(R.p010_to_rgb10(y, uv), exp)
    assert exp[0, 0, 0].tolist() == [518, 0, 0] and exp[0, 0, 1].tolist() == [1023, 902, 701]
    # the encode filter on a 2 x 4 frame with one channel ramp: columns clamp on the left only (x = 0 reads column 0 twice)
    rgb = np.zeros((1, 2, 4, 3), np.int32)
    rgb[0, :, :, 2] = [[40, 200, 360, 1000], [120, 280, 440, 520]]
    s0 = (40 + 2 * 40 + 200) + (120 + 2 * 120 + 280)                        # 960
    s1 = (200 + 2 * 360 + 1000) + (280 + 2 * 440 + 520)                     # 3600
    _, uv = R.rgb10_to_p010(rgb, "bt709", True)
    half = (512 << 19) + (1 << 18)
    assert R.codes(uv)[0, 0, :, 0].tolist() == [(32768 * s0 + half) >> 19, (32768 * s1 + half) >> 19] == [572, 737]
    assert R.codes(uv)[0, 0, :, 1].tolist() == [(-3005 * s0 + half) >> 19, (-3005 * s1 + half) >> 19] == [506, 491]
    # 2 x 2 encode: both column neighbours of x = 0 clamp (x - 1 -> 0; x + 1 = 1 exists)
    rgb = np.zeros((1, 2, 2, 3), np.int32)
    rgb[0, :, :, 0] = [[1023, 0], [1023, 0]]
    _, uv = R.rgb10_to_p010(rgb, "bt601", True)
    s = 2 * (1023 + 2 * 1023 + 0)                                           # 6138
    assert R.codes(uv)[0, 0, 0].tolist() == [(-11058 * s + half) >> 19, min(1023, (32768 * s + half) >> 19)] == [383, 896]


def test_tensor_to_p010_quantises_by_rounding():
    x = np.array([0.0, 1.0, 0.5, 1.0 / 1023, 1022.999 / 1023, 2.0, -1.0, 0.4995, np.nan, 0.25, 0.75, 0.1], np.float32).reshape(1, 3, 2, 2)
    q = R.quantise10(x)
    assert q.transpose(0, 3, 1, 2).reshape(-1).tolist() == [0, 1023, 512, 1, 1023, 1023, 0, 511, 0, 256, 767, 102]
    y, uv = R.tensor_to_p010(x, "bt709", True)
    ry, ruv = R.rgb10_to_p010(q, "bt709", True)
    assert np.array_equal(y, ry) and np.array_equal(uv, ruv)


def test_frame_speed_parser_takes_the_p010_flags():
    import frame_speed as speed_test
    a = speed_test.parse_args(["--pixfmt", "p010"])
    assert (a.pixfmt, a.matrix, a.full_range) == ("p010", "bt709", False)
    a = speed_test.parse_args(["--pixfmt", "p010", "--graph", "--matrix", "bt2020", "--full_range"])
    assert (a.pixfmt, a.matrix, a.full_range, a.graph) == ("p010", "bt2020", True, True)
    assert speed_test.parse_args(["--pixfmt", "p010", "--matrix", "bt601"]).matrix == "bt601"
    for bad in (["--pixfmt", "p010", "--bgr"], ["--pixfmt", "p010", "--source_res", "1080"], ["--pixfmt", "p016"],
                ["--matrix", "bt2020"], ["--pixfmt", "nv12", "--matrix", "bt2020"], ["--pixfmt", "rgb24", "--matrix", "bt2020"],
                ["--pixfmt", "p010", "--matrix", "bt2100"]):
        with pytest.raises(SystemExit):
            speed_test.parse_args(bad)


def test_bad_geometry_is_refused_on_the_host():
    """The argument checks of the C entries and of the ops wrappers run before anything touches a device, so they run here."""
    import torch
    from transformerupscaler_amd import _lib, ops
    lib = _lib.load()
    inval = 1                                                               # hipErrorInvalidValue
    # H, W, y pitch, uv pitch (bytes), matrix, range, B: odd H, odd W, short pitches, odd pitches, matrix and range outside, B too large
    for H, W, yp, up, m, fr, B in [(3, 4, 8, 8, 1, 0, 1), (4, 3, 8, 8, 1, 0, 1), (4, 4, 6, 8, 1, 0, 1), (4, 4, 8, 6, 1, 0, 1),
                                   (4, 4, 9, 8, 1, 0, 1), (4, 4, 8, 9, 1, 0, 1), (4, 4, 8, 8, 3, 0, 1), (4, 4, 8, 8, -1, 0, 1),
                                   (4, 4, 8, 8, 1, 2, 1), (4, 4, 8, 8, 1, -1, 1), (4, 4, 8, 8, 1, 0, 65536)]:
        assert lib.tup_p010_to_f32chw(None, None, 48, yp, 48, up, None, B, H, W, m, fr, None) == inval, (H, W, yp, up, m, fr, B)
        assert lib.tup_f32chw_to_p010(None, None, None, 48, yp, 48, up, B, H, W, m, fr, None) == inval, (H, W, yp, up, m, fr, B)
    assert lib.tup_p010_to_f32chw(None, None, 47, 8, 48, 8, None, 2, 4, 4, 1, 0, None) == inval      # an odd batch stride
    assert lib.tup_f32chw_to_p010(None, None, None, 48, 8, 47, 8, 2, 4, 4, 1, 0, None) == inval
    a = 1 << 12                                                             # any non-null even address: the checks fail before it is used
    assert lib.tup_p010_to_f32chw(None, a, 48, 8, 48, 8, a, 1, 4, 4, 1, 0, None) == inval            # a null pointer with good geometry
    assert lib.tup_p010_to_f32chw(a, None, 48, 8, 48, 8, a, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_p010_to_f32chw(a, a, 48, 8, 48, 8, None, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_f32chw_to_p010(None, a, a, 48, 8, 48, 8, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_f32chw_to_p010(a, None, a, 48, 8, 48, 8, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_f32chw_to_p010(a, a, None, 48, 8, 48, 8, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_p010_to_f32chw(a + 1, a, 48, 8, 48, 8, a, 1, 4, 4, 1, 0, None) == inval           # an odd plane pointer
    assert lib.tup_p010_to_f32chw(None, None, 0, 8, 0, 8, None, 0, 4, 4, 1, 0, None) == 0            # empty: nothing to do
    assert lib.tup_f32chw_to_p010(None, None, None, 0, 8, 0, 8, 1, 0, 4, 2, 0, None) == 0
    y, uv = torch.zeros((4, 8), dtype=torch.uint16), torch.zeros((2, 4, 2), dtype=torch.uint16)
    with pytest.raises(ValueError, match="y lives on cpu"):
        ops.p010_to_tensor(y, uv)
    with pytest.raises(ValueError, match="y lives on cpu"):
        ops.p010_to_tensor(y, uv, matrix="bt2020")
    with pytest.raises(TypeError, match="y must be a uint16"):
        ops.p010_to_tensor(y.to(torch.uint8), uv)
    with pytest.raises(TypeError, match="x must be a float32"):
        ops.tensor_to_p010(torch.zeros((1, 3, 4, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="matrix"):
        ops.p010_to_tensor(y, uv, matrix="bt2100")
    with pytest.raises(ValueError, match="x lives on cpu"):
        ops.tensor_to_p010(torch.zeros((1, 3, 4, 8)))
    with pytest.raises(ValueError, match="even"):
        ops.tensor_to_p010(torch.zeros((1, 3, 3, 8)))
    with pytest.raises(TypeError, match="buf must be a uint16"):
        ops.p010_planes(torch.zeros((6, 20), dtype=torch.uint8), 4, 8)
    with pytest.raises(ValueError):
        ops.p010_planes(torch.zeros((5, 20), dtype=torch.uint16), 4, 8)                              # 3H/2 = 6 rows needed
    yv, uvv = ops.p010_planes(torch.zeros((2, 6, 20), dtype=torch.uint16), 4, 8)                     # views only: fine on the CPU
    assert yv.shape == (2, 4, 8) and uvv.shape == (2, 2, 4, 2) and uvv.stride() == (120, 20, 2, 1)
    assert uvv.data_ptr() - yv.data_ptr() == 2 * 4 * 20
    # the 8-bit format keeps refusing the matrix it does not have
    with pytest.raises(ValueError, match="matrix"):
        ops.nv12_to_tensor(torch.zeros((4, 8), dtype=torch.uint8), torch.zeros((2, 4, 2), dtype=torch.uint8), matrix="bt2020")
