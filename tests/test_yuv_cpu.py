"""The numpy definition of the NV12 <-> RGB conversions (tests/_yuv_ref.py, DESIGN 3 "NV12 frames") checked on its own: the
coefficient tables, the exact anchors (white, black, greys), its distance from the real-valued formula, round trips, Pillow's
YCbCr, the chroma edge clamps by hand, and the flags frame_speed.py takes for it.  No GPU."""
import numpy as np
import pytest

import _yuv_ref as R

DECODE_TABLE = {            # (yoff, cy, rv, bu, gu, gv)
    ("bt601", False): (16, 76309, 13075, 16525, -3209, -6660),
    ("bt601", True): (0, 65536, 11485, 14516, -2819, -5850),
    ("bt709", False): (16, 76309, 14686, 17305, -1747, -4366),
    ("bt709", True): (0, 65536, 12901, 15201, -1535, -3835),
}
ENCODE_TABLE = {            # (ry, gy, by, ur, ug, ub, vr, vg, vb)
    ("bt601", False): (16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681),
    ("bt601", True): (19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329),
    ("bt709", False): (11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639),
    ("bt709", True): (13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005),
}


def flat(colours, h=4, w=6):
    """One flat-colour frame per row of `colours`: uint8 [N][h][w][3]."""
    c = np.asarray(colours, np.uint8)
    return np.ascontiguousarray(np.broadcast_to(c[:, None, None, :], (len(c), h, w, 3)))


def colours():
    rng = np.random.default_rng(0)
    corners = [[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    return np.concatenate([rng.integers(0, 256, (4096, 3)), np.array(corners + [[128, 128, 128]])]).astype(np.uint8)


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_coefficient_rows_equal_the_tables(matrix, full):
    assert R.decode_coeffs(matrix, full) == DECODE_TABLE[matrix, full]
    enc = R.encode_coeffs(matrix, full)
    assert enc[0] == (0 if full else 16) and enc[1:] == ENCODE_TABLE[matrix, full]
    assert all(isinstance(v, int) for v in R.decode_coeffs(matrix, full) + enc)


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_white_black_and_greys_are_exact(matrix, full):
    y, uv = R.rgb8_to_nv12(flat([[255, 255, 255], [0, 0, 0]]), matrix, full)
    assert (y[0] == (255 if full else 235)).all() and (y[1] == (0 if full else 16)).all()
    greys = np.arange(256, dtype=np.uint8)[:, None].repeat(3, axis=1)
    y, uv = R.rgb8_to_nv12(flat(greys), matrix, full)
    assert (uv == 128).all()
    assert (np.diff(y[:, 0, 0].astype(int)) >= 0).all()


@pytest.mark.parametrize("matrix,full", R.COMBOS)
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 6, 8), (1, 16, 24)])
def test_decode_is_within_half_a_level_of_the_real_formula(matrix, full, shape):
    """|integer result - float64 formula| <= 0.5 (the final rounding) + 0.0175 (the rounded coefficients: 0.5 / 65536 * 239 on Y,
    0.5 / 8192 * 1024 / 8 * 2 on the chroma terms), wherever the float64 value is inside 0..255."""
    rng = np.random.default_rng(sum(shape))
    B, H, W = shape
    y = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    uv = rng.integers(0, 256, (B, H // 2, W // 2, 2), dtype=np.uint8)
    y.reshape(-1)[:2] = (0, 255)
    uv.reshape(-1)[:2] = (255, 0)
    got = R.nv12_to_rgb8(y, uv, matrix, full).astype(np.float64)
    ref = np.clip(R.decode_float64(y, uv, matrix, full), 0.0, 255.0)
    err = np.abs(got - ref).max()
    assert err <= 0.52, err


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_flat_colour_round_trip(matrix, full):
    rgb = flat(colours())
    back = R.nv12_to_rgb8(*R.rgb8_to_nv12(rgb, matrix, full), matrix, full)
    err = np.abs(back.astype(int) - rgb.astype(int)).max()
    assert err <= (1 if full else 2), err


def test_pillow_ycbcr_agrees_within_one_level():
    """Pillow's YCbCr is full-range BT.601 without subsampling; on flat-colour frames the subsampling drops out."""
    from PIL import Image
    cols = colours()
    img = Image.fromarray(cols[None])                                       # one pixel per colour: [1][N][3]
    ycc = np.asarray(img.convert("YCbCr"))[0].astype(int)                   # [N][3]
    y, uv = R.rgb8_to_nv12(flat(cols), "bt601", True)
    assert np.abs(y[:, 0, 0].astype(int) - ycc[:, 0]).max() <= 1
    assert np.abs(uv[:, 0, 0].astype(int) - ycc[:, 1:]).max() <= 1
    # and back: Pillow's RGB of our NV12 values against our decode of them
    ours = R.nv12_to_rgb8(y, uv, "bt601", True)[:, 0, 0].astype(int)
    pil = np.asarray(Image.fromarray(np.concatenate([y[:, :1, 0], uv[:, 0, 0]], axis=1)[None], "YCbCr").convert("RGB"))[0].astype(int)
    assert np.abs(ours - pil).max() <= 1


def test_chroma_edge_clamps_by_hand():
    # 2 x 2: one chroma sample; every neighbour clamps onto it, so all four pixels see 8 x that sample
    uv = np.array([[[[90, 200]]]], np.uint8)
    assert np.array_equal(R.upsample_c8(uv[..., 0]), np.full((1, 2, 2), 720))
    assert np.array_equal(R.upsample_c8(uv[..., 1]), np.full((1, 2, 2), 1600))
    y = np.array([[[16, 235], [100, 180]]], np.uint8)
    # bt709 limited by hand: cb = 720 - 1024 = -304, cr = 1600 - 1024 = 576; base = 76309 * (Y - 16) + 32768
    exp = np.zeros((1, 2, 2, 3), np.uint8)
    for (r, c), yy in np.ndenumerate(y[0]):
        base = 76309 * (int(yy) - 16) + 32768
        exp[0, r, c] = [min(255, max(0, (base + 14686 * 576) >> 16)),
                        min(255, max(0, (base - 1747 * -304 - 4366 * 576) >> 16)),
                        min(255, max(0, (base + 17305 * -304) >> 16))]
    assert np.array_equal(R.nv12_to_rgb8(y, uv), exp)
    assert exp[0, 0, 0].tolist() == [129, 0, 0] and exp[0, 0, 1].tolist() == [255, 225, 175]
    # 2 x 4: one chroma row (vertical taps clamp: 4 C), two samples a = 40, b = 200 -> columns 8a, 4a + 4b, 8b, 8b (right clamp)
    c = np.array([[[40, 200]]], np.uint8)
    assert np.array_equal(R.upsample_c8(c), np.array([[[320, 960, 1600, 1600], [320, 960, 1600, 1600]]]))
    # two chroma rows: luma rows 0..3 weigh (4, 0), (3, 1), (1, 3), (0, 4)
    c = np.array([[[40], [200]]], np.uint8)
    assert np.array_equal(R.upsample_c8(c)[0, :, 0], np.array([320, 640, 1280, 1600]))
    # the encode filter on a 2 x 4 frame with one channel ramp: columns clamp on the left only (x = 0 reads column 0 twice)
    rgb = np.zeros((1, 2, 4, 3), np.uint8)
    rgb[0, :, :, 2] = [[10, 50, 90, 250], [30, 70, 110, 130]]
    s0 = (10 + 2 * 10 + 50) + (30 + 2 * 30 + 70)                            # 240
    s1 = (50 + 2 * 90 + 250) + (70 + 2 * 110 + 130)                         # 900
    _, uv = R.rgb8_to_nv12(rgb, "bt709", True)
    half = (128 << 19) + (1 << 18)
    assert uv[0, 0, :, 0].tolist() == [(32768 * s0 + half) >> 19, (32768 * s1 + half) >> 19] == [143, 184]
    assert uv[0, 0, :, 1].tolist() == [(-3005 * s0 + half) >> 19, (-3005 * s1 + half) >> 19] == [127, 123]
    # 2 x 2 encode: both column neighbours of x = 0 clamp (x - 1 -> 0; x + 1 = 1 exists)
    rgb = np.zeros((1, 2, 2, 3), np.uint8)
    rgb[0, :, :, 0] = [[255, 0], [255, 0]]
    _, uv = R.rgb8_to_nv12(rgb, "bt601", True)
    s = 2 * (255 + 2 * 255 + 0)                                             # 1530
    assert uv[0, 0, 0].tolist() == [(-11058 * s + half) >> 19, min(255, (32768 * s + half) >> 19)]


def test_quantise_is_tensor_to_frames():
    x = np.array([0.0, 1.0, 0.5, 1.0 / 255, 254.999 / 255, 2.0, -1.0, 0.999999, np.nan, 0.25, 0.75, 0.1], np.float32).reshape(1, 3, 2, 2)
    q = R.quantise(x)
    assert q.transpose(0, 3, 1, 2).reshape(-1).tolist() == [0, 255, 127, 1, 254, 255, 0, 254, 0, 63, 191, 25]


def test_frame_speed_parser_takes_the_nv12_flags():
    import frame_speed as speed_test
    a = speed_test.parse_args([])
    assert (a.pixfmt, a.matrix, a.full_range) == ("rgb24", "bt709", False)
    a = speed_test.parse_args(["--pixfmt", "nv12", "--graph", "--matrix", "bt601", "--full_range"])
    assert (a.pixfmt, a.matrix, a.full_range, a.graph) == ("nv12", "bt601", True, True)
    assert speed_test.parse_args(["--bgr", "--source_res", "1080"]).bgr                    # unchanged without the new flags
    for bad in (["--pixfmt", "nv12", "--bgr"], ["--pixfmt", "nv12", "--source_res", "1080"], ["--pixfmt", "i420"],
                ["--matrix", "bt2020"]):
        with pytest.raises(SystemExit):
            speed_test.parse_args(bad)


def test_bad_geometry_is_refused_on_the_host():
    """The argument checks of the C entries and of the ops wrappers run before anything touches a device, so they run here."""
    import torch
    from transformerupscaler_amd import _lib, ops
    lib = _lib.load()
    inval = 1                                                               # hipErrorInvalidValue
    for H, W, yp, up, m, fr, B in [(3, 4, 4, 4, 1, 0, 1), (4, 3, 4, 4, 1, 0, 1), (4, 4, 2, 4, 1, 0, 1), (4, 4, 4, 2, 1, 0, 1),
                                   (4, 4, 4, 4, 2, 0, 1), (4, 4, 4, 4, 1, 2, 1), (4, 4, 4, 4, 1, 0, 65536)]:
        assert lib.tup_nv12_to_f32chw(None, None, 24, yp, 24, up, None, B, H, W, m, fr, None) == inval
        assert lib.tup_f32chw_to_nv12(None, None, None, 24, yp, 24, up, B, H, W, m, fr, None) == inval
    a = 1 << 12                                                             # any non-null address: the checks fail before it is used
    assert lib.tup_nv12_to_f32chw(None, a, 24, 4, 24, 4, a, 1, 4, 4, 1, 0, None) == inval            # a null pointer with good geometry
    assert lib.tup_nv12_to_f32chw(a, None, 24, 4, 24, 4, a, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_nv12_to_f32chw(a, a, 24, 4, 24, 4, None, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_f32chw_to_nv12(None, a, a, 24, 4, 24, 4, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_f32chw_to_nv12(a, None, a, 24, 4, 24, 4, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_f32chw_to_nv12(a, a, None, 24, 4, 24, 4, 1, 4, 4, 1, 0, None) == inval
    assert lib.tup_nv12_to_f32chw(None, None, 0, 4, 0, 4, None, 0, 4, 4, 1, 0, None) == 0            # empty: nothing to do
    assert lib.tup_f32chw_to_nv12(None, None, None, 0, 4, 0, 4, 1, 0, 4, 1, 0, None) == 0
    y, uv = torch.zeros((4, 8), dtype=torch.uint8), torch.zeros((2, 4, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="y lives on cpu"):
        ops.nv12_to_tensor(y, uv)
    with pytest.raises(TypeError, match="y must be a uint8"):
        ops.nv12_to_tensor(y.float(), uv)
    with pytest.raises(ValueError, match="x lives on cpu"):
        ops.tensor_to_nv12(torch.zeros((1, 3, 4, 8)))
    yv, uvv = ops.nv12_planes(torch.zeros((2, 6, 20), dtype=torch.uint8), 4, 8)                       # views only: fine on the CPU
    assert yv.shape == (2, 4, 8) and uvv.shape == (2, 2, 4, 2) and uvv.stride() == (120, 20, 2, 1)
    assert uvv.data_ptr() - yv.data_ptr() == 4 * 20
