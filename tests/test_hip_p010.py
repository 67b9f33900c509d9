"""`tup_p010_to_f32chw` / `tup_f32chw_to_p010` (csrc/p010.hip) through `ops.p010_to_tensor` / `ops.tensor_to_p010` on the MI355X,
bit-exact against the numpy definition tests/_p010_ref.py (itself checked in tests/test_p010_cpu.py).

Shapes (B, H, W): (1, 2, 2) every clamp at once; (1, 4, 6) W % 4 == 2; (2, 6, 8) the vector path with interior and border chroma
rows; (3, 10, 520) lanes, waves and workgroups crossed along x, with a batch stride; (1, 34, 66) odd chroma counts; (1, 720, 1280)
for the default matrix and range only.  Each runs on separate contiguous planes and on the two views of one [B][3H/2][pitch]
buffer with pitch = W + 6 samples (still dword-aligned where W % 4 == 0) and pitch = W + 3 samples (never: the element path).
Decode inputs carry random low six bits; encode outputs must have none."""
import functools

import numpy as np
import pytest
import torch

import _p010_ref as R
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 2, 2), (1, 4, 6), (2, 6, 8), (3, 10, 520), (1, 34, 66)]
CASES = [(s, m, f) for s in SHAPES for m, f in R.COMBOS] + [((1, 720, 1280), "bt709", False)]
PADS = [None, 6, 3]                     # separate planes; one buffer with pitch = W + pad samples
SENTINEL = 0xA5A5


def gpu(a):
    """A numpy array on the GPU (uint16 goes over as it is)."""
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def put(view, a):
    """Copy a uint16 array into a (strided) uint16 view on the GPU; through int16 views of both, bit for bit."""
    view.view(torch.int16).copy_(gpu(a).view(torch.int16))


@functools.lru_cache(maxsize=None)
def surface(shape):
    """Random P010 samples that include codes 0 and 1023 in both planes, with random low six bits."""
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    yc = rng.integers(0, 1024, (B, H, W))
    uvc = rng.integers(0, 1024, (B, H // 2, W // 2, 2))
    yc.reshape(-1)[[0, -1]] = (0, 1023)
    uvc.reshape(-1)[[0, -1]] = (1023, 0)
    y = R.samples(yc) | rng.integers(0, 64, yc.shape).astype(np.uint16)
    uv = R.samples(uvc) | rng.integers(0, 64, uvc.shape).astype(np.uint16)
    y.setflags(write=False); uv.setflags(write=False)
    return y, uv


@functools.lru_cache(maxsize=None)
def decoded(shape, matrix, full):
    out = R.p010_to_tensor(*surface(shape), matrix, full)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_output(shape):
    """`rand * 1.2 - 0.1` with the special values of q_10 in front, and the codes q_10 makes of it."""
    B, H, W = shape
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(B * 7919 + H * 31 + W)) * 1.2 - 0.1
    special = torch.tensor([0.0, 1.0, 0.5, 1.0 / 1023, 1022.999 / 1023, 2.0, -1.0, 0.4995, float("nan")])
    x.view(-1)[:len(special)] = special
    x = x.numpy()
    rgb = R.quantise10(x)
    x.setflags(write=False); rgb.setflags(write=False)
    return x, rgb


@functools.lru_cache(maxsize=None)
def encoded(shape, matrix, full):
    return R.rgb10_to_p010(model_output(shape)[1], matrix, full)


def single_buffer(shape, pad):
    """One allocation of B frames [3H/2][pitch] plus one spare pitch row, all SENTINEL; returns (flat, buf [B][3H/2][pitch])."""
    B, H, W = shape
    pitch, rows = W + pad, H + H // 2
    flat = gpu(np.full((B * rows * pitch + pitch,), SENTINEL, np.uint16))
    return flat, flat[:B * rows * pitch].view(B, rows, pitch)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape,matrix,full", CASES)
def test_decode_bit_exact(shape, matrix, full, pad):
    B, H, W = shape
    y, uv = (gpu(a) for a in surface(shape))
    if pad is not None:
        _, buf = single_buffer(shape, pad)
        yv, uvv = ops.p010_planes(buf, H, W)
        assert yv.data_ptr() == buf.data_ptr() and uvv.data_ptr() == buf.data_ptr() + 2 * H * (W + pad)
        assert yv.stride() == ((H + H // 2) * (W + pad), W + pad, 1) and uvv.stride()[2:] == (2, 1)
        assert H == 2 or uvv.stride(1) == W + pad            # (the stride of a one-row plane means nothing)
        put(yv, surface(shape)[0]); put(uvv, surface(shape)[1])
        y, uv = yv, uvv
    got = ops.p010_to_tensor(y, uv, matrix=matrix, full_range=full)
    assert got.shape == (B, 3, H, W) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), decoded(shape, matrix, full))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape,matrix,full", CASES)
def test_encode_bit_exact_and_padding_untouched(shape, matrix, full, pad):
    B, H, W = shape
    x = gpu(model_output(shape)[0])
    ry, ruv = encoded(shape, matrix, full)
    assert not (ry & 63).any() and not (ruv & 63).any()
    if pad is None:
        y, uv = ops.tensor_to_p010(x, matrix=matrix, full_range=full)
        assert y.shape == (B, H, W) and uv.shape == (B, H // 2, W // 2, 2) and y.dtype == uv.dtype == torch.uint16
        y, uv = y.cpu().numpy(), uv.cpu().numpy()
        assert not (y & 63).any() and not (uv & 63).any(), "low six bits written"
        assert np.array_equal(y, ry) and np.array_equal(uv, ruv)
        return
    flat, buf = single_buffer(shape, pad)
    out = ops.p010_planes(buf, H, W)
    y, uv = ops.tensor_to_p010(x, matrix=matrix, full_range=full, out=out)
    assert y is out[0] and uv is out[1]
    pitch, rows = W + pad, H + H // 2
    exp = np.full((B * rows * pitch + pitch,), SENTINEL, np.uint16)
    ev = exp[:B * rows * pitch].reshape(B, rows, pitch)
    ev[:, :H, :W] = ry
    ev[:, H:, :W] = ruv.reshape(B, H // 2, W)
    got = flat.cpu().numpy()
    assert np.array_equal(got[-pitch:], exp[-pitch:]), "the row after the last frame was written"
    assert np.array_equal(got, exp)                          # planes equal the reference, every padding sample still the sentinel


def test_default_arguments_are_bt709_limited_and_single_frames_are_accepted():
    shape = (1, 6, 8)
    y, uv = (gpu(a) for a in surface(shape))
    got = ops.p010_to_tensor(y[0], uv[0])                    # [H][W] and [H/2][W/2][2]
    assert np.array_equal(got.cpu().numpy(), R.p010_to_tensor(*surface(shape), "bt709", False))
    x = gpu(model_output(shape)[0])
    y2, uv2 = ops.tensor_to_p010(x[0])
    ry, ruv = R.rgb10_to_p010(model_output(shape)[1], "bt709", False)
    assert np.array_equal(y2.cpu().numpy(), ry) and np.array_equal(uv2.cpu().numpy(), ruv)


def test_decode_keeps_ten_bits():
    """The tensor is code / 1023, never routed through 8 bits: a luma ramp of all 1024 codes under grey chroma comes back as 1024
    distinct values, each the fp32 quotient."""
    y = R.samples(np.arange(1024).reshape(1, 2, 512))
    uv = R.samples(np.full((1, 1, 256, 2), 512))
    got = ops.p010_to_tensor(gpu(y), gpu(uv), full_range=True).cpu().numpy()
    exp = (np.arange(1024).astype(np.float32) / np.float32(1023.0)).reshape(2, 512)
    assert np.array_equal(got[0, 0], exp) and np.array_equal(got[0, 1], exp) and np.array_equal(got[0, 2], exp)


@pytest.mark.parametrize("matrix,full", R.COMBOS)
def test_round_trip_of_an_encoded_flat_frame_is_exact(matrix, full):
    """s = an encode output of flat frames -> tensor_to_p010(p010_to_tensor(s)) == s: q_10 inverts the division (rounding, not
    truncation, is what makes that hold) and on a flat frame both filters drop out.  The definition itself returns s for all but about
    one flat colour in 10^4 (numpy, 400 000 random colours: 33 to 61 per matrix and range come back one code off, after three roundings
    in a row), so the colours are a fixed set that the reference returns exactly, which is asserted first; the kernels must then do
    the same, and must re-quantise every decoded pixel to the code it came from."""
    rng = np.random.default_rng(17)
    cols = np.concatenate([rng.integers(0, 1024, (29, 3)), [[0, 0, 0], [1023, 1023, 1023], [512, 512, 512]]])
    rgb = np.ascontiguousarray(np.broadcast_to(cols[:, None, None, :], (32, 4, 8, 3))).astype(np.int32)
    ry, ruv = R.rgb10_to_p010(rgb, matrix, full)
    back = R.p010_to_rgb10(ry, ruv, matrix, full)
    ry1, ruv1 = R.rgb10_to_p010(back, matrix, full)
    assert np.array_equal(ry1, ry) and np.array_equal(ruv1, ruv), "choose colours that the definition returns exactly"
    x = gpu(rgb.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(1023.0))
    s0 = ops.tensor_to_p010(x, matrix=matrix, full_range=full)
    assert np.array_equal(s0[0].cpu().numpy(), ry) and np.array_equal(s0[1].cpu().numpy(), ruv)
    t1 = ops.p010_to_tensor(*s0, matrix=matrix, full_range=full)
    s1 = ops.tensor_to_p010(t1, matrix=matrix, full_range=full)
    assert np.array_equal(s1[0].cpu().numpy(), ry) and np.array_equal(s1[1].cpu().numpy(), ruv)
    assert np.array_equal(R.quantise10(t1.cpu().numpy()), back)              # q_10(p / 1023) == p for every decoded pixel


def test_invalid_arguments_raise_before_any_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    u16 = lambda *s: torch.zeros(s, dtype=torch.uint16, device=DEV)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
    bad_decode = {
        "odd H": (u16(1, 5, 8), u16(1, 2, 4, 2)),
        "odd W": (u16(1, 4, 7), u16(1, 2, 3, 2)),
        "uv rows": (u16(1, 4, 8), u16(1, 4, 4, 2)),
        "uv pairs": (u16(1, 4, 8), u16(1, 2, 8, 1)),
        "uv batch": (u16(2, 4, 8), u16(1, 2, 4, 2)),
        "uv rank": (u16(1, 4, 8), u16(2, 8)),
        "float y": (f32(1, 4, 8), u16(1, 2, 4, 2)),
        "uint8 y": (torch.zeros((1, 4, 8), dtype=torch.uint8, device=DEV), u16(1, 2, 4, 2)),
        "int16 uv": (u16(1, 4, 8), u16(1, 2, 4, 2).view(torch.int16)),
        "cpu y": (u16(1, 4, 8).cpu(), u16(1, 2, 4, 2)),
        "cpu uv": (u16(1, 4, 8), u16(1, 2, 4, 2).cpu()),
        "strided y columns": (u16(1, 4, 16)[:, :, ::2], u16(1, 2, 4, 2)),
        "strided uv pairs": (u16(1, 4, 8), u16(1, 2, 8, 2)[:, :, ::2]),
        "transposed y": (u16(1, 8, 4).transpose(1, 2), u16(1, 2, 4, 2)),
    }
    for what, (y, uv) in bad_decode.items():
        with pytest.raises((ValueError, TypeError)):
            ops.p010_to_tensor(y, uv)
            pytest.fail(f"p010_to_tensor accepted: {what}")
        if y.dtype == torch.uint16 and uv.dtype == torch.uint16 and y.dim() == 3 and y.shape[1] % 2 == 0 and y.shape[2] % 2 == 0:
            B, H, W = y.shape
            with pytest.raises((ValueError, TypeError)):     # the same planes as an output
                ops.tensor_to_p010(f32(B, 3, H, W), out=(y, uv))
                pytest.fail(f"tensor_to_p010 accepted out: {what}")
    bad_encode = {
        "odd H": f32(1, 3, 5, 8), "odd W": f32(1, 3, 4, 7), "two channels": f32(1, 2, 4, 8), "uint16 x": u16(1, 3, 4, 8),
        "cpu x": f32(1, 3, 4, 8).cpu(), "strided x": f32(1, 3, 4, 16)[..., ::2],
    }
    for what, x in bad_encode.items():
        with pytest.raises((ValueError, TypeError)):
            ops.tensor_to_p010(x)
            pytest.fail(f"tensor_to_p010 accepted: {what}")
    with pytest.raises(ValueError, match="matrix"):
        ops.p010_to_tensor(u16(1, 4, 8), u16(1, 2, 4, 2), matrix="bt2100")
    with pytest.raises(ValueError, match="matrix"):
        ops.tensor_to_p010(f32(1, 3, 4, 8), matrix="rec2020")
    with pytest.raises(ValueError, match="overlap"):
        ops.tensor_to_p010(f32(2, 3, 4, 8), out=(u16(1, 4, 8).expand(2, 4, 8), u16(2, 2, 4, 2)))
    with pytest.raises(ValueError):
        ops.p010_planes(u16(6, 8), 5, 8)
    with pytest.raises(ValueError):
        ops.p010_planes(u16(5, 8), 4, 8)                     # 3H/2 = 6 rows needed
    with pytest.raises(TypeError):
        ops.p010_planes(torch.zeros((6, 8), dtype=torch.uint8, device=DEV), 4, 8)
    assert launched == []


def test_c_abi_rejects_bad_geometry_before_any_launch():
    lib = _lib.load()
    inval = 1                                                # hipErrorInvalidValue
    y, uv = (torch.zeros(128, dtype=torch.uint8, device=DEV) for _ in range(2))
    dst = torch.zeros(96, device=DEV)
    args = lambda H, W, yp, up, m=1, fr=0, B=1, yo=0: (y.data_ptr() + yo, uv.data_ptr(), 128, yp, 128, up, dst.data_ptr(), B, H, W, m, fr, None)
    for H, W, yp, up, m, fr, yo in [(3, 4, 8, 8, 1, 0, 0), (4, 3, 8, 8, 1, 0, 0), (4, 4, 6, 8, 1, 0, 0), (4, 4, 8, 6, 1, 0, 0),
                                    (4, 4, 9, 8, 1, 0, 0), (4, 4, 8, 9, 1, 0, 0), (4, 4, 8, 8, 3, 0, 0), (4, 4, 8, 8, -1, 0, 0),
                                    (4, 4, 8, 8, 0, 2, 0), (4, 4, 8, 8, 1, 0, 1)]:
        a = args(H, W, yp, up, m, fr, yo=yo)
        assert lib.tup_p010_to_f32chw(*a) == inval, (H, W, yp, up, m, fr, yo)
        assert lib.tup_f32chw_to_p010(a[6], a[0], a[1], *a[2:6], *a[7:]) == inval, (H, W, yp, up, m, fr, yo)
    assert lib.tup_p010_to_f32chw(*args(4, 4, 8, 8, B=65536)) == inval
    assert lib.tup_p010_to_f32chw(*args(0, 4, 8, 8)) == 0 and lib.tup_p010_to_f32chw(*args(4, 4, 8, 8, B=0)) == 0
    torch.cuda.synchronize()
    assert (dst == 0).all()


def test_p010_frame_path_under_hipgraph_replay_equals_eager():
    """P010 surface -> model -> P010 planes captured into a hipGraph (frame_speed.py --pixfmt p010 --graph) replays to exactly the
    eager result, also for a new frame copied into the static buffer; the frame size of the NV12 twin of this test."""
    import importlib
    from transformerupscaler_amd.weights import deterministic_state_dict
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.cuda().eval()
    H, W = 90, 120
    rng = np.random.default_rng(5)
    f0, f1 = (gpu(rng.integers(0, 65536, (H + H // 2, W)).astype(np.uint16)) for _ in range(2))

    def one(buf):
        return ops.tensor_to_p010(m(ops.p010_to_tensor(*ops.p010_planes(buf, H, W), matrix="bt2020"), res_out=(270, 360)), matrix="bt2020")

    same = lambda a, b: np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    with torch.no_grad():
        eager0, eager1 = [t.clone() for t in one(f0)], [t.clone() for t in one(f1)]
        torch.cuda.synchronize()
        assert eager0[0].shape == (1, 270, 360) and eager0[1].shape == (1, 135, 180, 2) and eager0[0].dtype == torch.uint16
        assert not same(eager0[0], eager1[0])
        static_in = f0.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = one(static_in)
        graph.replay(); torch.cuda.synchronize()
        assert same(static_out[0], eager0[0]) and same(static_out[1], eager0[1])
        static_in.copy_(f1)
        graph.replay(); torch.cuda.synchronize()
        assert same(static_out[0], eager1[0]) and same(static_out[1], eager1[1])


def test_frame_speed_converts_rgb_files_to_p010_surfaces_once(tmp_path):
    """frame_speed.py --pixfmt p010 --data_dir: each RGB file becomes one uint16 [3H/2][W] surface, Y on top, by tensor_to_p010 on the
    GPU; a byte v arrives as q_10(v / 255)."""
    import argparse
    from PIL import Image
    import frame_speed as speed_test
    h, w = speed_test.resolutions["350"]
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    for i, a in enumerate(imgs):
        Image.fromarray(a).save(tmp_path / f"f{i}.png")
    args = argparse.Namespace(data_dir=str(tmp_path), frames=2, res_in="350", source_res=None, matrix="bt2020", full_range=False)
    bufs, source = speed_test.load_p010_frames(args, torch.device(DEV, 0))
    assert source == "files" and len(bufs) == 2
    for buf, a in zip(bufs, imgs):
        rgb10 = np.floor(a.astype(np.int64) * 1023 / 255 + 0.5).astype(np.int32)
        ry, ruv = R.rgb10_to_p010(rgb10[None], "bt2020", False)
        got = buf.cpu().numpy()
        assert got.shape == (h + h // 2, w) and got.dtype == np.uint16
        assert np.array_equal(got[:h], ry[0]) and np.array_equal(got[h:], ruv[0].reshape(h // 2, w))
