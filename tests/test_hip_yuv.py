"""`tup_nv12_to_f32chw` / `tup_f32chw_to_nv12` (csrc/image_io.hip) through `ops.nv12_to_tensor` / `ops.tensor_to_nv12` on the MI355X,
bit-exact against the numpy definition tests/_yuv_ref.py (itself checked in tests/test_yuv_cpu.py).

Shapes (B, H, W): (1, 2, 2) every clamp at once; (1, 4, 6) W % 4 == 2; (2, 6, 8) the aligned path with interior and border chroma
rows; (3, 10, 520) lanes, waves and workgroups crossed along x, with a batch stride; (1, 34, 66) odd chroma counts; (1, 720, 1280)
for the default matrix and range only.  Each runs on separate contiguous planes and on the two views of one [B][3H/2][pitch]
buffer with pitch = W + 12 (still dword-aligned where W % 4 == 0) and pitch = W + 6 (never: the element path)."""
import functools

import numpy as np
import pytest
import torch

import _yuv_ref as R
from oracle import image_io_oracle as IO
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 2, 2), (1, 4, 6), (2, 6, 8), (3, 10, 520), (1, 34, 66)]
CASES = [(s, m, f) for s in SHAPES for m, f in R.COMBOS] + [((1, 720, 1280), "bt709", False)]
PADS = [None, 12, 6]                    # separate planes; one buffer with pitch = W + pad
SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def surface(shape):
    """Random NV12 bytes that include 0 and 255 in both planes."""
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    y = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    uv = rng.integers(0, 256, (B, H // 2, W // 2, 2), dtype=np.uint8)
    y.reshape(-1)[[0, -1]] = (0, 255)
    uv.reshape(-1)[[0, -1]] = (255, 0)
    y.setflags(write=False); uv.setflags(write=False)
    return y, uv


@functools.lru_cache(maxsize=None)
def decoded(shape, matrix, full):
    out = R.nv12_to_tensor(*surface(shape), matrix, full)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_output(shape):
    """`rand * 1.2 - 0.1` with the special values of tests/test_image_io.py, and the bytes tensor_to_frames makes of it."""
    B, H, W = shape
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(B * 7919 + H * 31 + W)) * 1.2 - 0.1
    n = min(8, x.numel())
    x.view(-1)[:n] = torch.tensor([0.0, 1.0, 0.5, 1.0 / 255, 254.999 / 255, 2.0, -1.0, 0.999999])[:n]
    x = x.numpy()
    rgb = IO.to_frame(x)
    x.setflags(write=False); rgb.setflags(write=False)
    return x, rgb


@functools.lru_cache(maxsize=None)
def encoded(shape, matrix, full):
    return R.rgb8_to_nv12(model_output(shape)[1], matrix, full)


def single_buffer(shape, pad):
    """One allocation of B frames [3H/2][pitch] plus one spare pitch row, all SENTINEL; returns (flat, buf [B][3H/2][pitch])."""
    B, H, W = shape
    pitch, rows = W + pad, H + H // 2
    flat = torch.full((B * rows * pitch + pitch,), SENTINEL, dtype=torch.uint8, device=DEV)
    return flat, flat[:B * rows * pitch].view(B, rows, pitch)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape,matrix,full", CASES)
def test_decode_bit_exact(shape, matrix, full, pad):
    B, H, W = shape
    y, uv = (torch.from_numpy(a.copy()).to(DEV) for a in surface(shape))
    if pad is not None:
        _, buf = single_buffer(shape, pad)
        yv, uvv = ops.nv12_planes(buf, H, W)
        assert yv.data_ptr() == buf.data_ptr() and uvv.data_ptr() == buf.data_ptr() + H * (W + pad)
        assert yv.stride() == ((H + H // 2) * (W + pad), W + pad, 1) and uvv.stride()[2:] == (2, 1)
        assert H == 2 or uvv.stride(1) == W + pad            # (the stride of a one-row plane means nothing)
        yv.copy_(y); uvv.copy_(uv)
        y, uv = yv, uvv
    got = ops.nv12_to_tensor(y, uv, matrix=matrix, full_range=full)
    assert got.shape == (B, 3, H, W) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), decoded(shape, matrix, full))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape,matrix,full", CASES)
def test_encode_bit_exact_and_padding_untouched(shape, matrix, full, pad):
    B, H, W = shape
    x = torch.from_numpy(model_output(shape)[0].copy()).to(DEV)
    ry, ruv = encoded(shape, matrix, full)
    if pad is None:
        y, uv = ops.tensor_to_nv12(x, matrix=matrix, full_range=full)
        assert y.shape == (B, H, W) and uv.shape == (B, H // 2, W // 2, 2) and y.dtype == uv.dtype == torch.uint8
        assert np.array_equal(y.cpu().numpy(), ry) and np.array_equal(uv.cpu().numpy(), ruv)
        return
    flat, buf = single_buffer(shape, pad)
    out = ops.nv12_planes(buf, H, W)
    y, uv = ops.tensor_to_nv12(x, matrix=matrix, full_range=full, out=out)
    assert y is out[0] and uv is out[1]
    pitch, rows = W + pad, H + H // 2
    exp = np.full((B * rows * pitch + pitch,), SENTINEL, np.uint8)
    ev = exp[:B * rows * pitch].reshape(B, rows, pitch)
    ev[:, :H, :W] = ry
    ev[:, H:, :W] = ruv.reshape(B, H // 2, W)
    got = flat.cpu().numpy()
    assert np.array_equal(got[-pitch:], exp[-pitch:]), "the row after the last frame was written"
    assert np.array_equal(got, exp)                          # planes equal the reference, every padding byte still the sentinel


def test_default_arguments_are_bt709_limited_and_single_frames_are_accepted():
    shape = (1, 6, 8)
    y, uv = (torch.from_numpy(a.copy()).to(DEV) for a in surface(shape))
    got = ops.nv12_to_tensor(y[0], uv[0])                    # [H][W] and [H/2][W/2][2]
    assert np.array_equal(got.cpu().numpy(), R.nv12_to_tensor(*surface(shape), "bt709", False))
    x = torch.from_numpy(model_output(shape)[0].copy()).to(DEV)
    y2, uv2 = ops.tensor_to_nv12(x[0])
    ry, ruv = R.rgb8_to_nv12(model_output(shape)[1], "bt709", False)
    assert np.array_equal(y2.cpu().numpy(), ry) and np.array_equal(uv2.cpu().numpy(), ruv)


@pytest.mark.parametrize("shape", [(2, 6, 8), (1, 34, 66), (1, 720, 1280)])
def test_decode_is_rgb24_then_to_tensor(shape):
    """The promise of the definition: nv12_to_tensor == frames_to_tensor of the RGB24 conversion, bit for bit."""
    y, uv = surface(shape)
    rgb = torch.from_numpy(R.nv12_to_rgb8(y, uv)).to(DEV)
    got = ops.nv12_to_tensor(torch.from_numpy(y.copy()).to(DEV), torch.from_numpy(uv.copy()).to(DEV))
    assert torch.equal(got, ops.frames_to_tensor(rgb))


def test_invalid_arguments_raise_before_any_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
    bad_decode = {
        "odd H": (u8(1, 5, 8), u8(1, 2, 4, 2)),
        "odd W": (u8(1, 4, 7), u8(1, 2, 3, 2)),
        "uv rows": (u8(1, 4, 8), u8(1, 4, 4, 2)),
        "uv pairs": (u8(1, 4, 8), u8(1, 2, 8, 1)),
        "uv batch": (u8(2, 4, 8), u8(1, 2, 4, 2)),
        "uv rank": (u8(1, 4, 8), u8(2, 8)),
        "float y": (f32(1, 4, 8), u8(1, 2, 4, 2)),
        "int8 uv": (u8(1, 4, 8), u8(1, 2, 4, 2).to(torch.int8)),
        "cpu y": (u8(1, 4, 8).cpu(), u8(1, 2, 4, 2)),
        "cpu uv": (u8(1, 4, 8), u8(1, 2, 4, 2).cpu()),
        "strided y columns": (u8(1, 4, 16)[:, :, ::2], u8(1, 2, 4, 2)),
        "strided uv pairs": (u8(1, 4, 8), u8(1, 2, 8, 2)[:, :, ::2]),
        "transposed y": (u8(1, 8, 4).transpose(1, 2), u8(1, 2, 4, 2)),
    }
    for what, (y, uv) in bad_decode.items():
        with pytest.raises((ValueError, TypeError)):
            ops.nv12_to_tensor(y, uv)
            pytest.fail(f"nv12_to_tensor accepted: {what}")
        if y.dtype == torch.uint8 and uv.dtype == torch.uint8 and y.dim() == 3 and y.shape[1] % 2 == 0 and y.shape[2] % 2 == 0:
            B, H, W = y.shape
            with pytest.raises((ValueError, TypeError)):     # the same planes as an output
                ops.tensor_to_nv12(f32(B, 3, H, W), out=(y, uv))
                pytest.fail(f"tensor_to_nv12 accepted out: {what}")
    bad_encode = {
        "odd H": f32(1, 3, 5, 8), "odd W": f32(1, 3, 4, 7), "two channels": f32(1, 2, 4, 8), "uint8 x": u8(1, 3, 4, 8),
        "cpu x": f32(1, 3, 4, 8).cpu(), "strided x": f32(1, 3, 4, 16)[..., ::2],
    }
    for what, x in bad_encode.items():
        with pytest.raises((ValueError, TypeError)):
            ops.tensor_to_nv12(x)
            pytest.fail(f"tensor_to_nv12 accepted: {what}")
    with pytest.raises(ValueError, match="matrix"):
        ops.nv12_to_tensor(u8(1, 4, 8), u8(1, 2, 4, 2), matrix="bt2020")
    with pytest.raises(ValueError, match="matrix"):
        ops.tensor_to_nv12(f32(1, 3, 4, 8), matrix="rec709")
    with pytest.raises(ValueError):
        ops.nv12_planes(u8(6, 8), 5, 8)
    with pytest.raises(ValueError):
        ops.nv12_planes(u8(5, 8), 4, 8)                      # 3H/2 = 6 rows needed
    with pytest.raises(TypeError):
        ops.nv12_planes(f32(6, 8), 4, 8)
    assert launched == []


def test_c_abi_rejects_bad_geometry_before_any_launch():
    lib = _lib.load()
    inval = 1                                                # hipErrorInvalidValue
    y, uv = (torch.zeros(64, dtype=torch.uint8, device=DEV) for _ in range(2))
    dst = torch.zeros(96, device=DEV)
    args = lambda H, W, yp, up, m=1, fr=0, B=1: (y.data_ptr(), uv.data_ptr(), 64, yp, 64, up, dst.data_ptr(), B, H, W, m, fr, None)
    for H, W, yp, up, m, fr in [(3, 4, 4, 4, 1, 0), (4, 3, 4, 4, 1, 0), (4, 4, 2, 4, 1, 0), (4, 4, 4, 2, 1, 0), (4, 4, 4, 4, 2, 0),
                                (4, 4, 4, 4, -1, 0), (4, 4, 4, 4, 0, 2)]:
        assert lib.tup_nv12_to_f32chw(*args(H, W, yp, up, m, fr)) == inval, (H, W, yp, up, m, fr)
        a = args(H, W, yp, up, m, fr)
        assert lib.tup_f32chw_to_nv12(a[6], a[0], a[1], *a[2:6], *a[7:]) == inval, (H, W, yp, up, m, fr)
    assert lib.tup_nv12_to_f32chw(*args(4, 4, 4, 4, B=65536)) == inval
    assert lib.tup_nv12_to_f32chw(*args(0, 4, 4, 4)) == 0 and lib.tup_nv12_to_f32chw(*args(4, 4, 4, 4, B=0)) == 0
    torch.cuda.synchronize()
    assert (dst == 0).all()


def test_nv12_frame_path_under_hipgraph_replay_equals_eager():
    """NV12 surface -> model -> NV12 planes captured into a hipGraph (frame_speed.py --pixfmt nv12 --graph) replays to exactly the
    eager result, also for a new frame copied into the static buffer (the counterpart of
    tests/test_image_io.py::test_frame_path_under_hipgraph_replay_equals_eager)."""
    import importlib
    from transformerupscaler_amd.weights import deterministic_state_dict
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.cuda().eval()
    H, W = 90, 120
    g = torch.Generator().manual_seed(5)
    f0, f1 = (torch.randint(0, 256, (H + H // 2, W), dtype=torch.uint8, generator=g).to(DEV) for _ in range(2))

    def one(buf):
        return ops.tensor_to_nv12(m(ops.nv12_to_tensor(*ops.nv12_planes(buf, H, W)), res_out=(270, 360)))

    with torch.no_grad():
        eager0, eager1 = [t.clone() for t in one(f0)], [t.clone() for t in one(f1)]
        torch.cuda.synchronize()
        assert eager0[0].shape == (1, 270, 360) and eager0[1].shape == (1, 135, 180, 2)
        assert not torch.equal(eager0[0], eager1[0])
        static_in = f0.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = one(static_in)
        graph.replay(); torch.cuda.synchronize()
        assert torch.equal(static_out[0], eager0[0]) and torch.equal(static_out[1], eager0[1])
        static_in.copy_(f1)
        graph.replay(); torch.cuda.synchronize()
        assert torch.equal(static_out[0], eager1[0]) and torch.equal(static_out[1], eager1[1])


def test_frame_speed_converts_rgb_files_to_nv12_surfaces_once(tmp_path):
    """frame_speed.py --pixfmt nv12 --data_dir: each RGB file becomes one [3H/2][W] surface, Y on top, by tensor_to_nv12 on the GPU."""
    import argparse
    from PIL import Image
    import frame_speed as speed_test
    h, w = speed_test.resolutions["350"]
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    for i, a in enumerate(imgs):
        Image.fromarray(a).save(tmp_path / f"f{i}.png")
    args = argparse.Namespace(data_dir=str(tmp_path), frames=2, res_in="350", source_res=None, matrix="bt601", full_range=True)
    bufs, source = speed_test.load_nv12_frames(args, torch.device(DEV, 0))
    assert source == "files" and len(bufs) == 2
    for buf, a in zip(bufs, imgs):
        ry, ruv = R.rgb8_to_nv12(a[None], "bt601", True)
        got = buf.cpu().numpy()
        assert got.shape == (h + h // 2, w)
        assert np.array_equal(got[:h], ry[0]) and np.array_equal(got[h:], ruv[0].reshape(h // 2, w))
