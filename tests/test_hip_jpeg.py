"""`ops.jpeg_encode` (csrc/jpeg_encode.hip) on the MI355X, byte for byte against the numpy statement tests/_jpeg_ref.py (itself pinned
to Pillow in tests/test_jpeg_cpu.py) and, for a subset, against Pillow directly; and `ops.resize_frames(resample="bicubic")` against
Pillow.  Sizes: 1 x 1; 7 x 13 (less than one MCU); 16 x 16 (exactly one 4:2:0 MCU); 17 x 23 (partial MCUs both ways, odd sizes through
the chroma downsample, luma blocks beyond the image); 33 x 16; 40 x 72 (an even height that is no multiple of 16: the chroma rows
below the image); 16 x 1000: a workgroup codes 96 blocks at a time = 16 MCUs of 4:2:0 or 32 of 4:4:4 = 256 pixels of a row either way,
so a row is four or five chunks with a partial last one and the open byte, the DC predictors and the byte count are carried."""
import functools

import numpy as np
import pytest
import torch

import _jpeg_cases as C
import _jpeg_ref as REF
import _yuv_ref as YUV
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def on_gpu(hw, kind):
    return torch.from_numpy(C.image(hw, kind).copy()).to(DEV)


def encode_one(frame, q, sub, r):
    data, lengths = ops.jpeg_encode(frame, quality=q, subsampling=sub, restart_rows=r)
    assert data.dtype == torch.uint8 and lengths.dtype == torch.int32 and data.shape == (1, int(lengths[0]))      # allocated exactly
    return ops.jpeg_files(data, lengths)[0]


def where(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


@pytest.mark.parametrize("hw", C.SIZES)
def test_files_equal_the_reference(hw):
    assert C.WIDE[1] >= 2 * C.CHUNK_PIXELS and C.WIDE[1] <= 4096 and C.WIDE[0] == 16 and ops.JPEG_CHUNK_BLOCKS == C.CHUNK_BLOCKS
    mine = [c for c in C.cases() if c[0] == hw]
    assert {c[3] for c in mine} == {0, 2} and {c[2] for c in mine} == {5, 75, 100} and {c[4] for c in mine} == {1, 2, 50}
    assert {c[1] for c in mine} >= ({"smooth", "noise"} if hw == C.WIDE else set(C.KINDS))
    for _, kind, q, sub, r in mine:
        want, _ = C.reference(hw, kind, q, sub, r)
        got = encode_one(on_gpu(hw, kind), q, sub, r)
        assert got == want, (hw, kind, q, sub, r, where(got, want))


@pytest.mark.parametrize("hw", ((17, 23), (40, 72), C.WIDE))
def test_files_equal_pillows(hw):
    for kind, q, sub, r in (("smooth", 75, "4:2:0", 1), ("noise", 100, "4:4:4", 2), ("checker", 100, 2, 1), ("smooth", 5, 0, 50)):
        got = encode_one(on_gpu(hw, kind), q, sub, r)
        want = C.pillow(C.image(hw, kind), q, REF.subsampling_code(sub), r)
        assert got == want, (hw, kind, q, sub, r, where(got, want))
    a = C.image(hw, "smooth")                                                       # the defaults are Pillow's: quality 75, 4:2:0
    assert ops.jpeg_files(*ops.jpeg_encode(on_gpu(hw, "smooth")))[0] == C.pillow(a, 75, 2, 1)


def test_a_batch_whose_images_differ():
    hw = (40, 72)
    kinds = ("smooth", "flat255", "noise")
    frames = torch.stack([on_gpu(hw, k) for k in kinds])
    for q, sub, r in ((75, 2, 1), (100, 0, 2)):
        data, lengths = ops.jpeg_encode(frames, quality=q, subsampling=sub, restart_rows=r)
        files = ops.jpeg_files(data, lengths)
        want = [C.reference(hw, k, q, sub, r)[0] for k in kinds]
        assert files == want
        assert len(set(lengths.tolist())) == 3 and data.shape == (3, max(len(w) for w in want))


def test_fp32_input_is_tensor_to_frames_then_the_byte_path():
    """Values off the k / 255 grid and outside [0, 1], NaN and the infinities included: the encoder's own quantisation is
    `tensor_to_frames`' (and tests/_yuv_ref.py's statement of it)."""
    rng = np.random.default_rng(7)
    for hw in ((17, 23), (40, 72)):
        x = (rng.random((2, 3) + hw, dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
        x[0, :, 0, :6] = np.array([np.nan, np.inf, -np.inf, 1.0, 254.999 / 255, 0.5 / 255], dtype=np.float32)
        xg = torch.from_numpy(x).to(DEV)
        frames = ops.tensor_to_frames(xg)
        assert np.array_equal(frames.cpu().numpy(), YUV.quantise(x)) and int(frames.min()) == 0 and int(frames.max()) == 255
        for q, sub, r in ((75, 2, 1), (100, 0, 2), (5, 2, 50)):
            from_f32 = ops.jpeg_files(*ops.jpeg_encode(xg, quality=q, subsampling=sub, restart_rows=r))
            from_u8 = ops.jpeg_files(*ops.jpeg_encode(frames, quality=q, subsampling=sub, restart_rows=r))
            assert from_f32 == from_u8
            assert from_u8[1] == REF.encode(frames[1].cpu().numpy(), q, sub, r)


def test_out_with_room_and_without(monkeypatch):
    hw = (40, 72)
    kinds = ("flat0", "noise", "smooth")
    frames = torch.stack([on_gpu(hw, k) for k in kinds])
    want = [C.reference(hw, k, 75, 2, 1)[0] for k in kinds]
    sizes = [len(w) for w in want]
    assert sizes[0] < sizes[2] < sizes[1]
    guard = 64

    def run(capacity):
        pool = torch.full((3 * capacity + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        lengths = torch.full((3,), 12345, dtype=torch.int32, device=DEV)
        data = pool[:3 * capacity].view(3, capacity)
        got = ops.jpeg_encode(frames, out=(data, lengths))
        assert got[0] is data and got[1] is lengths
        return pool.cpu().numpy(), lengths.cpu().tolist()

    # with room: every file, then the row's remaining bytes as they were
    pool, lengths = run(sizes[1] + 7)
    assert lengths == sizes
    for i, w in enumerate(want):
        row = pool[i * (sizes[1] + 7):(i + 1) * (sizes[1] + 7)]
        assert row[:len(w)].tobytes() == w and (row[len(w):] == 0xA5).all()
    assert (pool[-guard:] == 0xA5).all()
    # the noise image does not fit, to the byte: length -1, its row and what follows it untouched; the others are whole
    capacity = sizes[1] - 1
    pool, lengths = run(capacity)
    assert lengths == [sizes[0], -1, sizes[2]]
    assert (pool[capacity:2 * capacity] == 0xA5).all() and (pool[-guard:] == 0xA5).all()
    assert pool[:sizes[0]].tobytes() == want[0] and pool[2 * capacity:2 * capacity + sizes[2]].tobytes() == want[2]
    assert (pool[sizes[0]:capacity] == 0xA5).all() and (pool[2 * capacity + sizes[2]:3 * capacity] == 0xA5).all()
    # the last image too small by far: nothing of it is written
    capacity = sizes[2] - 300
    assert capacity > sizes[0]
    pool, lengths = run(capacity)
    assert lengths == [sizes[0], -1, -1] and (pool[capacity:] == 0xA5).all()
    with pytest.raises(ValueError, match="image 1 did not fit"):
        ops.jpeg_files(torch.zeros((3, 8), dtype=torch.uint8), torch.tensor(lengths, dtype=torch.int32))
    # out= never synchronises or reads back: no tensor leaves the GPU inside the call
    data = torch.empty((3, sizes[1]), dtype=torch.uint8, device=DEV)
    lengths = torch.empty((3,), dtype=torch.int32, device=DEV)

    def no_readback(*a, **k):
        raise AssertionError("the out= path read a tensor back")
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, no_readback)
    ops.jpeg_encode(frames, out=(data, lengths))
    monkeypatch.undo()
    assert ops.jpeg_files(data, lengths) == want


def test_one_call_is_three_launches(monkeypatch):
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    for frames in (on_gpu((17, 23), "smooth"), torch.stack([on_gpu(C.WIDE, "noise")] * 2), ops.frames_to_tensor(on_gpu((40, 72), "smooth"))):
        del calls[:]
        ops.jpeg_encode(frames)
        assert [c for c in calls if c.startswith("tup_jpeg")] == ["tup_jpeg_sizes", "tup_jpeg_offsets", "tup_jpeg_write"]
        assert len(calls) == 3                                                    # whatever the size of the image or the batch


@pytest.mark.parametrize("size", ((40, 56), (60, 84), (33, 47)))
def test_bicubic_resize_is_pillows(size):
    """x 2, x 3 and a ratio that is no integer, on 20 x 28 frames; uint8 out and the fused ToTensor."""
    from PIL import Image
    rng = np.random.default_rng(28)
    frames = np.stack([C.image((20, 28), "smooth"), rng.integers(0, 256, (20, 28, 3)).astype(np.uint8)])
    want = np.stack([np.asarray(Image.fromarray(f).resize((size[1], size[0]), Image.BICUBIC)) for f in frames])
    g = torch.from_numpy(frames).to(DEV)
    got = ops.resize_frames(g, size, resample="bicubic")
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.resize_frames(g, size, resample="bicubic", to_tensor=True), ops.frames_to_tensor(got))
    bilinear = np.stack([np.asarray(Image.fromarray(f).resize((size[1], size[0]), Image.BILINEAR)) for f in frames])
    assert np.array_equal(ops.resize_frames(g, size).cpu().numpy(), bilinear) and not np.array_equal(bilinear, want)
    assert torch.equal(ops.resize_frames(g, size, resample="bilinear"), ops.resize_frames(g, size))
