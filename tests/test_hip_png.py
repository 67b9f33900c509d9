"""`ops.png_encode` (csrc/png_encode.hip) on the MI355X, byte for byte against the Python statement tests/_png_ref.py (itself decoded by
Pillow and zlib in tests/test_png_cpu.py) and, independently of it, through Pillow; the `out=` contract; and `inference.py` writing
PNG files end to end.  Sizes (tests/_png_cases.py): 1 x 1 (a block of four bytes); 17 x 23 at 256 bytes a block (five blocks); 16 x 1000
at 1024 (every row split over three blocks); 3 x 4000 at 32768 (one cut, inside a row); "deep" (the length limit of the Huffman code);
64 x 350 at 256 (263 blocks: two sweeps of the scan kernel)."""
import functools
import io
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import _png_cases as C
import _png_ref as REF
import _yuv_ref as YUV
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def on_gpu(hw, kind):
    return torch.from_numpy(C.image(hw, kind).copy()).to(DEV)


def encode_one(frame, bb, f):
    data, lengths = ops.png_encode(frame, filter=f, block_bytes=bb)
    assert data.dtype == torch.uint8 and lengths.dtype == torch.int32 and data.shape == (1, int(lengths[0]))      # allocated exactly
    return ops.png_files(data, lengths)[0]


def where(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


def pillow_pixels(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Image.open(io.BytesIO(data)).verify()
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("hw", C.SIZES + C.EXTRA)
def test_files_equal_the_reference(hw):
    mine = [c for c in C.cases() if c[0] == hw]
    assert mine and (hw in C.EXTRA or {c[2] for c in mine} >= set(C.BLOCKS))
    for _, kind, bb, f in mine:
        want, _ = C.reference(hw, kind, bb, f)
        got = encode_one(on_gpu(hw, kind), bb, f)
        assert got == want, (hw, kind, bb, f, where(got, want))


@pytest.mark.parametrize("hw", ((1, 1), (17, 23), (40, 72), (16, 1000), (3, 4000)))
def test_pillow_decodes_the_files_to_the_input(hw):
    """Independent of tests/_png_ref.py: what Pillow reads is what went in."""
    for kind, bb, f in (("smooth", 256, "adaptive"), ("noise", 1024, "paeth"), ("flat255", 32768, "adaptive"), ("checker", 1024, "average"),
                        ("smooth", ops.PNG_BLOCK_BYTES, "sub"), ("flat0", 256, "up"), ("checker", 300, "none")):
        got = encode_one(on_gpu(hw, kind), bb, f)
        assert np.array_equal(pillow_pixels(got), C.image(hw, kind)), (hw, kind, bb, f)
        assert len(got) <= ops.png_max_bytes(hw[0], hw[1], bb)
    assert ops.png_files(*ops.png_encode(on_gpu(hw, "smooth")))[0] == C.reference(hw, "smooth", ops.PNG_BLOCK_BYTES, "adaptive")[0]      # the defaults


def test_a_batch_whose_images_differ():
    hw = (40, 72)
    kinds = ("smooth", "flat255", "noise")
    frames = torch.stack([on_gpu(hw, k) for k in kinds])
    for bb, f in ((1024, "adaptive"), (256, "paeth"), (32768, "none")):
        data, lengths = ops.png_encode(frames, filter=f, block_bytes=bb)
        files = ops.png_files(data, lengths)
        want = [C.reference(hw, k, bb, f)[0] for k in kinds]
        assert files == want                                                        # three images in one call = three calls
        assert files == [encode_one(on_gpu(hw, k), bb, f) for k in kinds]
        assert len(set(lengths.tolist())) == 3 and data.shape == (3, max(len(w) for w in want))


def test_fp32_input_is_tensor_to_frames_then_the_byte_path():
    """Values below 0, above 1, at k / 255 +- 1e-7, NaN and the infinities: the encoder's own quantisation is `tensor_to_frames`' (and
    tests/_yuv_ref.py's statement of it)."""
    rng = np.random.default_rng(7)
    for hw in ((17, 23), (40, 72)):
        x = (rng.random((3, 3) + hw, dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
        k = rng.integers(0, 256, (3,) + hw).astype(np.float32) / np.float32(255)
        x[1] = k + np.float32(1e-7)
        x[2] = k - np.float32(1e-7)
        x[0, :, 0, :6] = np.array([np.nan, np.inf, -np.inf, 1.0, 254.999 / 255, 0.5 / 255], dtype=np.float32)
        assert (x < 0).any() and (x > 1).any()
        xg = torch.from_numpy(x).to(DEV)
        frames = ops.tensor_to_frames(xg)
        assert np.array_equal(frames.cpu().numpy(), YUV.quantise(x)) and int(frames.min()) == 0 and int(frames.max()) == 255
        for bb, f in ((256, "adaptive"), (1024, "paeth"), (32768, "average"), (512, "none")):
            from_f32 = ops.png_files(*ops.png_encode(xg, filter=f, block_bytes=bb))
            from_u8 = ops.png_files(*ops.png_encode(frames, filter=f, block_bytes=bb))
            assert from_f32 == from_u8
            for b in range(3):
                assert from_u8[b] == REF.encode(frames[b].cpu().numpy(), bb, f)


def test_out_with_room_and_without(monkeypatch):
    hw = (40, 72)
    kinds = ("flat0", "noise", "smooth")
    bb = 1024
    frames = torch.stack([on_gpu(hw, k) for k in kinds])
    want = [C.reference(hw, k, bb, "adaptive")[0] for k in kinds]
    sizes = [len(w) for w in want]
    assert sizes[0] < sizes[2] < sizes[1] == ops.png_max_bytes(hw[0], hw[1], bb)    # noise is stored: the bound itself
    guard = 64

    def run(capacity):
        pool = torch.full((3 * capacity + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        lengths = torch.full((3,), 12345, dtype=torch.int32, device=DEV)
        data = pool[:3 * capacity].view(3, capacity)
        got = ops.png_encode(frames, block_bytes=bb, out=(data, lengths))
        assert got[0] is data and got[1] is lengths
        return pool.cpu().numpy(), lengths.cpu().tolist()

    # with room (rows of an odd length, so that chunks start at every alignment): every file, then the row's bytes as they were
    for extra in (7, 0, 1, 2):
        capacity = sizes[1] + extra
        pool, lengths = run(capacity)
        assert lengths == sizes == ops.png_encode(frames, block_bytes=bb)[1].tolist()
        for i, w in enumerate(want):
            row = pool[i * capacity:(i + 1) * capacity]
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
        ops.png_files(torch.zeros((3, 8), dtype=torch.uint8), torch.tensor(lengths, dtype=torch.int32))
    # out= never synchronises or reads back: no tensor leaves the GPU inside the call
    data = torch.empty((3, ops.png_max_bytes(hw[0], hw[1], bb)), dtype=torch.uint8, device=DEV)
    lengths = torch.empty((3,), dtype=torch.int32, device=DEV)

    def no_readback(*a, **k):
        raise AssertionError("the out= path read a tensor back")
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, no_readback)
    ops.png_encode(frames, block_bytes=bb, out=(data, lengths))
    monkeypatch.undo()
    assert ops.png_files(data, lengths) == want


def test_the_launches_of_one_call(monkeypatch):
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    for frames in (on_gpu((17, 23), "smooth"), torch.stack([on_gpu((16, 1000), "noise")] * 2), ops.frames_to_tensor(on_gpu((40, 72), "smooth"))):
        del calls[:]
        ops.png_encode(frames)
        assert calls == ["tup_png_filters", "tup_png_sizes", "tup_png_offsets", "tup_png_write"]
        del calls[:]
        ops.png_encode(frames, filter="paeth")                                     # a fixed filter skips launch 0
        assert calls == ["tup_png_sizes", "tup_png_offsets", "tup_png_write"]


def test_inference_writes_png_files_end_to_end(tmp_path):
    from PIL import Image
    from transformerupscaler_amd import metrics
    import inference
    hw = (64, 80)
    a = C.image(hw, "smooth")
    src = str(tmp_path / "in.png")
    Image.fromarray(a).save(src)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--image_path", src, "--model", "BicubicInterpolation", "--no-checkpoint",
                        "--scale", "2", "--inp", "i.png", "--out", "o.png", "--json", "rec.json"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(tmp_path / "rec.json"))
    files = {k: open(tmp_path / n, "rb").read() for k, n in (("inp", "i.png"), ("bicubic", "bicubic.jpg"), ("out", "o.png"))}
    assert files["inp"][:8] == REF.SIGNATURE and files["out"][:8] == REF.SIGNATURE and files["bicubic"][:3] == b"\xff\xd8\xff"
    assert {k: v["format"] for k, v in rec["files"].items()} == {"inp": "png", "bicubic": "jpeg", "out": "png"}
    assert all(rec["files"][k]["bytes"] == len(v) for k, v in files.items())
    # the same steps here: no res_in, so the low-resolution input is the image itself
    original = torch.from_numpy(a.copy()).to(DEV)
    assert np.array_equal(pillow_pixels(files["inp"]), a)
    import importlib
    model = importlib.import_module("models.BicubicInterpolation.model").TransformerModel().to(DEV).eval()
    with torch.no_grad():
        output = inference.forward(model, ops.frames_to_tensor(original), 2)
    out_u8 = ops.tensor_to_frames(output.contiguous())[0]
    assert np.array_equal(out_u8.cpu().numpy(), YUV.quantise(output.cpu().numpy())[0])      # trunc(clamp(255 x, 0, 255))
    assert np.array_equal(pillow_pixels(files["out"]), out_u8.cpu().numpy())
    assert files["out"] == REF.encode(out_u8.cpu().numpy(), ops.PNG_BLOCK_BYTES, "adaptive")
    want = inference.score(original, out_u8, original)
    for name in ("model", "bicubic"):
        for m in ("ssim", "psnr"):
            assert rec["scores"][name][m] == float(want[name][m]), (name, m)
    big = ops.resize_frames(original, tuple(out_u8.shape[:2]))[0]
    q = metrics.quality(big.contiguous(), out_u8.contiguous())
    assert rec["scores"]["model"]["ssim"] == float(q["ssim"][0]) and rec["scores"]["model"]["psnr"] == float(q["psnr"][0])
