"""`ops.png_encode(.., bits=16)` (csrc/png16_encode.hip: the kernels of csrc/png_kernels.h for two-byte samples) on the MI355X, byte for
byte against the Python statement tests/_png16_ref.py (itself opened by Pillow, inflated by zlib and unfiltered independently in
tests/test_png16_cpu.py); fp32 input quantised by q_16 inside the kernels; a batch; the `out=` contract; the 8-bit encoder still equal
to tests/_png_ref.py; and `inference.py --png_bits 16` end to end.  Sizes, contents, block sizes and filters: tests/_png16_cases.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _png16_cases as C
import _png16_ref as REF
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def on_gpu(hw, kind):
    return torch.from_numpy(C.image(hw, kind).copy()).to(DEV)


def encode_one(frame, bb, f):
    data, lengths = ops.png_encode(frame, filter=f, block_bytes=bb, bits=16)
    assert data.dtype == torch.uint8 and lengths.dtype == torch.int32 and data.shape == (1, int(lengths[0]))      # allocated exactly
    return ops.png_files(data, lengths)[0]


def where(got, want):
    k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"{len(got)} bytes against {len(want)}, first difference at {k}"


@pytest.mark.parametrize("hw", C.SIZES)
def test_files_equal_the_reference(hw):
    mine = [c for c in C.cases() if c[0] == hw]
    assert mine and {c[1] for c in mine} == set(C.KINDS) and {c[2] for c in mine} == set(C.BLOCKS) and len({c[3] for c in mine}) >= 5
    for _, kind, bb, f in mine:
        want, _ = C.reference(hw, kind, bb, f)
        got = encode_one(on_gpu(hw, kind), bb, f)
        assert got == want, (hw, kind, bb, f, where(got, want))
        assert len(got) <= ops.png_max_bytes(hw[0], hw[1], bb, bits=16)
    if hw == (40, 72):
        assert ops.png_files(*ops.png_encode(on_gpu(hw, "ramp"), bits=16))[0] == C.reference(hw, "ramp", ops.PNG_BLOCK_BYTES, "adaptive")[0]      # the defaults


def test_fp32_input_is_q16_then_the_sample_path():
    """Values below 0, above 1, at k / 65535 +- 1e-7, the special values of q_16, NaN and the infinities: the encoder's own
    quantisation is tests/_png16_ref.py's q_16 (rounding), and the file is that of the uint16 frame."""
    rng = np.random.default_rng(7)
    s = np.float32(65535)
    for hw in ((3, 5), (40, 72)):
        x = (rng.random((3, 3) + hw, dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
        k = rng.integers(0, 65536, (3,) + hw).astype(np.float32) / s
        x[1] = k + np.float32(1e-7)
        x[2] = k - np.float32(1e-7)
        x[0, 0].reshape(-1)[:11] = np.array([0.0, 1.0, 0.5, 1.0 / 65535, (65535 - 0.001) / 65535, 2.0, -1.0, np.nan, np.inf, -np.inf, 0.5 / 65535],
                                            dtype=np.float32)
        assert (x < 0).any() and (x > 1).any()
        frames = REF.quantise16(x)
        assert frames.dtype == np.uint16 and frames.shape == (3,) + hw + (3,) and frames.min() == 0 and frames.max() == 65535
        assert frames[0].reshape(-1, 3)[:10, 0].tolist() == [0, 65535, 32768, 1, 65535, 65535, 0, 0, 65535, 0]
        xg, fg = torch.from_numpy(x).to(DEV), torch.from_numpy(frames).to(DEV)
        for bb, f in ((256, "adaptive"), (1024, "paeth"), (32768, "average"), (16384, "none")):
            from_f32 = ops.png_files(*ops.png_encode(xg, filter=f, block_bytes=bb, bits=16))
            from_u16 = ops.png_files(*ops.png_encode(fg, filter=f, block_bytes=bb, bits=16))
            want = [REF.encode(frames[b], bb, f) for b in range(3)]
            assert from_u16 == want, [where(g, w) for g, w in zip(from_u16, want)]
            assert from_f32 == want, [where(g, w) for g, w in zip(from_f32, want)]


def test_a_batch_of_three_equals_three_calls():
    hw = (40, 72)
    kinds = ("ramp", "flat65535", "noise")
    frames = torch.stack([on_gpu(hw, k).view(torch.int16) for k in kinds]).view(torch.uint16)
    for bb, f in ((1024, "adaptive"), (256, "paeth"), (32768, "none")):
        data, lengths = ops.png_encode(frames, filter=f, block_bytes=bb, bits=16)
        files = ops.png_files(data, lengths)
        want = [REF.encode(C.image(hw, k), bb, f) for k in kinds]
        assert files == want
        assert files == [encode_one(on_gpu(hw, k), bb, f) for k in kinds]
        assert len(set(lengths.tolist())) == 3 and data.shape == (3, max(len(w) for w in want))


def test_out_with_room_and_without():
    hw = (40, 72)
    kinds = ("flat0", "noise", "ramp")
    bb = 1024
    frames = torch.stack([on_gpu(hw, k).view(torch.int16) for k in kinds]).view(torch.uint16)
    want = [REF.encode(C.image(hw, k), bb, "adaptive") for k in kinds]
    sizes = [len(w) for w in want]
    assert sizes[0] < sizes[2] < sizes[1] == ops.png_max_bytes(hw[0], hw[1], bb, bits=16)    # noise is stored: the bound itself
    guard = 64

    def run(capacity):
        pool = torch.full((3 * capacity + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        lengths = torch.full((3,), 12345, dtype=torch.int32, device=DEV)
        data = pool[:3 * capacity].view(3, capacity)
        got = ops.png_encode(frames, block_bytes=bb, out=(data, lengths), bits=16)
        assert got[0] is data and got[1] is lengths
        return pool.cpu().numpy(), lengths.cpu().tolist()

    # with room, rows starting at each of the four alignments: every file, then the row's bytes as they were
    assert {(sizes[1] + e) % 4 for e in (0, 1, 2, 3)} == {0, 1, 2, 3}
    for extra in (0, 1, 2, 3):
        capacity = sizes[1] + extra
        pool, lengths = run(capacity)
        assert lengths == sizes
        for i, w in enumerate(want):
            row = pool[i * capacity:(i + 1) * capacity]
            assert row[:len(w)].tobytes() == w and (row[len(w):] == 0xA5).all()
        assert (pool[-guard:] == 0xA5).all()
    # the noise image does not fit, by one byte: length -1, its row and what follows it untouched; the others are whole
    capacity = sizes[1] - 1
    pool, lengths = run(capacity)
    assert lengths == [sizes[0], -1, sizes[2]]
    assert (pool[capacity:2 * capacity] == 0xA5).all() and (pool[-guard:] == 0xA5).all()
    assert pool[:sizes[0]].tobytes() == want[0] and pool[2 * capacity:2 * capacity + sizes[2]].tobytes() == want[2]
    assert (pool[sizes[0]:capacity] == 0xA5).all() and (pool[2 * capacity + sizes[2]:3 * capacity] == 0xA5).all()


def test_the_launches_of_one_call_and_the_8_bit_encoder_as_it_was(monkeypatch):
    import _png_cases as C8
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    ops.png_encode(on_gpu((40, 72), "ramp"), bits=16)
    assert calls == ["tup_png16_filters", "tup_png16_sizes", "tup_png16_offsets", "tup_png16_write"]
    del calls[:]
    ops.png_encode(torch.zeros((1, 3, 8, 8), device=DEV), filter="paeth", bits=16)         # a fixed filter skips launch 0
    assert calls == ["tup_png16_sizes", "tup_png16_offsets", "tup_png16_write"]
    del calls[:]
    hw, kind, bb, f = (17, 23), "smooth", 256, "adaptive"                                  # an 8-bit case of tests/_png_cases.py
    frame = torch.from_numpy(C8.image(hw, kind).copy()).to(DEV)
    for kw in ({}, {"bits": 8}):
        assert ops.png_files(*ops.png_encode(frame, filter=f, block_bytes=bb, **kw))[0] == C8.reference(hw, kind, bb, f)[0]
    assert calls == ["tup_png_filters", "tup_png_sizes", "tup_png_offsets", "tup_png_write"] * 2


def test_wrong_dtypes_raise_before_any_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: launched.append(name))
    with pytest.raises(TypeError, match="uint16 or float32"):
        ops.png_encode(torch.zeros((1, 4, 8, 3), dtype=torch.uint8, device=DEV), bits=16)
    with pytest.raises(TypeError, match="uint8 or float32"):
        ops.png_encode(torch.zeros((1, 4, 8, 3), dtype=torch.uint16, device=DEV))
    with pytest.raises(ValueError, match="bits"):
        ops.png_encode(torch.zeros((1, 4, 8, 3), dtype=torch.uint16, device=DEV), bits=10)
    with pytest.raises(ValueError, match="out\\[0\\]"):
        ops.png_encode(torch.zeros((1, 4, 8, 3), dtype=torch.uint16, device=DEV), bits=16,
                       out=(torch.zeros((2, 512), dtype=torch.uint8, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)))
    assert launched == []


def test_inference_writes_a_16_bit_png_end_to_end(tmp_path):
    import importlib
    from PIL import Image
    import _png_cases as C8
    import _yuv_ref as YUV
    import inference
    a = C8.image((64, 80), "smooth")
    src = str(tmp_path / "in.png")
    Image.fromarray(a).save(src)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--image_path", src, "--model", "BicubicInterpolation", "--no-checkpoint",
                        "--scale", "2", "--inp", "i.png", "--out", "y.png", "--png_bits", "16", "--json", "rec.json"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(tmp_path / "rec.json"))
    out, inp = open(tmp_path / "y.png", "rb").read(), open(tmp_path / "i.png", "rb").read()
    assert {k: (v["format"], v["bits"]) for k, v in rec["files"].items()} == {"inp": ("png", 8), "bicubic": ("jpeg", 8), "out": ("png", 16)}
    assert rec["files"]["out"]["bytes"] == len(out) and rec["files"]["inp"]["bytes"] == len(inp)
    assert out[24:26] == b"\x10\x02" and inp[24:26] == b"\x08\x02"                           # IHDR: depth, colour type
    original = torch.from_numpy(a.copy()).to(DEV)
    model = importlib.import_module("models.BicubicInterpolation.model").TransformerModel().to(DEV).eval()
    with torch.no_grad():
        output = inference.forward(model, ops.frames_to_tensor(original), 2).contiguous()
    q16 = REF.quantise16(output.cpu().numpy())[0]
    assert out == REF.encode(q16, ops.PNG_BLOCK_BYTES, "adaptive")
    assert len(np.unique(q16 & 255)) > 64                                                    # the low bytes carry something
    # the scores stay on the 8-bit frame
    out_u8 = ops.tensor_to_frames(output)[0]
    assert np.array_equal(out_u8.cpu().numpy(), YUV.quantise(output.cpu().numpy())[0])
    want = inference.score(original, out_u8, original)
    for name in ("model", "bicubic"):
        for m in ("ssim", "psnr"):
            assert rec["scores"][name][m] == float(want[name][m]), (name, m)
