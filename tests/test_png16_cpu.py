"""The Python statement of the 16-bit PNG file (tests/_png16_ref.py) checked on its own: Pillow opens every case, a chunk
walker checks IHDR and every CRC, zlib inflates the joined IDATs to the filtered stream, an independent numpy unfilter gives the 16-bit
samples back, no block is longer than its stored form; then q_16, `ops.png_encode(.., bits=16)`'s validation ahead of any library call,
the `tup_png16_*` entries through header / binding / library, and inference.py's `--png_bits`.  No GPU."""
import io
import os
import re
import struct
import warnings
import zlib

import numpy as np
import pytest
import torch

import _png16_cases as C
import _png16_ref as REF
import _png_ref as REF8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walk(data):
    """[(type, payload)] of a PNG file, every length and CRC checked"""
    assert data[:8] == REF8.SIGNATURE
    out, i = [], 8
    while i < len(data):
        n, kind = struct.unpack(">I4s", data[i:i + 8])
        payload = data[i + 8:i + 8 + n]
        assert len(payload) == n
        assert struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(kind + payload), (kind, i)
        out.append((kind, payload))
        i += 12 + n
    assert i == len(data)
    return out


def unfilter(stream, h, w):
    """The PNG specification's reconstruction on bytes with bpp = 6, written without the reference's filter code: uint16 [h][w][3]."""
    n = 6 * w
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + n)
    out = np.zeros((h, n), np.int32)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        prev = out[y - 1] if y else np.zeros(n, np.int32)
        for x in range(n):
            a = out[y, x - 6] if x >= 6 else 0
            b = prev[x]
            c = prev[x - 6] if x >= 6 else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) // 2
            else:
                assert ft == 4
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[y, x] = (line[x] + p) & 255
    return (out[:, 0::2] * 256 + out[:, 1::2]).astype(np.uint16).reshape(h, w, 3)


def pillow_view(data):
    """What Pillow makes of a 16-bit RGB file: mode RGB, every sample's high byte; opened and verified with warnings as errors."""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Image.open(io.BytesIO(data)).verify()
        with Image.open(io.BytesIO(data)) as im:
            assert im.mode == "RGB"
            return np.asarray(im)


SLOW_UNFILTER = 40 * 72 * 6           # the per-byte Python unfilter runs up to this many bytes a case


@pytest.mark.parametrize("hw", C.SIZES)
def test_files_are_valid_16_bit_png(hw):
    mine = [c for c in C.cases() if c[0] == hw]
    assert mine and {c[1] for c in mine} == set(C.KINDS) and {c[2] for c in mine} == set(C.BLOCKS) and len({c[3] for c in mine}) >= 5
    h, w = hw
    unfiltered = 0
    for _, kind, bb, f in mine:
        img = C.image(hw, kind)
        data, stats = C.reference(hw, kind, bb, f)
        assert np.array_equal(pillow_view(data), (img >> 8).astype(np.uint8)), (kind, bb, f)
        chunks = walk(data)
        assert chunks[0] == (b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) and chunks[-1] == (b"IEND", b"")
        idat = [p for k, p in chunks[1:-1]]
        assert all(k == b"IDAT" for k, _ in chunks[1:-1]) and len(idat) == REF.blocks(h, w, bb) + 1 and len(idat[-1]) == 4
        stream = REF.filtered(img, f)
        assert len(stream) == h * (1 + 6 * w)
        assert zlib.decompress(b"".join(idat)) == stream                            # header, every block, the Adler-32
        types = np.frombuffer(stream, np.uint8).reshape(h, 1 + 6 * w)[:, 0]
        assert (types == REF.FILTERS[f]).all() if f != "adaptive" else (types <= 4).all()
        # no block is longer than its stored form (5 + n, + 4 bytes of IDAT framing each, + the zlib header on the first)
        for i, p in enumerate(idat[:-1]):
            n = min(bb, len(stream) - i * bb)
            assert len(p) <= 5 + n + (2 if i == 0 else 0), (kind, bb, f, i)
        assert len(data) <= REF.file_bound(h, w, bb)
        assert len(stats["forms"]) == REF.blocks(h, w, bb)
        if h * w * 6 <= SLOW_UNFILTER and (unfiltered < 6 or hw != (40, 72)):
            assert np.array_equal(unfilter(stream, h, w), img), (kind, bb, f)
            unfiltered += 1
    assert unfiltered >= min(6, len(mine)) or hw == C.BIG


def test_unfilter_of_the_big_image_by_rows():
    """The per-byte unfilter is too slow for 64 x 683; its "sub" and "up" cases are undone with numpy here: cumulative sums modulo 256
    over the six byte lanes of a row / down the rows."""
    hw, (h, w) = C.BIG, C.BIG
    for kind, f in (("lowbyte", "sub"), ("flat65535", "up")):
        img = C.image(hw, kind)
        rows = np.frombuffer(REF.filtered(img, f), np.uint8).reshape(h, 1 + 6 * w)[:, 1:].astype(np.int64)
        if f == "sub":
            raw = np.cumsum(rows.reshape(h, w, 6), axis=1).reshape(h, 6 * w) & 255
        else:
            raw = np.cumsum(rows, axis=0) & 255
        assert np.array_equal((raw[:, 0::2] * 256 + raw[:, 1::2]).astype(np.uint16).reshape(h, w, 3), img)


def test_noise_is_stored_and_reaches_the_bound_and_flat_images_are_tiny():
    data, stats = C.reference((40, 72), "noise", 256, "none")
    assert set(stats["forms"]) == {"stored"} and len(data) == REF.file_bound(40, 72, 256)
    data, stats = C.reference(C.BIG, "flat0", 32768, "average")
    assert "stored" not in stats["forms"] and len(data) < 1024


def test_low_bytes_are_in_the_file_big_endian():
    """A frame whose samples differ only in the low byte: Pillow's view is flat, the inflated stream is not, and byte order matters."""
    img = C.image((3, 5), "lowbyte")
    data, _ = C.reference((3, 5), "lowbyte", 256, "none")
    assert (pillow_view(data) == 0x80).all()
    raw = np.frombuffer(zlib.decompress(b"".join(p for k, p in walk(data) if k == b"IDAT")), np.uint8).reshape(3, 31)[:, 1:]
    assert (raw[:, 0::2] == 0x80).all() and np.array_equal(raw[:, 1::2].reshape(3, 5, 3), (img & 255).astype(np.uint8))
    assert len(np.unique(raw[:, 1::2])) > 8
    assert np.array_equal(REF.row_bytes(np.array([[[0x0102, 0xA0B0, 0x00FF]]], np.uint16)), [[1, 2, 0xA0, 0xB0, 0, 0xFF]])


def test_the_8_bit_reference_is_what_it_was():
    """tests/_png16_ref.py borrows _png_ref's deflate pieces and changes none: one 8-bit case, still Pillow's pixels."""
    import _png_cases as C8
    from PIL import Image
    data, _ = C8.reference((17, 23), "smooth", 256, "adaptive")
    assert walk(data)[0][1][8:10] == b"\x08\x02"
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), C8.image((17, 23), "smooth"))


def test_q16_special_values_and_facts():
    s = 65535
    x = np.array([0.0, 1.0, 0.5, 1.0 / s, (s - 0.001) / s, 2.0, -1.0, np.nan, np.inf, -np.inf, 0.25, 0.1], np.float32).reshape(3, 2, 2)
    q = REF.quantise16(x)
    assert q.dtype == np.uint16 and q.shape == (2, 2, 3)
    assert np.moveaxis(q, -1, 0).reshape(-1).tolist() == [0, s, 32768, 1, s, s, 0, 0, s, 0, 16384, 6554]
    p = np.arange(65536, dtype=np.int64)
    assert np.array_equal(REF.quantise16((p.astype(np.float32) / np.float32(s)).reshape(1, 256, 256))[..., 0].reshape(-1), p)
    v = np.arange(256)
    assert np.array_equal(REF.quantise16((v.astype(np.float32) / np.float32(255)).reshape(1, 16, 16))[..., 0].reshape(-1), 257 * v)
    b = REF.quantise16(np.zeros((2, 3, 4, 5), np.float32))
    assert b.shape == (2, 4, 5, 3)


# ---- ops: validation before any library call ----
def test_png_encode_bits_is_validated_before_any_library_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    monkeypatch.setattr(_lib, "load", reached)
    u16 = torch.zeros((1, 4, 8, 3), dtype=torch.uint16)
    f32 = torch.zeros((1, 3, 4, 8))
    for bad in (0, 10, 12, 32, "16", None, True, 16.5):
        with pytest.raises(ValueError, match="bits must be 8 or 16"):
            ops.png_encode(u16, bits=bad)
        with pytest.raises(ValueError, match="bits must be 8 or 16"):
            ops.png_max_bytes(4, 8, bits=bad)
    with pytest.raises(TypeError, match="uint16 or float32"):
        ops.png_encode(torch.zeros((1, 4, 8, 3), dtype=torch.uint8), bits=16)      # no silent widening of bytes
    with pytest.raises(TypeError, match="uint8 or float32"):
        ops.png_encode(u16)                                                        # ... and no silent narrowing
    with pytest.raises(TypeError):
        ops.png_encode(u16.view(torch.int16), bits=16)
    for bad in (torch.zeros((4, 8, 4), dtype=torch.uint16), torch.zeros((1, 4, 8), dtype=torch.uint16).unsqueeze(0), torch.zeros((3, 4, 8))):
        with pytest.raises(ValueError, match=r"must be \["):
            ops.png_encode(bad, bits=16)
    with pytest.raises(ValueError, match="contiguous"):
        ops.png_encode(torch.zeros((1, 4, 16, 3), dtype=torch.uint16)[:, :, ::2], bits=16)
    with pytest.raises(ValueError, match="filter"):
        ops.png_encode(u16, bits=16, filter="best")
    with pytest.raises(ValueError, match="block_bytes"):
        ops.png_encode(u16, bits=16, block_bytes=100)
    with pytest.raises(ValueError, match="lives on cpu"):
        ops.png_encode(u16, bits=16)
    with pytest.raises(ValueError, match="lives on cpu"):
        ops.png_encode(f32, bits=16)
    # the stream of a 16-bit file is H (1 + 6 W) bytes: the 2^31 limit comes at half the width
    assert ops.png_max_bytes(1, 178956970) > 0
    with pytest.raises(ValueError, match="below 2\\^31"):
        ops.png_max_bytes(2, 178956971, bits=16)
    for h, w, bb in ((1, 1, 256), (40, 72, 256), (40, 72, 16384), (64, 683, 32768), (3, 5, 1024)):
        assert ops.png_max_bytes(h, w, bb, bits=16) == REF.file_bound(h, w, bb)
        assert ops.png_max_bytes(h, w, bb, bits=8) == ops.png_max_bytes(h, w, bb) == REF8.file_bound(h, w, bb)
    assert ops.png_max_bytes(40, 72, bits=16) == REF.file_bound(40, 72, ops.PNG_BLOCK_BYTES)


# ---- ABI ----
def test_png16_entries_are_declared_bound_and_exported():
    import ctypes
    import _abi
    from transformerupscaler_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())
    for decl in ("int tup_png16_blocks(int H, int W, int block_bytes);",
                 "int tup_png16_filters(const void* frames_u16, const float* frames_f32, int B, int H, int W, void* filters, void* stream);",
                 "int tup_png16_sizes(const void* frames_u16, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, "
                 "const void* filters, int* sizes, int* partials, void* stream);",
                 "int tup_png16_offsets(const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, "
                 "int* offsets, int* lengths, int* adlers, void* stream);",
                 "int tup_png16_write(const void* frames_u16, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, "
                 "const void* filters, const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity, void* stream);"):
        assert decl in header, decl
    for name in ("blocks", "filters", "sizes", "offsets", "write"):                # argument for argument the 8-bit entry
        assert _lib.SIGNATURES["tup_png16_" + name] == _lib.SIGNATURES["tup_png_" + name]
    assert _lib.SIGNATURES["tup_png16_offsets"][6] is ctypes.c_longlong
    assert _lib.ABI_VERSION == _abi.ABI == 16                              # entries were added: the number stays
    lib = _lib.load()
    assert all(hasattr(lib, "tup_png16_" + n) for n in ("blocks", "filters", "sizes", "offsets", "write"))
    import importlib.util
    import json
    csrc = os.path.join(ROOT, "transformerupscaler_amd", "csrc")
    spec = importlib.util.spec_from_file_location("check_resources", os.path.join(csrc, "check_resources.py"))
    guard = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(guard)
    guarded = {fn for src, fns in guard.GUARDED if src == "png16_encode.hip" for fn in fns}
    assert guarded == {"png_filter_kernel", "png_block_kernel"}
    usage = os.path.join(csrc, "build", "resource_usage.json")                     # written by the build that made the library loaded above
    assert os.path.exists(usage), "the build leaves build/resource_usage.json beside the objects"
    mine = {k: v for k, v in json.load(open(usage))["kernels"].items() if v["source"] == "png16_encode.hip"}
    assert len(mine) == 3 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] for v in mine.values())


def test_png16_entries_refuse_bad_arguments_before_they_launch():
    from transformerupscaler_amd import _lib
    lib = _lib.load()
    invalid = 1                                                                    # hipErrorInvalidValue
    blocks = lib.tup_png16_blocks
    assert blocks(1, 1, 256) == 1 and blocks(40, 72, 256) == 68 and blocks(40, 72, 16384) == 2 and blocks(64, 683, 256) == 1025
    assert blocks(40, 72, 256) == REF.blocks(40, 72, 256) and lib.tup_png_blocks(40, 72, 256) == REF8.blocks(40, 72, 256) == 34
    for h, w, bb in ((0, 8, 256), (8, 0, 256), (8, 8, 255), (8, 8, 32769), (2, 178956971, 256), (1, 357913942, 256)):
        assert blocks(h, w, bb) == -1, (h, w, bb)
    assert blocks(1, 357913941, 32768) == 65536                                 # 1 + 6 W = 2^31 - 1
    a = 1 << 12                                                                    # any non-null even address: nothing is dereferenced before the checks fail
    filters, sizes, offsets, write = lib.tup_png16_filters, lib.tup_png16_sizes, lib.tup_png16_offsets, lib.tup_png16_write
    assert filters(None, None, 1, 8, 8, a, None) == invalid and filters(a, a, 1, 8, 8, a, None) == invalid      # neither / both inputs
    assert filters(a, None, 0, 8, 8, a, None) == invalid and filters(a, None, 65536, 8, 8, a, None) == invalid
    assert filters(a, None, 1, 8, 8, None, None) == invalid and filters(a, None, 1, 0, 8, a, None) == invalid
    assert filters(a + 1, None, 1, 8, 8, a, None) == invalid                       # uint16 frames at an odd address
    assert sizes(a, None, 1, 8, 8, 6, 256, a, a, a, None) == invalid and sizes(a, None, 1, 8, 8, -1, 256, a, a, a, None) == invalid
    assert sizes(a, None, 1, 8, 8, 5, 256, None, a, a, None) == invalid            # adaptive without the row filters
    assert sizes(a, None, 1, 8, 8, 0, 100, None, a, a, None) == invalid and sizes(a, None, 1, 8, 8, 0, 256, None, None, a, None) == invalid
    assert sizes(a + 1, None, 1, 8, 8, 0, 256, None, a, a, None) == invalid
    assert offsets(a, a, 1, 8, 8, 256, -1, a, a, a, None) == invalid and offsets(a, a, 1, 8, 8, 256, 2 ** 31, a, a, a, None) == invalid
    assert offsets(None, a, 1, 8, 8, 256, 4096, a, a, a, None) == invalid and offsets(a, a, 0, 8, 8, 256, 4096, a, a, a, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, a, a, None, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, a, a, a, 2 ** 31, None) == invalid
    assert write(a, None, 1, 8, 8, 5, 256, None, a, a, a, a, 4096, None) == invalid
    assert write(a + 1, None, 1, 8, 8, 0, 256, None, a, a, a, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, a, a, None, 0, None) == 0      # capacity 0: nothing fits, nothing to do


# ---- inference.py: --png_bits ----
def test_inference_png_bits_dispatch(monkeypatch, tmp_path, capsys):
    import inference
    from transformerupscaler_amd import metrics, ops
    parse = inference.parse_args                                                   # what main() parses with: build_parser() + --png_bits
    assert parse([]).png_bits == 8 and parse(["--png_bits", "16"]).png_bits == 16 and parse(["--png_bits", "8"]).png_bits == 8
    assert {k: v for k, v in vars(parse([])).items() if k != "png_bits"} == vars(inference.build_parser().parse_args([]))
    for bad in (["--png_bits", "10"], ["--png_bits", "sixteen"], ["--png_bits"]):
        with pytest.raises(SystemExit):
            parse(bad)
    with pytest.raises(SystemExit):
        parse(["--help"])
    assert "--png_bits" in capsys.readouterr().out

    calls = []
    monkeypatch.setattr(ops, "jpeg_encode", lambda frames, **kw: calls.append(("jpeg", frames.dtype, kw)) or ("jpeg", frames))
    monkeypatch.setattr(ops, "png_encode", lambda frames, **kw: calls.append(("png", frames.dtype, kw)) or ("png", frames))
    monkeypatch.setattr(ops, "jpeg_files", lambda kind, frames: [b"JPEG" + bytes(3)])
    monkeypatch.setattr(ops, "png_files", lambda kind, frames: [b"\x89PNG" + bytes(5)])
    monkeypatch.setattr(ops, "resize_frames", lambda x, size, resample="bilinear": torch.zeros((1,) + tuple(size) + (3,), dtype=torch.uint8) + 3)
    monkeypatch.setattr(ops, "frames_to_tensor", lambda x: x.unsqueeze(0).permute(0, 3, 1, 2).float() / 255)
    monkeypatch.setattr(ops, "tensor_to_frames", lambda x: (x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    scored = []
    monkeypatch.setattr(metrics, "quality", lambda a, b: scored.append(b.clone()) or {"ssim": torch.tensor([0.5]), "psnr": torch.tensor([20.0])})
    original = torch.arange(6 * 8 * 3, dtype=torch.uint8).reshape(6, 8, 3)
    monkeypatch.setattr(inference, "decode_image", lambda src, device, gpu=True:
                        torch.full((12, 16, 3), 99, dtype=torch.uint8) if isinstance(src, (bytes, bytearray)) else original)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    monkeypatch.chdir(tmp_path)

    class Model(torch.nn.Module):
        def forward(self, x, upscale_factor=2):
            return torch.full((1, 3, 12, 16), 0.5)
    import models.BicubicInterpolation.model as plugin
    monkeypatch.setattr(plugin, "TransformerModel", Model)

    def run(inp, out, *more):
        del calls[:], scored[:]
        return inference.run(parse(["--image_path", "x.png", "--model", "BicubicInterpolation", "--no-checkpoint", "--scale", "2",
                                           "--inp", inp, "--out", out, *more]), device="cpu")

    rec = run("i.png", "o.PNG", "--png_bits", "16")
    # only --out, made from the fp32 output, is a 16-bit file; --inp stays an 8-bit PNG from uint8, bicubic.jpg a JPEG
    assert [(c[0], c[1]) for c in calls] == [("png", torch.uint8), ("jpeg", torch.uint8), ("png", torch.float32)]
    assert calls[0][2] == {} and calls[2][2] == {"bits": 16}
    assert {k: (v["format"], v["bits"]) for k, v in rec["files"].items()} == {"inp": ("png", 8), "bicubic": ("jpeg", 8), "out": ("png", 16)}
    assert (scored[0] == 127).all() and scored[0].dtype == torch.uint8            # the score stays on the 8-bit frame: trunc(0.5 * 255)
    rec = run("i.png", "o.png")                                                    # the default is 8
    assert calls[2][2] == {} and rec["files"]["out"]["bits"] == 8
    rec = run("i.png", "o.png", "--png_bits", "8")
    assert calls[2][2] == {} and rec["files"]["out"]["bits"] == 8
    rec = run("i.png", "o.jpg", "--png_bits", "16")                                # not a .png: the flag does not apply
    assert [c[0] for c in calls] == ["png", "jpeg", "jpeg"] and "bits" not in calls[2][2] and rec["files"]["out"]["bits"] == 8
