"""CPU checks of the baseline JPEG encoder: the numpy statement tests/_jpeg_ref.py against the files Pillow writes, byte
for byte, on inputs asserted to reach the coder's hard cases; `ops.jpeg_header` against the same files; `ops.jpeg_encode`'s validation
ahead of any library call; the `tup_jpeg_*` entries through header / binding / library; and the Pillow-BICUBIC coefficient tables of
`resize_taps.pil_bicubic_coeffs` against what `Image.resize` does to impulses.  Images are synthesised in tests/_jpeg_cases.py."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import _jpeg_cases as C
import _jpeg_ref as REF
from _abi import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference is Pillow's file ----
@pytest.mark.parametrize("hw", C.SIZES)
def test_reference_equals_pillow(hw):
    Image = pytest.importorskip("PIL.Image")
    mine = [c for c in C.cases() if c[0] == hw]
    assert {c[3] for c in mine} == {0, 2} and {c[2] for c in mine} == {5, 75, 100} and {c[4] for c in mine} == {1, 2, 50}
    for _, kind, q, sub, r in mine:
        a = C.image(hw, kind)
        ref, _ = C.reference(hw, kind, q, sub, r)
        pil = C.pillow(a, q, sub, r)
        ref_head, ref_scan = REF.split(ref)
        pil_head, pil_scan = REF.split(pil)
        assert ref_head == pil_head, ("marker segments", hw, kind, q, sub, r)
        assert ref_scan == pil_scan, ("scan", hw, kind, q, sub, r)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(ref)).convert("RGB")), np.asarray(Image.open(io.BytesIO(pil)).convert("RGB"))), \
            ("pixels", hw, kind, q, sub, r)


def test_the_inputs_reach_the_hard_cases():
    """Conditions on the inputs, not on the encoder: each case the coder can get wrong occurs in a file that is compared."""
    all_cases = C.cases()
    stats = {c: C.reference(*c)[1] for c in all_cases if c[0] in ((40, 72), (17, 23))}
    assert any(s.get("stuffed", 0) >= 1 for s in stats.values())                               # a stuffed 0xFF
    assert any(s.get("zrl", 0) >= 1 for s in stats.values())                                   # a run of 16 zeros before a coefficient
    assert any(s.get("eob_after_run", 0) >= 1 for s in stats.values())                         # an EOB after coefficients
    assert any(s["dc_size"] == 11 for c, s in stats.items() if c[2] == 100)                    # the largest DC category, at quality 100
    assert any(s.get("full_blocks", 0) >= 1 for s in stats.values())                           # 63 AC coefficients, no EOB
    for kind in ("flat0", "flat255"):                                                          # no AC coefficient anywhere
        flat = [s for c, s in stats.items() if c[1] == kind]
        assert flat and all(s["dc_only_blocks"] == s["blocks"] for s in flat)
    # the markers the file is said to consist of, in order
    data, _ = C.reference((40, 72), "smooth", 75, 2, 1)
    order, i = [], 2
    while data[i + 1] != 0xDA:
        order.append(data[i + 1])
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    assert data[:2] == b"\xff\xd8" and order == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD] and data[-2:] == b"\xff\xd9"
    assert data.count(b"\xff\xd0") >= 1 and data.count(b"\xff\xd1") >= 1                       # three MCU rows, two restart markers


def test_restart_markers_do_not_change_the_pixels():
    Image = pytest.importorskip("PIL.Image")
    a = C.image((40, 72), "smooth")
    plain = io.BytesIO()
    Image.fromarray(a).save(plain, "JPEG", quality=75)
    want = np.asarray(Image.open(plain).convert("RGB"))
    for r in (1, 2, 50):
        got = np.asarray(Image.open(io.BytesIO(REF.encode(a, 75, 2, r))).convert("RGB"))
        assert np.array_equal(got, want), r


def test_header_is_built_from_the_parameters():
    from transformerupscaler_amd import ops
    for hw, kind, q, sub, r in C.cases()[::7] + [((40, 72), "smooth", 75, 2, 1)]:
        pil_head, _ = REF.split(C.pillow(C.image(hw, kind), q, sub, r))
        assert ops.jpeg_header(hw[0], hw[1], q, sub, r) == pil_head == REF.header(hw[0], hw[1], q, sub, r), (hw, q, sub, r)
    assert ops.jpeg_header(4320, 7680) == REF.header(4320, 7680, 75, 2, 1) and len(ops.jpeg_header(4320, 7680)) < 1000
    assert ops.jpeg_header(8, 8, subsampling="4:4:4") == ops.jpeg_header(8, 8, subsampling=0)
    assert ops.JPEG_ZIGZAG == tuple(REF.ZIGZAG.tolist()) and ops.JPEG_CHUNK_BLOCKS == C.CHUNK_BLOCKS


# ---- the op's host checks ----
def test_jpeg_encode_validates_before_any_library_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("a library call was reached")
    monkeypatch.setattr(_lib, "call", reached)
    monkeypatch.setattr(_lib, "load", reached)
    u = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
    f = torch.zeros((2, 3, 9, 11))
    for s in ("4:2:2", 1, "420", None, True, 2.5):
        with pytest.raises(ValueError, match="subsampling"):
            ops.jpeg_encode(u, subsampling=s)
    for q in (0, 101, -5, 75.0, "75", True):
        with pytest.raises(ValueError, match="quality"):
            ops.jpeg_encode(u, quality=q)
    for r in (0, -1, 1.0, None, False):
        with pytest.raises(ValueError, match="restart_rows"):
            ops.jpeg_encode(u, restart_rows=r)
    with pytest.raises(ValueError, match="restart interval above 65535"):                      # 4096 MCUs a row x 16 rows = 65536
        ops.jpeg_encode(torch.zeros((1, 1, 65535, 3), dtype=torch.uint8), restart_rows=16)
    with pytest.raises(ValueError, match="restart interval above 65535"):
        ops.jpeg_encode(torch.zeros((1, 1, 65535, 3), dtype=torch.uint8), subsampling=0, restart_rows=8)
    with pytest.raises(ValueError, match="1..65535"):
        ops.jpeg_encode(torch.zeros((1, 1, 65536, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="1..65535"):
        ops.jpeg_encode(torch.zeros((1, 0, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="images in one call"):
        ops.jpeg_encode(u[:0])
    for bad in (u[..., :2], u[0, 0], f[:, :2], f[0], torch.zeros((2, 9, 11, 3))):
        with pytest.raises(ValueError, match="frames must be"):
            ops.jpeg_encode(bad)
    for bad in (u.numpy(), f.double(), u.to(torch.int32), None):
        with pytest.raises(TypeError):
            ops.jpeg_encode(bad)
    with pytest.raises(ValueError, match="contiguous"):
        ops.jpeg_encode(u[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ops.jpeg_encode(f[:, :, :, ::2])
    lengths = torch.zeros(2, dtype=torch.int32)
    for out in ((torch.zeros((2, 64)), lengths), (torch.zeros((3, 64), dtype=torch.uint8), lengths), (torch.zeros(128, dtype=torch.uint8), lengths),
                (torch.zeros((2, 128), dtype=torch.uint8)[:, ::2], lengths)):
        with pytest.raises(ValueError, match=r"out\[0\]"):
            ops.jpeg_encode(u, out=out)
    data = torch.zeros((2, 64), dtype=torch.uint8)
    for out in ((data, lengths.long()), (data, torch.zeros(3, dtype=torch.int32)), (data, [0, 0])):
        with pytest.raises(ValueError, match=r"out\[1\]"):
            ops.jpeg_encode(u, out=out)
    for good in (u, f, u[0]):                                                                   # all valid, on the CPU: refused, still no call
        with pytest.raises(ValueError, match="no CPU fallback"):
            ops.jpeg_encode(good)
    with pytest.raises(ValueError, match="resample"):
        ops.resize_frames(u, (4, 4), resample="lanczos")
    with pytest.raises(ValueError, match="did not fit"):
        ops.jpeg_files(torch.zeros((2, 8), dtype=torch.uint8), torch.tensor([4, -1], dtype=torch.int32))
    assert ops.jpeg_files(torch.arange(16, dtype=torch.uint8).view(2, 8), torch.tensor([3, 0], dtype=torch.int32)) == [b"\0\1\2", b""]


# ---- ABI ----
def test_jpeg_entries_are_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())
    for decl in ("int tup_jpeg_segments(int H, int W, int subsampling, int restart_rows);",
                 "int tup_jpeg_sizes(const void* frames_u8, const float* frames_f32, int B, int H, int W, int quality, int subsampling, "
                 "int restart_rows, int* sizes, void* stream);",
                 "int tup_jpeg_offsets(const int* sizes, int B, int S, int header_len, long long capacity, int* offsets, int* lengths, void* stream);",
                 "int tup_jpeg_write(const void* frames_u8, const float* frames_f32, int B, int H, int W, int quality, int subsampling, "
                 "int restart_rows, const void* header, int header_len, const int* offsets, const int* lengths, void* data, long long capacity, "
                 "void* stream);"):
        assert decl in header, decl
    P, I, L = _lib.P, _lib.I, ctypes.c_longlong
    assert _lib.SIGNATURES["tup_jpeg_segments"] == [I, I, I, I]                  # an int count, called through load(), not call()
    assert _lib.SIGNATURES["tup_jpeg_sizes"] == [P, P, I, I, I, I, I, I, P, P]
    assert _lib.SIGNATURES["tup_jpeg_offsets"] == [P, I, I, I, L, P, P, P]
    assert _lib.SIGNATURES["tup_jpeg_write"] == [P, P, I, I, I, I, I, I, P, I, P, P, P, L, P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("tup_jpeg_segments", "tup_jpeg_sizes", "tup_jpeg_offsets", "tup_jpeg_write"))
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("jpeg_encode.hip", ["jpeg_segment_kernel", "jpeg_scan_kernel"])' in guard
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "jpeg_encode.hip")).read()
    assert f"JP_BLOCKS = {C.CHUNK_BLOCKS};" in src and '#include "jpeg_dct.h"' in src
    assert '#include "jpeg_dct.h"' in open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "degrade.hip")).read()
    usage = os.path.join(ROOT, "transformerupscaler_amd", "csrc", "build", "resource_usage.json")
    if os.path.exists(usage):                           # written by the build
        import json
        mine = {k: v for k, v in json.load(open(usage))["kernels"].items() if v["source"] == "jpeg_encode.hip"}
        assert len(mine) == 3 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] for v in mine.values())


def test_entries_refuse_bad_arguments_before_they_launch():
    from transformerupscaler_amd import _lib
    lib = _lib.load()
    seg = lib.tup_jpeg_segments
    assert seg(40, 72, 2, 1) == 3 and seg(40, 72, 0, 1) == 5 and seg(40, 72, 2, 2) == 2 and seg(40, 72, 2, 50) == 1 and seg(1, 1, 0, 1) == 1
    assert seg(4320, 7680, 2, 1) == 270 and seg(65535, 65535, 2, 15) == 274 and seg(65535, 65535, 0, 7) == 1171
    for bad in ((0, 8, 2, 1), (8, 0, 2, 1), (65536, 8, 2, 1), (8, 65536, 0, 1), (8, 8, 1, 1), (8, 8, 3, 1), (8, 8, 2, 0), (1, 65535, 2, 16), (1, 65535, 0, 8)):
        assert seg(*bad) == -1, bad
    invalid = 1                                         # hipErrorInvalidValue
    buf = (ctypes.c_int * 64)()                         # host memory: never dereferenced by a refused call
    a = ctypes.addressof(buf)
    sizes, offsets, write = lib.tup_jpeg_sizes, lib.tup_jpeg_offsets, lib.tup_jpeg_write
    assert sizes(None, None, 1, 8, 8, 75, 2, 1, a, None) == invalid                            # neither input
    assert sizes(a, a, 1, 8, 8, 75, 2, 1, a, None) == invalid    # both
    assert sizes(a, None, 1, 8, 8, 75, 2, 1, None, None) == invalid
    for B, H, W, q, s, r in ((0, 8, 8, 75, 2, 1), (65536, 8, 8, 75, 2, 1), (1, 0, 8, 75, 2, 1), (1, 8, 65536, 75, 2, 1), (1, 8, 8, 0, 2, 1),
                             (1, 8, 8, 101, 2, 1), (1, 8, 8, 75, 1, 1), (1, 8, 8, 75, 2, 0), (1, 8, 65535, 75, 2, 16)):
        assert sizes(a, None, B, H, W, q, s, r, a, None) == invalid, (B, H, W, q, s, r)
        assert write(a, None, B, H, W, q, s, r, a, 600, a, a, a, 4096, None) == invalid, (B, H, W, q, s, r)
    assert offsets(None, 1, 1, 600, 4096, a, a, None) == invalid and offsets(a, 1, 1, 600, 4096, None, a, None) == invalid
    assert offsets(a, 1, 1, 600, 4096, a, None, None) == invalid and offsets(a, 0, 1, 600, 4096, a, a, None) == invalid
    assert offsets(a, 1, 0, 600, 4096, a, a, None) == invalid and offsets(a, 1, 1, -1, 4096, a, a, None) == invalid
    assert offsets(a, 1, 1, 600, -1, a, a, None) == invalid and offsets(a, 1, 1, 600, 2 ** 31, a, a, None) == invalid
    assert write(a, None, 1, 8, 8, 75, 2, 1, None, 600, a, a, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 75, 2, 1, a, 0, a, a, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 75, 2, 1, a, 600, None, a, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 75, 2, 1, a, 600, a, None, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 75, 2, 1, a, 600, a, a, None, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 75, 2, 1, a, 600, a, a, a, 2 ** 31, None) == invalid


# ---- Pillow's BICUBIC tables ----
@pytest.mark.parametrize("pair", ((20, 40), (28, 84), (20, 33), (28, 47), (48, 20), (17, 5)))
def test_bicubic_coefficients_are_pillows(pair):
    """An impulse of 255 at input j resized along one axis gives clip8((255 k[i][j - lo[i]] + 2^21) >> 22) at output i: Pillow's own
    numbers for every coefficient.  (A table value below 1 / 510 rounds away; the sum over all impulses is checked through a ramp.)"""
    Image = pytest.importorskip("PIL.Image")
    from transformerupscaler_amd import resize_taps
    n_in, n_out = pair
    lo, n, k, ksize = resize_taps.pil_bicubic_coeffs(n_in, n_out)
    assert k.shape == (n_out, ksize) and ksize == int(np.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
    assert (k.sum(1) - (1 << 22)).__abs__().max() <= ksize and (k < 0).any()                   # normalised; the negative lobes are there
    assert (lo >= 0).all() and (lo + n <= n_in).all() and (n >= 1).all()
    for j in range(n_in):
        for axis in (0, 1):
            a = np.zeros((3, n_in) if axis else (n_in, 3), np.uint8)
            a[(slice(None), j) if axis else j] = 255
            size = (n_out, 3) if axis else (3, n_out)
            got = np.asarray(Image.fromarray(a).resize(size, Image.BICUBIC)).astype(np.int64)
            line = got[0] if axis else got[:, 0]
            kj = np.array([k[i, j - lo[i]] if lo[i] <= j < lo[i] + n[i] else 0 for i in range(n_out)], dtype=np.int64)
            assert np.array_equal(line, np.clip((255 * kj + (1 << 21)) >> 22, 0, 255)), (pair, j, axis)
    ramp = (np.arange(n_in) * 255 // (n_in - 1)).astype(np.uint8)
    got = np.asarray(Image.fromarray(np.tile(ramp, (3, 1))).resize((n_out, 3), Image.BICUBIC))[0]
    want = [np.clip((int((ramp[lo[i]:lo[i] + n[i]].astype(np.int64) * k[i, :n[i]]).sum()) + (1 << 21)) >> 22, 0, 255) for i in range(n_out)]
    assert got.tolist() == want
    # the bilinear tables are untouched by the shared builder
    blo, bn, bk, bks = resize_taps.pil_bilinear_coeffs(n_in, n_out)
    assert bks == int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1 and (bk >= 0).all()
