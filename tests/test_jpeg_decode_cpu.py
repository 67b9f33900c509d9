"""The baseline JPEG decoder without a GPU: tests/_jpeg_decode_ref.py (the numpy statement of `ops.jpeg_decode`) against Pillow pixel
for pixel, what its walker's inputs reach, `ops.jpeg_parse` and its refusals, `ops.jpeg_decode`'s validation, the C ABI, and damaged
scans through csrc/jpeg_entropy.h on the host under the address and undefined-behaviour sanitizers."""
import ctypes
import glob
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _degrade_ref as D  # noqa: E402
import _jpeg_cases as C  # noqa: E402
import _jpeg_decode_cases as DC  # noqa: E402
import _jpeg_decode_ref as R  # noqa: E402
import _jpeg_ref as REF  # noqa: E402
from _abi import ABI  # noqa: E402


# ---- the reference against Pillow ----
def test_reference_equals_pillow_on_every_case_with_and_without_restarts():
    from transformerupscaler_amd import ops
    stats, n = {}, 0
    for hw, kind, q, sub, r in C.cases():
        for rr in (r, 0):
            f = C.pillow(C.image(hw, kind), q, sub, rr)
            got, status = R.decode(f, stats)
            assert status == 0 and np.array_equal(got, DC.pillow_pixels(f)), (hw, kind, q, sub, rr, status)
            assert ops.jpeg_parse(f) == R.parse(f)
            n += 1
    assert n == 2 * len(C.cases()) == 318
    # what the walker met on the way (the contents were chosen for the encoder's sake; asserted, not assumed)
    assert stats["stuffed"] > 0 and stats["zrl"] > 0 and stats["eob_after_run"] > 0 and stats["full_blocks"] > 0 and stats["dc_size"] == 11


def test_walker_coverage_per_content():
    for kind, key in (("noise", "stuffed"), ("noise", "full_blocks"), ("smooth", "zrl"), ("smooth", "eob_after_run")):
        stats = {}
        for q in (5, 75, 100):
            for sub in (0, 2):
                assert R.decode(C.pillow(C.image((40, 72), kind), q, sub, 1), stats)[1] == 0
        assert stats.get(key, 0) > 0, (kind, key, stats)
    stats = {}
    assert R.decode(C.pillow(C.image((40, 72), "checker"), 100, 0, 1), stats)[1] == 0
    assert stats["dc_size"] == 11
    for kind in ("flat0", "flat255"):                                   # an all-EOB image: every block ends at its first AC symbol
        stats = {}
        assert R.decode(C.pillow(C.image((40, 72), kind), 75, 2, 1), stats)[1] == 0
        assert stats["eob_first"] == stats["blocks"] == 3 * 5 * 6 and "zrl" not in stats and "eob_after_run" not in stats


@pytest.mark.parametrize("name,data", DC.extra_files(), ids=[n for n, _ in DC.extra_files()])
def test_reference_equals_pillow_on_other_files(name, data):
    from transformerupscaler_amd import ops
    got, status = R.decode(data)
    assert status == 0 and np.array_equal(got, DC.pillow_pixels(data))
    info = ops.jpeg_parse(data)
    assert info == R.parse(data)
    if name.startswith("blocks"):
        m = 16 if info["subsampling"] == "4:2:0" else 8
        assert info["restart_interval"] == int(name[6])
        if name != "blocks5-40x72-2":                                   # 5 MCUs are a whole row of that one; the others begin segments mid-row
            assert info["restart_interval"] % ((info["W"] + m - 1) // m) != 0
    if name.startswith("optimize"):
        assert info["huffman_tables"][(1, 0)] != (tuple(REF.AC_LUMA[0]), tuple(REF.AC_LUMA[1]))
    if name.startswith("grey"):
        assert info["components"] == 1 and info["subsampling"] == "grey" and (got[..., 0] == got[..., 1]).all()
    if name == "exif-com":
        assert b"Exif\0\0" in data and b"\xff\xfe" in data and b"a comment" in data
    if name == "dqt-merged":
        assert data.count(b"\xff\xdb") == 1 and len(info["quant_tables"]) == 2


# ---- cross-checks ----
def test_decode_of_the_reference_encoder_is_the_degrade_round_trip():
    for hw, kind, q in (((17, 23), "smooth", 75), ((40, 72), "noise", 5), ((33, 16), "checker", 100)):
        u = C.image(hw, kind)
        got, status = R.decode(REF.encode(u, q, "4:4:4"))
        want = D.jpeg_roundtrip(np.asarray(u).astype(np.int64).transpose(2, 0, 1), q)            # [3][H][W]
        assert status == 0 and np.array_equal(got, np.asarray(want).transpose(1, 2, 0).astype(np.uint8))


def test_parse_recovers_what_jpeg_header_was_built_from():
    from transformerupscaler_amd import ops
    for H, W, q, sub, rows in ((40, 72, 75, "4:2:0", 1), (17, 23, 5, "4:4:4", 2), (2160, 3840, 100, "4:2:0", 1)):
        head = ops.jpeg_header(H, W, q, sub, rows)
        info = ops.jpeg_parse(head + b"\xff\xd9")
        m = 16 if sub == "4:2:0" else 8
        assert (info["H"], info["W"], info["subsampling"], info["components"]) == (H, W, sub, 3)
        assert info["restart_interval"] == rows * ((W + m - 1) // m) and info["scan"] == (len(head), len(head))
        assert info["quant_tables"] == {0: ops.jpeg_quant_table(0, q), 1: ops.jpeg_quant_table(1, q)}
        assert info["quant_selectors"] == (0, 1, 1) and info["dc_selectors"] == (0, 1, 1) and info["ac_selectors"] == (0, 1, 1)
        assert info["huffman_tables"][(0, 0)] == (tuple(REF.DC_LUMA[0]), tuple(REF.DC_LUMA[1]))
        assert info["huffman_tables"][(1, 1)] == (tuple(REF.AC_CHROMA[0]), tuple(REF.AC_CHROMA[1]))


# ---- refusals ----
def _patch(data, marker, at, value):
    i = data.index(bytes([0xFF, marker]))
    return data[:i + 4 + at] + bytes(value) + data[i + 4 + at + len(value):]


def test_parse_refuses_what_the_decoder_does_not_decode():
    from PIL import Image
    from transformerupscaler_amd import ops
    a = C.image((40, 72), "smooth")
    good = DC.save(a, quality=75)
    assert ops.jpeg_parse(good)["subsampling"] == "4:2:0"
    cmyk = io.BytesIO()
    Image.new("CMYK", (16, 16)).save(cmyk, "JPEG")
    sof = good.index(b"\xff\xc0")
    sos = good.index(b"\xff\xda")
    dht = good.index(b"\xff\xc4")
    dqt = good.index(b"\xff\xdb")
    over_full = good[:dht + 5] + bytes([3]) + good[dht + 6:]                      # three codes of one bit
    rgb_ids = good[:2] + good[good.index(b"\xff\xdb"):]                           # no JFIF segment ...
    rgb_ids = _patch(_patch(_patch(rgb_ids, 0xC0, 6, b"R"), 0xC0, 9, b"G"), 0xC0, 12, b"B")
    rgb_ids = _patch(_patch(_patch(rgb_ids, 0xDA, 1, b"R"), 0xDA, 3, b"G"), 0xDA, 5, b"B")
    adobe = good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + good[2:]      # transform 0: RGB / CMYK
    two_scans = good[:-2] + good[sos:]
    for data, reason in ((DC.save(a, progressive=True), "progressive"),
                         (DC.save(a, subsampling=1), "sampling factors 2x1, 1x1, 1x1"),
                         (cmyk.getvalue(), "four components"),
                         (_patch(good, 0xC0, 0, [12]), "12-bit precision"),
                         (good[:2] + b"\xff\xc1" + good[sof + 2:], r"extended sequential \(SOF1\)"),
                         (good[:2] + b"\xff\xc9" + good[sof + 2:], "arithmetic"),
                         (good[:sof + 7], "ends before SOS"),
                         (good[:sos + 3], "ends before SOS"),
                         (good[:20], "ends before SOS"),
                         (over_full, "not a valid prefix code"),
                         (_patch(good, 0xDB, 0, [0x10]), "16-bit quantisation tables"),
                         (_patch(good, 0xDA, 7, [1]), "Ss, Se, Ah/Al"),
                         (_patch(good, 0xDA, 8, [62]), "Ss, Se, Ah/Al"),
                         (_patch(good, 0xDA, 9, [0x10]), "Ss, Se, Ah/Al"),
                         (two_scans, "more than one scan"),
                         (adobe, "Adobe transform 0"),
                         (rgb_ids, "'R', 'G', 'B'"),
                         (good[:dqt] + good[dqt + 69:], "missing quantisation table 0"),
                         (good[:dht] + good[dht + 33:], "missing Huffman table"),
                         (_patch(good, 0xC0, 7, [0x21]), "sampling factors 2x1"),
                         (b"\x89PNG\r\n\x1a\n" + good, "no SOI")):
        with pytest.raises(ValueError, match=reason):
            ops.jpeg_parse(data)
        with pytest.raises(ValueError, match=reason):                             # and through the decoder, ahead of everything else
            ops.jpeg_decode([good, data])
    with pytest.raises(TypeError):
        ops.jpeg_parse("a string")


# ---- validation, ahead of any library call ----
def test_decode_validates_before_it_calls(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(_lib, "load", no_call)
    a = C.image((40, 72), "smooth")
    f = C.pillow(a, 75, 2, 1)
    for other, what in ((C.pillow(C.image((17, 23), "smooth"), 75, 2, 1), "share H, W"), (C.pillow(a, 75, 0, 1), "share H, W"),
                        (C.pillow(a, 75, 2, 2), "share H, W"), (C.pillow(a, 75, 2, 0), "share H, W")):
        with pytest.raises(ValueError, match=what):
            ops.jpeg_decode([f, other])
    with pytest.raises(ValueError, match="images in one call"):
        ops.jpeg_decode([])
    for bad in (None, 3, ["a string"], [f, None]):
        with pytest.raises(TypeError):
            ops.jpeg_decode(bad)
    for out in (torch.zeros((1, 40, 72, 3)), torch.zeros((2, 40, 72, 3), dtype=torch.uint8), torch.zeros((1, 3, 40, 72), dtype=torch.uint8),
                torch.zeros((1, 40, 72, 6), dtype=torch.uint8)[..., ::2], np.zeros((1, 40, 72, 3), dtype=np.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            ops.jpeg_decode(f, out=out)
    with pytest.raises(ValueError, match="out must be"):
        ops.jpeg_decode(f, to_tensor=True, out=torch.zeros((1, 40, 72, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU fallback"):                      # valid, on the CPU: refused, still no call
        ops.jpeg_decode(f, out=torch.zeros((1, 40, 72, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.jpeg_decode([f, f], to_tensor=True, out=torch.zeros((2, 3, 40, 72)))


def test_decode_refuses_a_missing_library(monkeypatch):
    from transformerupscaler_amd import _lib, ops
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.jpeg_decode(C.pillow(C.image((40, 72), "smooth"), 75, 2, 1))
        return
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "no_such_library.so"))
    with pytest.raises(_lib.TupscaleLibraryError, match="no CPU fallback"):
        ops.jpeg_decode(C.pillow(C.image((40, 72), "smooth"), 75, 2, 1))


def test_record_and_geometry_twins():
    from transformerupscaler_amd import _lib, ops
    assert ops._JPEG_DEC_REC.size == 1488
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "jpeg_decode.hip")).read()
    assert "sizeof(JdImage) == 1488" in src and '#include "jpeg_entropy.h"' in src and '#include "jpeg_dct.h"' in src
    seg = _lib.load().tup_jpeg_decode_segments
    for H, W, layout, interval in ((40, 72, 2, 5), (40, 72, 0, 9), (40, 72, 2, 0), (40, 72, 0, 0), (17, 23, 4, 1), (1, 1, 0, 0), (4320, 7680, 2, 480),
                                  (65535, 65535, 0, 65535), (65535, 65535, 2, 0), (16, 1000, 2, 7)):
        assert seg(H, W, layout, interval) == ops._jpeg_decode_geometry(H, W, layout, interval)[0], (H, W, layout, interval)
    assert ops._jpeg_decode_geometry(40, 72, 2, 5) == (3, 48 * 80 + 2 * 24 * 40) and ops._jpeg_decode_geometry(17, 23, 4, 0) == (3, 24 * 24)
    for bad in ((0, 8, 2, 0), (8, 65536, 0, 0), (8, 8, 1, 0), (8, 8, 3, 0), (8, 8, 2, -1), (8, 8, 2, 65536)):
        assert seg(*bad) == -1, bad


# ---- ABI ----
def test_decode_entries_are_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())
    for decl in ("int tup_jpeg_decode_segments(int H, int W, int layout, int restart_interval);",
                 "int tup_jpeg_decode_index(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout, "
                 "int restart_interval, int S, int* segs, int* status, void* stream);",
                 "int tup_jpeg_decode_blocks(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout, "
                 "int restart_interval, int S, const int* segs, int* status, void* workspace, long long ws_bytes, void* stream);",
                 "int tup_jpeg_decode_finish(const void* workspace, long long ws_bytes, int B, int H, int W, int layout, void* out_u8, "
                 "float* out_f32, void* stream);"):
        assert decl in header, decl
    P, I, L = _lib.P, _lib.I, ctypes.c_longlong
    assert _lib.SIGNATURES["tup_jpeg_decode_segments"] == [I, I, I, I]
    assert _lib.SIGNATURES["tup_jpeg_decode_index"] == [P, P, L, I, I, I, I, I, I, P, P, P]
    assert _lib.SIGNATURES["tup_jpeg_decode_blocks"] == [P, P, L, I, I, I, I, I, I, P, P, P, L, P]
    assert _lib.SIGNATURES["tup_jpeg_decode_finish"] == [P, L, I, I, I, I, P, P, P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.SIGNATURES if n.startswith("tup_jpeg_decode_"))
    assert "tup_jpeg_decode_index" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("jpeg_decode.hip", ["jpeg_index_kernel", "jpeg_blocks_kernel", "jpeg_finish_kernel"])' in guard
    csrc = os.path.join(ROOT, "transformerupscaler_amd", "csrc")
    assert "dg_idct8" in open(os.path.join(csrc, "jpeg_dct.h")).read()                        # one inverse DCT, beside the forward one
    assert "void dg_idct8" not in open(os.path.join(csrc, "degrade.hip")).read()
    assert len(re.findall(r"__global__", open(os.path.join(csrc, "jpeg_decode.hip")).read())) == 3


def test_decode_entries_refuse_bad_arguments_before_they_launch():
    from transformerupscaler_amd import _lib
    lib = _lib.load()
    invalid = 1                                         # hipErrorInvalidValue
    buf = (ctypes.c_int * 1024)()                       # host memory: never dereferenced by a refused call
    a = (ctypes.addressof(buf) + 15) & ~15
    index, blocks, finish = lib.tup_jpeg_decode_index, lib.tup_jpeg_decode_blocks, lib.tup_jpeg_decode_finish
    ws = 48 * 80 + 2 * 24 * 40
    for args in ((None, a, 64, 1, 40, 72, 2, 5, 3, a, a), (a, None, 64, 1, 40, 72, 2, 5, 3, a, a), (a, a + 4, 64, 1, 40, 72, 2, 5, 3, a, a),
                 (a, a, -1, 1, 40, 72, 2, 5, 3, a, a), (a, a, 2 ** 31, 1, 40, 72, 2, 5, 3, a, a), (a, a, 64, 0, 40, 72, 2, 5, 3, a, a),
                 (a, a, 64, 65536, 40, 72, 2, 5, 3, a, a), (a, a, 64, 1, 0, 72, 2, 5, 3, a, a), (a, a, 64, 1, 40, 65536, 2, 5, 3, a, a),
                 (a, a, 64, 1, 40, 72, 1, 5, 3, a, a), (a, a, 64, 1, 40, 72, 2, 65536, 3, a, a), (a, a, 64, 1, 40, 72, 2, 5, 4, a, a),
                 (a, a, 64, 1, 40, 72, 2, 5, 3, None, a), (a, a, 64, 1, 40, 72, 2, 5, 3, a, None)):
        assert index(*args, None) == invalid, args
        assert blocks(*args, a, ws, None) == invalid, args
    good = (a, a, 64, 1, 40, 72, 2, 5, 3, a, a)
    assert blocks(*good, None, ws, None) == invalid and blocks(*good, a, ws + 1, None) == invalid and blocks(*good, a + 4, ws, None) == invalid
    for args in ((None, ws, 1, 40, 72, 2, a, None), (a, ws - 1, 1, 40, 72, 2, a, None), (a, ws, 0, 40, 72, 2, a, None), (a, ws, 1, 40, 72, 3, a, None),
                 (a, ws, 1, 40, 72, 2, a, a), (a, ws, 1, 40, 72, 2, None, None), (a, ws, 1, 40, 0, 2, a, None)):
        assert finish(*args, None) == invalid, args


# ---- damaged scans through the shared header, on the host, under the sanitizers ----
def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(c) and glob.glob(os.path.join(os.path.dirname(os.path.dirname(c)), "lib", "clang", "*", "lib", "linux", "*asan*")):
            return c
    return None


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm clang++ with a host address-sanitizer runtime found")
    exe = str(tmp_path_factory.mktemp("jpeg_entropy") / "jpeg_entropy_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "transformerupscaler_amd", "csrc"), os.path.join(HERE, "jpeg_entropy_main.cpp"), "-o", exe], check=True)

    def run(blob, path=exe + ".in"):
        with open(path, "wb") as fh:
            fh.write(blob)
        p = subprocess.run([exe, path], capture_output=True, text=True)      # a plain child process
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        m = re.fullmatch(r"status (\d+) blocks (\d+) checksum (\d+)\n", p.stdout)
        assert m, p.stdout
        return tuple(int(v) for v in m.groups())
    return run


def test_host_walker_equals_the_reference_on_good_files(walker):
    from transformerupscaler_amd import ops
    files = [C.pillow(C.image(hw, kind), q, sub, r) for hw in ((17, 23), (40, 72)) for kind, q in (("smooth", 75), ("noise", 100), ("checker", 100))
             for sub in (0, 2) for r in (1, 0)]
    files += [data for name, data in DC.extra_files() if "16x1000" not in name]
    for data in files:
        info = ops.jpeg_parse(data)
        blocks, status = R.walk(data)
        assert status == 0
        got = walker(DC.program_input(info, data[info["scan"][0]:info["scan"][1]], ops._jpeg_decode_record))
        assert got == (0, blocks.size // 64, R.checksum(blocks))


def test_host_walker_survives_damaged_scans(walker):
    from transformerupscaler_amd import ops
    info = ops.jpeg_parse(DC.good())
    cases = DC.damaged()
    assert len(cases) > 200 and sum(n.startswith("byte") for n, *_ in cases) == 64
    complete = 0
    for name, head, scan, interval in cases:
        status, blocks, _ = walker(DC.program_input(dict(info, restart_interval=interval), scan, ops._jpeg_decode_record))
        assert status != 0 or blocks == 3 * 5 * 6, name                          # a non-zero status, or a complete decode
        complete += status == 0
        if name.startswith("cut") or name in ("no-markers", "no-dri"):
            assert status != 0, name
        # the numpy walker says the same of it
        data = head + scan + DC.EOI
        assert (R.walk(data, dict(info, restart_interval=interval, scan=(len(head), len(head) + len(scan))))[1] != 0) == (status != 0), name
    assert complete < 64                                                          # most byte changes are noticed; none may crash
