"""CPU checks of the PNG encoder: the Python statement tests/_png_ref.py decoded by Pillow and taken apart with zlib, on
inputs asserted to reach the coder's hard cases; conditions on the files' lengths; the Huffman builder, run-length coder and checksums
of csrc/png_deflate.h, built for the host under the address and undefined-behaviour sanitizers, against the same statement;
`ops.png_encode`'s validation ahead of any library call; the `tup_png_*` entries through header / binding / library; and
`inference.py`'s choice of format by suffix.  Images are synthesised in tests/_png_cases.py."""
import ctypes
import io
import os
import re
import struct
import subprocess
import warnings
import zlib

import numpy as np
import pytest
import torch

import _png_cases as C
import _png_ref as REF
from _abi import ABI

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def walk(data):
    """[(type, payload)] of a PNG file, every chunk's CRC checked"""
    assert data[:8] == REF.SIGNATURE
    out, i = [], 8
    while i < len(data):
        n, kind = struct.unpack(">I4s", data[i:i + 8])
        payload = data[i + 8:i + 8 + n]
        assert len(payload) == n and struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(kind + payload), (kind, i)
        out.append((kind, payload))
        i += 12 + n
    assert i == len(data)
    return out


def check_file(data, a, block_bytes, filter):
    from PIL import Image
    h, w, _ = a.shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Image.open(io.BytesIO(data)).verify()
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), a)
    chunks = walk(data)
    n = REF.blocks(h, w, block_bytes)
    assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (n + 1) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and chunks[-1][1] == b"" and len(chunks[-2][1]) == 4
    stream = b"".join(p for k, p in chunks if k == b"IDAT")
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == REF.filtered(a, filter)                      # the Adler-32 is checked by zlib
    assert len(data) <= REF.file_bound(h, w, block_bytes)
    return chunks


@pytest.mark.parametrize("hw", C.SIZES + C.EXTRA)
def test_reference_files_are_png_files(hw):
    pytest.importorskip("PIL.Image")
    mine = [c for c in C.cases() if c[0] == hw]
    assert mine and (hw in C.EXTRA or ({c[2] for c in mine} >= set(C.BLOCKS) and {c[1] for c in mine} == set(C.KINDS)))
    for _, kind, bb, f in mine:
        data, stats = C.reference(hw, kind, bb, f)
        a = C.image(hw, kind)
        chunks = check_file(data, a, bb, f)
        # every block is an IDAT of its own that is no longer than its stored form
        stream_len = hw[0] * (1 + 3 * hw[1])
        for i, (_, payload) in enumerate(chunks[1:-2]):
            n = min(bb, stream_len - i * bb)
            assert len(payload) - (2 if i == 0 else 0) <= 5 + n, (hw, kind, bb, f, i)
        assert len(stats["forms"]) == len(chunks) - 3


def test_the_cases_cover_sizes_kinds_blocks_and_filters():
    cases = C.cases()
    assert 140 <= len(cases) <= 200 and len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == set(C.SIZES) | set(C.EXTRA) and REF.blocks(C.MANY[0], C.MANY[1], 256) > 256
    for f in C.FIXED:
        assert len({c[0] for c in cases if c[3] == f}) >= 2, f
    assert sum(c[3] == "adaptive" for c in cases) >= 60
    assert REF.blocks(17, 23, 256) == 5 and 1 + 3 * 1000 > 2 * 1024 and REF.blocks(3, 4000, 32768) == 2 and 32768 % (1 + 3 * 4000) != 0
    forms = {}
    for c in cases:
        for f in C.reference(*c)[1]["forms"]:
            forms[f] = forms.get(f, 0) + 1
    assert forms["stored"] > 10 and forms["fixed"] > 10 and forms["dynamic"] > 10


def test_the_inputs_reach_the_hard_cases():
    """Conditions on the inputs, not on the encoder."""
    # deep: without the limit the code is deeper than 15 bits, so the repair acts; no match anywhere
    data, stats = C.reference(C.DEEP, "deep", 32768, "none")
    plan = stats["plans"][0]
    assert stats["forms"] == ["dynamic"] and all(k == "L" for k, _ in plan["tokens"])
    hist = [0] * 286
    for _, v in plan["tokens"]:
        hist[v] += 1
    hist[256] = 1
    assert max(REF.code_lengths(hist, 40)) > 15 and max(plan["ll"]) == 15
    assert abs(sum(2.0 ** -l for l in plan["ll"] if l) - 1.0) == 0.0
    assert plan["dl"] == [0] * 30 and plan["hdist"] == 1                          # no distance code at all
    # noise: no match, stored; flat: one literal value and matches of 258; 1 x 1: a block of four bytes
    assert set(C.reference((40, 72), "noise", 1024, "adaptive")[1]["forms"]) == {"stored"}
    _, flat = C.reference((16, 1000), "flat255", 32768, "none")
    toks = flat["plans"][0]["tokens"]
    assert {v for k, v in toks if k == "L"} == {0, 255} and ("M", 258) in toks
    data, one = C.reference((1, 1), "smooth", 256, "adaptive")
    assert len(one["plans"][0]["tokens"]) <= 4 and len(REF.filtered(C.image((1, 1), "smooth"))) == 4
    # the remainder rule: a run's tail of one or two bytes is literals, of three or more a match
    for r, want in ((1, ["L"]), (3, ["L"] * 3), (4, ["L", "M"]), (259, ["L", "M"]), (260, ["L", "M", "L"]), (261, ["L", "M", "L", "L"]),
                    (262, ["L", "M", "M"]), (517, ["L", "M", "M"])):
        assert [k for k, _ in REF.tokens(bytes([7]) * r)] == want, r
    assert REF.tokens(bytes([7]) * 262)[1:] == [("M", 258), ("M", 3)]
    # the header's run lengths use 16, 17 and 18
    used = set()
    for c in C.cases()[::5]:
        for p in C.reference(*c)[1]["plans"]:
            used |= {s for s, _, _ in p["cl_tokens"]}
    assert {16, 17, 18} <= used


def test_adaptive_filter_is_the_arg_min_with_ties_to_the_lowest():
    a = C.image((17, 23), "smooth")
    types = REF.filter_types(a)
    rows = a.reshape(17, 69)
    for y in range(17):
        cand = REF._candidates(rows[y], rows[y - 1] if y else np.zeros(69, np.uint8))
        sums = [int(np.abs(c.view(np.int8).astype(np.int64)).sum()) for c in cand]
        assert types[y] == sums.index(min(sums))
    assert len(set(types.tolist())) >= 2
    # rows built to tie.  A flat image of 9s: in row 0 sub and paeth both leave the first pixel only (27; none and up 135, average 87)
    # -> sub; below it up and paeth are both 0 -> up
    flat = np.full((3, 5, 3), 9, np.uint8)
    assert REF.filter_types(flat).tolist() == [1, 2, 2]
    assert REF.filter_types(np.zeros((2, 4, 3), np.uint8)).tolist() == [0, 0]      # all five are 0 -> none
    tie = np.zeros((2, 2, 3), np.uint8)
    tie[1, 0] = 4                                                                   # row 1: none 12 and up 12 (sub 24) -> none
    assert REF.filter_types(tie).tolist() == [0, 0]
    # signed reading: 255 counts as 1, 128 as 128
    assert REF.filter_types(np.full((1, 1, 3), 255, np.uint8)).tolist() == [0]


def test_conditions_on_length():
    Image = pytest.importorskip("PIL.Image")
    noise = C.image((64, 96), "noise")
    assert len(REF.encode(noise, 32768, "adaptive")) <= REF.file_bound(64, 96, 32768)
    assert len(REF.encode(noise, 1024, "adaptive")) <= REF.file_bound(64, 96, 1024)
    flat = C.image((64, 96), "flat255")
    size = len(REF.encode(flat, 1024, "adaptive"))
    print("flat255 (64, 96) at 1024:", size, "bytes =", size / (64 * 289.0), "of the filtered stream")
    assert size <= 64 * (1 + 3 * 96) / 10
    from transformerupscaler_amd import ops
    smooth = C.image((256, 384), "smooth")
    mine = len(REF.encode(smooth, ops.PNG_BLOCK_BYTES, "adaptive"))
    pil = {}
    for level in (1, 6):
        buf = io.BytesIO()
        Image.fromarray(smooth).save(buf, "PNG", compress_level=level)
        pil[level] = len(buf.getvalue())
    print("smooth (256, 384):", mine, "bytes; Pillow level 1:", pil[1], "ratio", mine / pil[1], "; level 6:", pil[6], "ratio", mine / pil[6])
    assert mine <= 1.05 * pil[1]


# ---- csrc/png_deflate.h on the host, under the sanitizers ----
def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def deflate(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm clang++ with a host address-sanitizer runtime found")
    exe = str(tmp_path_factory.mktemp("png_deflate") / "png_deflate_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "transformerupscaler_amd", "csrc"), os.path.join(HERE, "png_deflate_main.cpp"), "-o", exe], check=True)

    def run(lines, path=exe + ".in"):
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip().split("\n")
    return run


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_huffman_builder_on_the_host(deflate):
    rng = np.random.default_rng(5)
    end_only = [0] * 286
    end_only[256] = 1
    hists = [(15, _fib(25)), (15, _fib(40)[:30]), (15, [0] * 100 + [9] + [0] * 185), (15, [3] + [0] * 255 + [1] + [0] * 29), (15, [5] * 286),
             (15, end_only), (7, _fib(19)), (7, [0] * 18 + [4]), (7, [1] * 19)]
    for _ in range(20):
        n = int(rng.integers(2, 287))
        hists.append((15, (rng.integers(0, 3, n) * rng.integers(0, 4000, n)).tolist()))
        hists.append((7, (rng.integers(0, 3, 19) * rng.integers(0, 400, 19)).tolist()))
    got = deflate([f"L {limit} {len(h)} " + " ".join(map(str, h)) for limit, h in hists])
    assert len(got) == len(hists)
    for (limit, h), line in zip(hists, got):
        lens, codes = ([int(v) for v in part.split()] for part in line[2:].split("|"))
        used = [l for l, f in zip(lens, h) if f]
        assert all(l == 0 for l, f in zip(lens, h) if not f) and all(1 <= l <= limit for l in used)
        if len(used) >= 2:
            assert sum(1 << (limit - l) for l in used) == 1 << limit                # Kraft sum exactly 1
        elif used:
            assert used == [1]
        want = REF.code_lengths(h, limit)
        assert lens == want and codes == REF.canonical(want)
    assert max(int(v) for v in got[0][2:].split("|")[0].split()) == 15 and max(REF.code_lengths(_fib(25), 40)) > 15
    assert max(int(v) for v in got[6][2:].split("|")[0].split()) == 7 and max(REF.code_lengths(_fib(19), 40)) > 7


def test_run_lengths_and_checksums_on_the_host(deflate):
    rng = np.random.default_rng(6)
    lines, want = [], []
    seqs = [[0] * 316, [8] * 316, [0] * 138 + [3], [0] * 139 + [3], [0] * 10 + [5] * 7 + [0] * 2 + [5] * 4 + [0] * 11, [1], [0, 0, 0], [7, 7, 7, 7]]
    for _ in range(20):
        n = int(rng.integers(1, 317))
        seqs.append(np.repeat(rng.integers(0, 16, n) * (rng.random(n) < 0.5), rng.integers(1, 150, n))[:n].tolist())
    for seq in seqs:
        lines.append(f"R {len(seq)} " + " ".join(map(str, seq)))
        toks = REF.run_length_code(seq)
        cl = [0] * 19
        for s, _, _ in toks:
            cl[s] += 1
        want.append("R " + " ".join(str(s | v << 8) for s, _, v in toks) + " | " + " ".join(map(str, cl)))
        # what the tokens say is the sequence
        back = []
        for s, _, v in toks:
            back += [s] if s < 16 else [back[-1]] * (v + 3) if s == 16 else [0] * (v + (3 if s == 17 else 11))
        assert back == list(seq)
    for n, piece in ((0, 5), (1, 1), (4, 7), (100, 7), (5000, 132), (40000, 516), (70000, 32768)):
        d = rng.integers(0, 256, n).astype(np.uint8) if n != 70000 else np.full(n, 255, np.uint8)
        text = " ".join(map(str, d.tolist()))
        lines += [f"C {piece} {n} {text}", f"A {piece} {n} {text}"]
        want += [f"C {zlib.crc32(d.tobytes())}", f"A {zlib.adler32(d.tobytes())}"]
        assert REF.adler32(d.tobytes()) == zlib.adler32(d.tobytes())
    lines.append("S 3 258")
    want.append("S " + " ".join("%d,%d,%d" % REF.length_symbol(n) for n in range(3, 259)))
    # the fixed code as RFC 1951 3.2.6 prints it: 00110000.. for 0..143, 110010000.. for 144..255, 0000000.. for 256..279, 11000000.. after
    rev = lambda code, n: int(format(code, f"0{n}b")[::-1], 2)
    lines.append("F")
    want.append("F " + " ".join(str(rev(0x30 + s, 8) if s < 144 else rev(0x190 + s - 144, 9) if s < 256 else rev(s - 256, 7) if s < 280
                                    else rev(0xC0 + s - 280, 8)) for s in range(288)))
    assert REF.canonical(REF.FIXED_LENGTHS) == [int(v) for v in want[-1][2:].split()]
    assert deflate(lines) == want
    # the length symbols are deflate's: bases 3..258 in 29 steps
    bases = sorted({s: n for n in range(258, 2, -1) for s in [REF.length_symbol(n)[0]]}.items())
    assert [n for _, n in bases] == [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    assert [s for s, _ in bases] == list(range(257, 286))


# ---- the op's host checks ----
def test_png_encode_validates_before_any_library_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("a library call was reached")
    monkeypatch.setattr(_lib, "call", reached)
    monkeypatch.setattr(_lib, "load", reached)
    u = torch.zeros((2, 9, 11, 3), dtype=torch.uint8)
    f = torch.zeros((2, 3, 9, 11))
    for bad in ("best", "Paeth", 0, None, True, 4):
        with pytest.raises(ValueError, match="filter"):
            ops.png_encode(u, filter=bad)
    for bad in (255, 32769, 0, -1, 1024.0, "1024", None, True):
        with pytest.raises(ValueError, match="block_bytes"):
            ops.png_encode(u, block_bytes=bad)
        with pytest.raises(ValueError, match="block_bytes"):
            ops.png_max_bytes(9, 11, bad)
    with pytest.raises(ValueError, match="at least 1 x 1"):
        ops.png_encode(torch.zeros((1, 0, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 1 x 1"):
        ops.png_max_bytes(4, 0)
    with pytest.raises(ValueError, match="below 2\\^31"):
        ops.png_max_bytes(46343, 15446)                                             # 46343 x 46339 = 2147488277 >= 2^31
    with pytest.raises(ValueError, match="images in one call"):
        ops.png_encode(u[:0])
    for bad in (u[..., :2], u[0, 0], f[:, :2], f[0], torch.zeros((2, 9, 11, 3))):
        with pytest.raises(ValueError, match="frames must be"):
            ops.png_encode(bad)
    for bad in (u.numpy(), f.double(), u.to(torch.int32), None):
        with pytest.raises(TypeError):
            ops.png_encode(bad)
    with pytest.raises(ValueError, match="contiguous"):
        ops.png_encode(u[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ops.png_encode(f[:, :, :, ::2])
    lengths = torch.zeros(2, dtype=torch.int32)
    for out in ((torch.zeros((2, 64)), lengths), (torch.zeros((3, 64), dtype=torch.uint8), lengths), (torch.zeros(128, dtype=torch.uint8), lengths),
                (torch.zeros((2, 128), dtype=torch.uint8)[:, ::2], lengths)):
        with pytest.raises(ValueError, match=r"out\[0\]"):
            ops.png_encode(u, out=out)
    data = torch.zeros((2, 64), dtype=torch.uint8)
    for out in ((data, lengths.long()), (data, torch.zeros(3, dtype=torch.int32)), (data, [0, 0])):
        with pytest.raises(ValueError, match=r"out\[1\]"):
            ops.png_encode(u, out=out)
    for good in (u, f, u[0]):                                                       # all valid, on the CPU: refused, still no call
        with pytest.raises(ValueError, match="no CPU fallback"):
            ops.png_encode(good)
    with pytest.raises(ValueError, match="png_files: image 1 did not fit"):
        ops.png_files(torch.zeros((2, 8), dtype=torch.uint8), torch.tensor([4, -1], dtype=torch.int32))
    assert ops.png_files(torch.arange(16, dtype=torch.uint8).view(2, 8), torch.tensor([3, 0], dtype=torch.int32)) == [b"\0\1\2", b""]
    with pytest.raises(ValueError, match="jpeg_files: image 0 did not fit"):
        ops.jpeg_files(torch.zeros((1, 8), dtype=torch.uint8), torch.tensor([-1], dtype=torch.int32))
    # the bound is the all-stored file, and the binding's constants are the reference's
    for (h, w), bb in (((1, 1), 256), ((17, 23), 256), ((16, 1000), 1024), ((2160, 3840), 32768), ((4320, 7680), 4096)):
        assert ops.png_max_bytes(h, w, bb) == REF.file_bound(h, w, bb)
    assert ops.png_max_bytes(40, 72) == REF.file_bound(40, 72, ops.PNG_BLOCK_BYTES)
    assert ops.PNG_FILTERS == REF.FILTERS and (ops.PNG_MIN_BLOCK, ops.PNG_MAX_BLOCK) == (REF.MIN_BLOCK, REF.MAX_BLOCK) == (256, 32768)
    assert ops.PNG_MIN_BLOCK <= ops.PNG_BLOCK_BYTES <= ops.PNG_MAX_BLOCK
    noise = C.image((40, 72), "noise")
    assert len(REF.encode(noise, 256, "none")) == REF.file_bound(40, 72, 256)      # noise is stored: the bound is reached


# ---- ABI ----
def test_png_entries_are_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())
    for decl in ("int tup_png_blocks(int H, int W, int block_bytes);",
                 "int tup_png_filters(const void* frames_u8, const float* frames_f32, int B, int H, int W, void* filters, void* stream);",
                 "int tup_png_sizes(const void* frames_u8, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, "
                 "const void* filters, int* sizes, int* partials, void* stream);",
                 "int tup_png_offsets(const int* sizes, const int* partials, int B, int H, int W, int block_bytes, long long capacity, "
                 "int* offsets, int* lengths, int* adlers, void* stream);",
                 "int tup_png_write(const void* frames_u8, const float* frames_f32, int B, int H, int W, int filter, int block_bytes, "
                 "const void* filters, const int* offsets, const int* lengths, const int* adlers, void* data, long long capacity, void* stream);"):
        assert decl in header, decl
    P, I, L = _lib.P, _lib.I, ctypes.c_longlong
    assert _lib.SIGNATURES["tup_png_blocks"] == [I, I, I]                         # an int count, called through load(), not call()
    assert _lib.SIGNATURES["tup_png_filters"] == [P, P, I, I, I, P, P]
    assert _lib.SIGNATURES["tup_png_sizes"] == [P, P, I, I, I, I, I, P, P, P, P]
    assert _lib.SIGNATURES["tup_png_offsets"] == [P, P, I, I, I, I, L, P, P, P, P]
    assert _lib.SIGNATURES["tup_png_write"] == [P, P, I, I, I, I, I, P, P, P, P, P, L, P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("tup_png_blocks", "tup_png_filters", "tup_png_sizes", "tup_png_offsets", "tup_png_write"))
    csrc = os.path.join(ROOT, "transformerupscaler_amd", "csrc")
    assert '("png_encode.hip", ["png_filter_kernel", "png_block_kernel", "png_scan_kernel"])' in open(os.path.join(csrc, "check_resources.py")).read()
    assert "png_deflate.h" in re.search(r"^HDRS\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1)
    assert '#include "png_deflate.h"' in open(os.path.join(csrc, "png_encode.hip")).read()
    usage = os.path.join(csrc, "build", "resource_usage.json")
    if os.path.exists(usage):                           # written by the build
        import json
        mine = {k: v for k, v in json.load(open(usage))["kernels"].items() if v["source"] == "png_encode.hip"}
        assert len(mine) == 4 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] for v in mine.values())


def test_entries_refuse_bad_arguments_before_they_launch():
    from transformerupscaler_amd import _lib
    lib = _lib.load()
    blocks = lib.tup_png_blocks
    assert blocks(1, 1, 256) == 1 and blocks(17, 23, 256) == 5 and blocks(16, 1000, 1024) == 47 and blocks(3, 4000, 32768) == 2
    assert blocks(2160, 3840, 32768) == 760 and blocks(4320, 7680, 32768) == 3038 and blocks(1, 65535, 32768) == 6
    assert blocks(46342, 15446, 32768) == REF.blocks(46342, 15446, 32768)          # 2147441938 bytes: the largest stream is accepted
    for bad in ((0, 8, 256), (8, 0, 256), (-1, 8, 256), (8, 8, 255), (8, 8, 32769), (8, 8, 0), (46343, 15446, 32768), (65535, 65535, 32768)):
        assert blocks(*bad) == -1, bad
    invalid = 1                                         # hipErrorInvalidValue
    buf = (ctypes.c_int * 64)()                         # host memory: never dereferenced by a refused call
    a = ctypes.addressof(buf)
    filters, sizes, offsets, write = lib.tup_png_filters, lib.tup_png_sizes, lib.tup_png_offsets, lib.tup_png_write
    assert filters(None, None, 1, 8, 8, a, None) == invalid and filters(a, a, 1, 8, 8, a, None) == invalid
    assert filters(a, None, 1, 8, 8, None, None) == invalid and filters(a, None, 0, 8, 8, a, None) == invalid
    assert filters(a, None, 1, 0, 8, a, None) == invalid and filters(a, None, 65536, 8, 8, a, None) == invalid
    assert sizes(None, None, 1, 8, 8, 0, 256, None, a, a, None) == invalid          # neither input
    assert sizes(a, a, 1, 8, 8, 0, 256, None, a, a, None) == invalid                # both
    assert sizes(a, None, 1, 8, 8, 0, 256, None, None, a, None) == invalid and sizes(a, None, 1, 8, 8, 0, 256, None, a, None, None) == invalid
    assert sizes(a, None, 1, 8, 8, 5, 256, None, a, a, None) == invalid             # adaptive without the rows' filters
    for B, H, W, f, bb in ((0, 8, 8, 0, 256), (65536, 8, 8, 0, 256), (1, 0, 8, 0, 256), (1, 8, 0, 0, 256), (1, 8, 8, -1, 256), (1, 8, 8, 6, 256),
                           (1, 8, 8, 0, 255), (1, 8, 8, 0, 32769), (1, 46343, 15446, 0, 256)):
        assert sizes(a, None, B, H, W, f, bb, a, a, a, None) == invalid, (B, H, W, f, bb)
        assert write(a, None, B, H, W, f, bb, a, a, a, a, a, 4096, None) == invalid, (B, H, W, f, bb)
    assert offsets(None, a, 1, 8, 8, 256, 4096, a, a, a, None) == invalid and offsets(a, None, 1, 8, 8, 256, 4096, a, a, a, None) == invalid
    assert offsets(a, a, 1, 8, 8, 256, 4096, None, a, a, None) == invalid and offsets(a, a, 1, 8, 8, 256, 4096, a, None, a, None) == invalid
    assert offsets(a, a, 1, 8, 8, 256, 4096, a, a, None, None) == invalid and offsets(a, a, 0, 8, 8, 256, 4096, a, a, a, None) == invalid
    assert offsets(a, a, 1, 8, 8, 255, 4096, a, a, a, None) == invalid and offsets(a, a, 1, 8, 8, 256, -1, a, a, a, None) == invalid
    assert offsets(a, a, 1, 8, 8, 256, 2 ** 31, a, a, a, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, None, a, a, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, None, a, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, a, None, a, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, a, a, None, 4096, None) == invalid
    assert write(a, None, 1, 8, 8, 0, 256, None, a, a, a, a, 2 ** 31, None) == invalid
    assert write(a, None, 1, 8, 8, 5, 256, None, a, a, a, a, 4096, None) == invalid


# ---- inference.py: the format follows the suffix ----
def test_inference_picks_the_format_from_the_suffix(monkeypatch, tmp_path):
    import inference
    from transformerupscaler_amd import metrics, ops
    assert [inference.file_format(p) for p in ("a.png", "b.PNG", "dir.png/c.Png", "d.jpg", "e.jpeg", "f", "g.png.jpg", "png")] == \
        ["png", "png", "png", "jpeg", "jpeg", "jpeg", "jpeg", "jpeg"]
    text = re.sub(r"\s+", " ", inference.build_parser().format_help())
    assert "ignored for .png files" in text and text.count("ignored for .png files") == 2 and "lossless PNG" in text and "ops.png_encode" in text

    calls = []

    def fake_jpeg(frames, **kw):
        calls.append(("jpeg", tuple(frames.shape), frames.dtype, kw))
        return "jpeg", frames

    def fake_png(frames, **kw):
        calls.append(("png", tuple(frames.shape), frames.dtype, kw))
        return "png", frames
    scored = []

    def fake_quality(a, b):
        scored.append((a.clone(), b.clone()))
        return {"ssim": torch.tensor([0.5]), "psnr": torch.tensor([20.0])}
    monkeypatch.setattr(ops, "jpeg_encode", fake_jpeg)
    monkeypatch.setattr(ops, "png_encode", fake_png)
    monkeypatch.setattr(ops, "jpeg_files", lambda kind, frames: [b"JPEG" + bytes(3)])
    monkeypatch.setattr(ops, "png_files", lambda kind, frames: [b"\x89PNG" + bytes(5)])
    monkeypatch.setattr(ops, "resize_frames", lambda x, size, resample="bilinear":
                        torch.zeros((1,) + tuple(size) + (3,), dtype=torch.uint8) + (7 if resample == "bicubic" else 3))
    monkeypatch.setattr(ops, "frames_to_tensor", lambda x: x.unsqueeze(0).permute(0, 3, 1, 2).float() / 255)
    monkeypatch.setattr(ops, "tensor_to_frames", lambda x: (x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    monkeypatch.setattr(metrics, "quality", fake_quality)
    original = torch.arange(6 * 8 * 3, dtype=torch.uint8).reshape(6, 8, 3)
    decoded = []

    def fake_decode(path_or_bytes, device, gpu=True):
        if isinstance(path_or_bytes, (bytes, bytearray)):
            decoded.append(bytes(path_or_bytes))
            return torch.full((12, 16, 3), 99, dtype=torch.uint8) if len(decoded) % 2 else torch.full((6, 8, 3), 98, dtype=torch.uint8)
        return original
    monkeypatch.setattr(inference, "decode_image", fake_decode)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    monkeypatch.chdir(tmp_path)

    def run(inp, out):
        del calls[:], scored[:], decoded[:]
        args = inference.build_parser().parse_args(["--image_path", "x.png", "--model", "BicubicInterpolation", "--no-checkpoint", "--scale", "2",
                                                    "--inp", inp, "--out", out, "--quality", "90"])
        return inference.run(args, device="cpu")

    class Model(torch.nn.Module):
        def forward(self, x, upscale_factor=2):
            return torch.full((1, 3, 12, 16), 0.5)
    import models.BicubicInterpolation.model as plugin
    monkeypatch.setattr(plugin, "TransformerModel", Model)

    rec = run("i.png", "o.PNG")
    assert [(c[0], c[2]) for c in calls] == [("png", torch.uint8), ("jpeg", torch.uint8), ("png", torch.float32)]
    assert calls[0][3] == {} and calls[2][3] == {} and calls[1][3] == {"quality": 90, "subsampling": "4:2:0"}      # no JPEG parameter reaches a PNG
    assert {k: v["format"] for k, v in rec["files"].items()} == {"inp": "png", "bicubic": "jpeg", "out": "png"}
    assert open("i.png", "rb").read()[:4] == b"\x89PNG" and open("o.PNG", "rb").read()[:4] == b"\x89PNG" and open("bicubic.jpg", "rb").read()[:4] == b"JPEG"
    assert decoded == []                                                            # nothing is decoded for a PNG
    # the model's score is on tensor_to_frames of the output (0.5 -> 127), the baseline's on the resized low-resolution frame
    assert (scored[0][1] == 127).all() and scored[0][1].dtype == torch.uint8 and tuple(scored[0][1].shape) == (12, 16, 3)
    assert (scored[1][1] == 3).all()
    rec = run("i.jpg", "o.jpeg")
    assert [c[0] for c in calls] == ["jpeg", "jpeg", "jpeg"] and all(c[3] == {"quality": 90, "subsampling": "4:2:0"} for c in calls)
    assert {k: v["format"] for k, v in rec["files"].items()} == {"inp": "jpeg", "bicubic": "jpeg", "out": "jpeg"} and len(decoded) == 2
    assert (scored[0][1] == 99).all()
    rec = run("i.jpg", "o.png")
    assert [c[0] for c in calls] == ["jpeg", "jpeg", "png"] and len(decoded) == 1 and (scored[0][1] == 127).all()
