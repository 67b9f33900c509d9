"""The self-synchronising index of a JPEG scan without restart markers (csrc/jpeg_sync.h, csrc/jpeg_sync.hip) without a
GPU: its Python statement tests/_jpeg_sync_ref.py against the serial walk on every case, csrc/jpeg_sync.h on the host under the address
and undefined-behaviour sanitizers (tests/jpeg_sync_main.cpp, a stand-alone program) on those cases and on damaged scans, the C ABI of
the new entry, and what `ops.jpeg_decode(index=...)` and `ops.jpeg_scan_index` refuse before any launch."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _jpeg_decode_cases as DC  # noqa: E402
import _jpeg_decode_ref as R  # noqa: E402
import _jpeg_sync_ref as S  # noqa: E402
from _abi import ABI  # noqa: E402

CSRC = os.path.join(ROOT, "transformerupscaler_amd", "csrc")


def _scan(data):
    from transformerupscaler_amd import ops
    info = ops.jpeg_parse(data)
    assert info["restart_interval"] == 0
    return info, data[info["scan"][0]:info["scan"][1]]


# ---- the constant, and what the cases are ----
def test_subsequence_size_is_the_headers():
    from transformerupscaler_amd import ops
    T = int(re.search(r"constexpr int JS_BYTES = (\d+);", open(os.path.join(CSRC, "jpeg_sync.h")).read()).group(1))
    assert ops.JPEG_SYNC_BYTES == T and T >= 16 and T % 4 == 0
    assert f"{T} raw bytes" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())


def test_cases_are_what_they_are_for():
    from transformerupscaler_amd import ops
    T = ops.JPEG_SYNC_BYTES
    scans = {name: _scan(data)[1] for name, data in S.cases()}
    assert len(scans["grey-8x8"]) < T
    noise = scans["noise-256x256-q95"]
    assert len(noise) > 256 * T and noise.count(b"\xff\x00") > 0
    assert any(noise[k - 1] == 0xFF and noise[k] == 0 for k in range(T, len(noise), T))       # a boundary on the 00 of a pair
    assert [len(scans[f"length-kT{d:+d}"]) % T for d in (-1, 0, 1)] == [T - 1, 0, 1]
    info = ops.jpeg_parse(dict(S.cases())["gradient-optimize"])
    assert info["huffman_tables"][(1, 0)] != ops.jpeg_parse(dict(S.cases())["420-16x16"])["huffman_tables"][(1, 0)]
    for name, rows in (("flat-grey-2048x8", 256), ("flat-420-1024x16", 64)):                 # many row starts in one subsequence
        assert len(scans[name]) < 2 * T + T and len(S.serial_rows(scans[name], _scan(dict(S.cases())[name])[0])[0]) == rows
    flat = scans["flat-grey-optimize-4096x4096"]                  # one-bit codes: two bits a block, four block ends a byte
    flat_info = ops.jpeg_parse(dict(S.cases())["flat-grey-optimize-4096x4096"])
    assert all(sum(counts) == 1 and counts[0] == 1 for counts, _ in flat_info["huffman_tables"].values())
    assert len(flat) * 4 == 512 * 512 and len(flat) > 256 * T and 256 * T * 4 > 1 << 17      # more than 2^17 block ends in the first span
    assert {n.split("-")[0] for n, _ in S.cases()} >= {"grey", "420", "444", "flat", "noise", "gradient", "length"}


# ---- the Python statement against the serial walk ----
@pytest.mark.parametrize("name,data", S.cases(), ids=[n for n, _ in S.cases()])
def test_python_statement_equals_the_serial_walk(name, data):
    from transformerupscaler_amd import ops
    info, scan = _scan(data)
    want, status = S.serial_rows(scan, info)
    assert status == 0 and R.walk(data, info)[1] == 0
    got, sync_status, rounds, nsub = S.sync_rows(scan, info, ops.JPEG_SYNC_BYTES)
    assert sync_status == 0 and got == want                           # the logical bit, mcu0 and the three predictors of every row
    assert 0 <= rounds <= nsub == -(-len(scan) // ops.JPEG_SYNC_BYTES)
    _, mh, mw, _ = R.geometry(info)
    assert sorted(got) == list(range(mh)) and [got[r][1] for r in range(mh)] == [r * mw for r in range(mh)]


def test_python_statement_on_damaged_scans_is_the_serial_walk():
    from transformerupscaler_amd import ops
    seen = set()
    for data in S.damaged_batch():
        info, scan = _scan(data)
        want, status = S.serial_rows(scan, info)
        got, sync_status, rounds, nsub = S.sync_rows(scan, info, ops.JPEG_SYNC_BYTES)
        assert (got, sync_status) == (want, status) and 0 <= rounds <= nsub
        seen.add(status)
    assert seen == {R.OK, R.END, R.MARKER}


# ---- csrc/jpeg_sync.h on the host, under the sanitizers ----
def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(c) and glob.glob(os.path.join(os.path.dirname(os.path.dirname(c)), "lib", "clang", "*", "lib", "linux", "*asan*")):
            return c
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm clang++ with a host address-sanitizer runtime found")
    exe = str(tmp_path_factory.mktemp("jpeg_sync") / "jpeg_sync_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(HERE, "jpeg_sync_main.cpp"), "-o", exe], check=True)

    def rows(text):
        return [None if r == "-" else tuple(int(v) for v in r.split(",")) for r in text.split()]

    def run(info, scan, path=exe + ".in"):
        from transformerupscaler_amd import ops
        with open(path, "wb") as fh:
            fh.write(DC.program_input(info, scan, ops._jpeg_decode_record))
        p = subprocess.run([exe, path], capture_output=True, text=True)          # a plain child process, nothing preloaded
        assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
        m = re.fullmatch(r"serial status (\d+) rows (\d+) :(.*)\nsync status (\d+) rounds (\d+) subsequences (\d+) fallback ([01]) rows (\d+) :(.*)\n", p.stdout)
        assert m, p.stdout[-500:]
        serial = {"status": int(m.group(1)), "rows": rows(m.group(3))}
        sync = {"status": int(m.group(4)), "rounds": int(m.group(5)), "subsequences": int(m.group(6)), "fallback": int(m.group(7)), "rows": rows(m.group(9))}
        assert len(serial["rows"]) == int(m.group(2)) == len(sync["rows"]) == int(m.group(8))
        return serial, sync
    return run


def test_host_program_equals_the_serial_walk_on_every_case(program):
    for name, data in S.cases():
        info, scan = _scan(data)
        serial, sync = program(info, scan)
        want, status = S.serial_rows(scan, info)
        assert serial["status"] == sync["status"] == status == 0 and sync["fallback"] == 0, name
        assert serial["rows"] == sync["rows"] == [want[r] for r in range(len(want))], name
        assert 0 <= sync["rounds"] <= sync["subsequences"], name


def test_host_program_on_damaged_scans_gives_the_serial_walks_answer(program):
    """Truncations, flipped bits, an inserted marker, random bytes: the run is clean, and records and status are the serial walker's
    (rows it did not place included)."""
    from transformerupscaler_amd import ops
    T = ops.JPEG_SYNC_BYTES
    base = dict(S.cases())["gradient-optimize"]
    info, scan = _scan(base)
    big_info, big = _scan(dict(S.cases())["noise-256x256-q95"])
    rng = np.random.default_rng(3)
    cases = [(f"cut-{t}", info, scan[:t]) for t in (0, 1, 2, T - 1, T, T + 1, len(scan) // 2, len(scan) - 1)]
    cases += [("cut-ff", info, scan[:scan.index(b"\xff\x00") + 1])] if b"\xff\x00" in scan else []
    for p, bit in zip(rng.integers(0, len(scan), 48), rng.integers(0, 8, 48)):
        cases.append((f"flip-{int(p)}.{int(bit)}", info, scan[:p] + bytes([scan[p] ^ (1 << int(bit))]) + scan[p + 1:]))
    for p, m in ((len(scan) // 2, b"\xff\xd9"), (T, b"\xff\xd9"), (T - 1, b"\xff\xd9"), (3 * T + 5, b"\xff\xc4"), (len(scan) - 3, b"\xff\xff")):
        cases.append((f"marker-{p}", info, scan[:p] + m + scan[p + 1:]))
    for n in (1, T, 2 * T + 7, 3000):
        cases.append((f"random-{n}", info, bytes(rng.integers(0, 256, n, dtype=np.uint8))))
    cases.append(("ff-only", info, b"\xff" * 300))
    cases.append(("ff00-only", info, b"\xff\x00" * 300))
    cases.append(("big-cut-second-span", big_info, big[:256 * T + 40 * T + 3]))
    cases.append(("big-marker-second-span", big_info, big[:300 * T] + b"\xff\xd9" + big[300 * T + 1:]))
    flat_info, flat = _scan(dict(S.cases())["flat-grey-optimize-4096x4096"])       # two bits a block: the most block ends a span holds
    cases.append(("big-cut-flat-second-span", flat_info, flat[:256 * T + 5000]))
    cases.append(("big-marker-flat-first-span", flat_info, flat[:200 * T] + b"\x80" + flat[200 * T + 1:]))          # a bit that is no code
    cases.append(("big-flip-first-span", big_info, big[:9 * T] + bytes([big[9 * T] ^ 0x10]) + big[9 * T + 1:]))
    flips = {True: 0, False: 0}
    for name, inf, sc in cases:
        serial, sync = program(inf, sc)
        assert (sync["status"], sync["rows"]) == (serial["status"], serial["rows"]), name
        assert 0 <= sync["rounds"] <= max(sync["subsequences"], 0), name
        want, status = S.serial_rows(sc, inf)                           # and the Python walker says the same of it
        assert serial["status"] == status and [r for r in serial["rows"] if r is not None] == [want[r] for r in range(len(want))], name
        if name.startswith("flip"):
            flips[status == 0] += 1
            assert sync["fallback"] == (status != 0), name
        if name.startswith(("cut", "big-cut", "big-marker", "ff")):
            assert status != 0 and sync["fallback"] == 1, name
    assert flips[True] > 0                            # changed scans that still decode do so through the parallel path


# ---- ABI ----
def test_sync_entry_is_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())
    assert ("int tup_jpeg_decode_index_sync(const void* records, const void* scans, long long scans_bytes, int B, int H, int W, int layout, "
            "int* segs, int* status, int* rounds, void* stream);") in header
    P, I, L = _lib.P, _lib.I, ctypes.c_longlong
    assert _lib.SIGNATURES["tup_jpeg_decode_index_sync"] == [P, P, L, I, I, I, I, P, P, P, P]
    assert _lib.SIGNATURES["tup_jpeg_decode_index"] == [P, P, L, I, I, I, I, I, I, P, P, P]                # unchanged
    assert _lib.ABI_VERSION == ABI == 16
    assert "#define TUP_ABI_VERSION 16" in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = _lib.load()
    assert hasattr(lib, "tup_jpeg_decode_index_sync") and lib.tup_abi_version() == 16
    guard = open(os.path.join(CSRC, "check_resources.py")).read()
    assert '("jpeg_sync.hip", ["jpeg_sync_index_kernel"])' in guard
    src = open(os.path.join(CSRC, "jpeg_sync.hip")).read()
    assert len(re.findall(r"__global__", src)) == 1 and '#include "jpeg_sync.h"' in src and "jd_serial_index" in src
    assert "jd_serial_index" in open(os.path.join(CSRC, "jpeg_decode.hip")).read()                          # one serial walk for both
    assert "tup_jpeg_decode_index_sync" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_sync_entry_refuses_bad_arguments_before_it_launches():
    from transformerupscaler_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int * 1024)()                       # host memory: never dereferenced by a refused call
    a = (ctypes.addressof(buf) + 15) & ~15
    for args in ((None, a, 64, 1, 40, 72, 2, a, a, a), (a, None, 64, 1, 40, 72, 2, a, a, a), (a, a + 4, 64, 1, 40, 72, 2, a, a, a),
                 (a, a, -1, 1, 40, 72, 2, a, a, a), (a, a, 2 ** 31, 1, 40, 72, 2, a, a, a), (a, a, 64, 0, 40, 72, 2, a, a, a),
                 (a, a, 64, 65536, 40, 72, 2, a, a, a), (a, a, 64, 1, 0, 72, 2, a, a, a), (a, a, 64, 1, 40, 65536, 2, a, a, a),
                 (a, a, 64, 1, 40, 72, 1, a, a, a), (a, a, 64, 1, 40, 72, 2, None, a, a), (a, a, 64, 1, 40, 72, 2, a, None, a)):
        assert lib.tup_jpeg_decode_index_sync(*args, None) == 1, args          # hipErrorInvalidValue


# ---- ops: validation ahead of any library call ----
def test_index_argument_is_validated_before_any_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(_lib, "load", no_call)
    plain = dict(S.cases())["420-16x16"]
    marked = DC.save(np.zeros((16, 16, 3), np.uint8), quality=75, subsampling=2, restart_marker_rows=1)
    assert ops.jpeg_parse(marked)["restart_interval"] > 0
    for fn in (ops.jpeg_decode, ops.jpeg_scan_index):
        with pytest.raises(ValueError, match="index must be one of"):
            fn(plain, index="parallel")
        with pytest.raises(ValueError, match="index must be one of"):
            fn(plain, index=None)
        with pytest.raises(ValueError, match="without restart markers"):
            fn(marked, index="sync")
        with pytest.raises(ValueError, match="without restart markers"):
            fn([marked, marked], index="sync")
        with pytest.raises(ValueError, match="share H, W"):
            fn([plain, marked], index="sync")
