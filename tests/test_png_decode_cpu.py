"""The PNG decoder without a GPU: the Python reference (tests/_png_decode_ref.py) against Pillow and zlib on every case
file, `ops.png_parse`'s acceptances and refusals, and csrc/png_inflate.h -- the walker the inflate kernel runs -- as a host program
under the address and undefined-behaviour sanitizers, on the sound cases and on damaged streams."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _png_decode_cases as C  # noqa: E402
import _png_decode_ref as R  # noqa: E402
from transformerupscaler_amd import ops  # noqa: E402

LOGO = os.path.join(HERE, "golden", "logo_rgba.png")


def test_reference_equals_pillow_and_zlib():
    pytest.importorskip("PIL.Image")
    names = [c.name for c in C.files()]
    assert len(set(names)) == len(names)
    for c in C.files():
        H, W, ct, _, stream = R.split(c.data)
        raw, status = R.inflate(stream, H * (1 + R.CHANNELS[ct] * W))
        assert status == R.OK, c.name
        assert raw == zlib.decompress(stream), c.name
        rgb, status = R.decode(c.data)
        assert status == R.OK and rgb.shape == (H, W, 3) and rgb.dtype == np.uint8, c.name
        if C.claimed(c):
            assert np.array_equal(rgb, C.pillow_rgb(c.data)), c.name
    short = R.decode(dict(C.files())["own_5x3_ct3_short_palette~"])[0]
    assert short[0, 0].tolist() == [0, 0, 0] and short[4, 2].tolist() != [0, 0, 0]


def test_handwritten_streams_are_what_they_claim():
    by_name = {n: s for n, _, _, s in C.handwritten()}
    assert len(by_name["distance_32768_ring_wrap"]) > 65536 or len(zlib.decompress(by_name["distance_32768_ring_wrap"])) > 65536
    # the distances and lengths the issue asks for are in the token streams: decode them with the reference's own token reader
    seen = set()
    for name, H, W, stream in C.handwritten():
        assert zlib.decompress(stream) == R.inflate(stream, H * (1 + W))[0]
        r = R.Reader(stream)
        r.pos = 16
        while True:
            head = r.peek() & 7
            r.pos += 3
            if head >> 1 == 0:
                r.pos = (r.pos + 7) & ~7
                r.pos += 32 + 8 * (r.peek() & 0xffff)
                seen.add(("stored", name))
            else:
                lit, dist = R.fixed_tables() if head >> 1 == 1 else R.dynamic_tables(r)
                seen.add(("longest", max(l for l, _ in lit)))
                seen.add(("distance codes", len(dist)))
                n = 0
                while True:
                    err, kind, used, value, length, distance = R.token(lit, dist, r.peek(), r.nbits - r.pos)
                    assert not err
                    r.pos += used
                    if kind == 2:
                        break
                    n += 1
                    if kind == 1:
                        seen.add((length, distance))
                if n == 0 and head & 1:
                    seen.add("final empty block")
            if head & 1:
                break
    assert {(258, d) for d in (1, 2, 3, 63, 64, 65, 32768)} <= seen
    assert {("longest", 15), ("distance codes", 1), ("distance codes", 0), "final empty block"} <= seen


def test_logo_fixture():
    pytest.importorskip("PIL.Image")
    data = open(LOGO, "rb").read()
    info = ops.png_parse(data)
    assert (info["H"], info["W"], info["color_type"], info["channels"]) == (768, 2400, 6, 4) and len(data) == 91833
    H, W, ct, _, stream = R.split(data)
    raw, status = R.inflate(stream, info["stream_bytes"])
    assert status == R.OK and raw == zlib.decompress(stream)
    samples, bad = R.unfilter(raw, H, W, 4)
    assert not bad and np.array_equal(R.to_rgb(samples, H, W, ct, b""), C.pillow_rgb(data))


# ---- ops.png_parse ----
def test_parse_accepts():
    for c in C.files():
        H, W, ct, palette, stream = R.split(c.data)
        info = ops.png_parse(c.data)
        assert (info["H"], info["W"], info["color_type"], info["channels"]) == (H, W, ct, R.CHANNELS[ct]), c.name
        assert info["stream_bytes"] == H * (1 + R.CHANNELS[ct] * W)
        assert b"".join(c.data[a:b] for a, b in info["idat"]) == stream, c.name
        if ct == 3:
            assert len(info["palette"]) == 768 and info["palette"][:len(palette)] == palette and not any(info["palette"][len(palette):])
        else:
            assert info["palette"] is None
    assert len(ops.png_parse(dict(C.files())["rechunk_1"])["idat"]) > 100


def test_parse_refuses():
    good = C.own(5, 3, 2, (0,))
    stream = R.split(good)[4]
    ops.png_parse(good)
    refusals = {
        "signature": b"\x89PNX" + good[4:],
        "bit depth 16": C.png(5, 3, 2, stream, depth=16),
        "bit depth 4": C.png(5, 3, 0, stream, depth=4),
        "bit depth 1": C.png(5, 3, 3, stream, depth=1, palette=bytes(6)),
        "bit depth 2": C.png(5, 3, 0, stream, depth=2),
        "Adam7": C.png(5, 3, 2, stream, interlace=1),
        "colour type 5": C.png(5, 3, 5, stream),
        "bad CRC": good[:40] + bytes([good[40] ^ 1]) + good[41:],
        "no IDAT": C.SIGNATURE + C.chunk(b"IHDR", struct.pack(">IIBBBBB", 3, 5, 8, 2, 0, 0, 0)) + C.chunk(b"IEND", b""),
        "not consecutive": C.own(5, 3, 2, (0,), idat=7, between=True),
        "without PLTE": C.png(5, 3, 3, stream),
        "ends": good[:-12],
        "ends inside": good[:-5],
        "zlib header": C.png(5, 3, 2, b"\x78\x20" + stream[2:]),
        "zlib header (method)": C.png(5, 3, 2, b"\x77\x01" + stream[2:]),
        "less than a zlib header": C.png(5, 3, 2, b"\x78"),
        "an image of": C.png(0, 3, 2, stream),
        "critical chunk": C.png(5, 3, 2, stream, before=((b"ABCD", b""),)),
    }
    for what, data in refusals.items():
        with pytest.raises(ValueError, match="png_parse"):
            ops.png_parse(data)
    with pytest.raises(ValueError, match="bit depth 16"):
        ops.png_parse(refusals["bit depth 16"])
    with pytest.raises(ValueError, match="Adam7"):
        ops.png_parse(refusals["Adam7"])
    with pytest.raises(ValueError, match="bad CRC"):
        ops.png_parse(refusals["bad CRC"])
    with pytest.raises(ValueError, match="not consecutive"):
        ops.png_parse(refusals["not consecutive"])
    with pytest.raises(ValueError, match="without PLTE"):
        ops.png_parse(refusals["without PLTE"])
    with pytest.raises(ValueError, match="no IDAT"):
        ops.png_parse(refusals["no IDAT"])
    with pytest.raises(TypeError):
        ops.png_parse("file.png")
    # ancillary chunks are skipped, wherever they are
    assert ops.png_parse(C.own(5, 3, 2, (0,), before=((b"tRNS", bytes(6)), (b"iCCP", b"x\0\0" + zlib.compress(b"p")))))["H"] == 5


def test_decode_validates_before_any_launch():
    a, b = C.own(5, 3, 2, (0,)), C.own(3, 5, 2, (0,))
    with pytest.raises(ValueError, match="share H and W"):
        ops.png_decode([a, b])
    with pytest.raises(ValueError, match="walk"):
        ops.png_decode(a, walk="lane")
    with pytest.raises(ValueError, match="images in one call"):
        ops.png_decode([])
    with pytest.raises(TypeError):
        ops.png_decode([a, "b.png"])
    with pytest.raises(ValueError, match="bit depth 16"):
        ops.png_decode([a, C.png(5, 3, 2, b"\x78\x01", depth=16)])
    with pytest.raises(ValueError, match="2\\^31"):
        ops.png_decode(C.png(60000, 60000, 0, b"\x78\x01"))


def test_damaged_streams_fail_in_the_reference():
    seen = set()
    for name, H, W, stream in C.damaged():
        rgb, status = R.decode(C.png(H, W, 0, stream))
        assert status != R.OK, name
        seen.add(status)
        try:
            zlib.decompress(stream)
            accepted = True
        except zlib.error:
            accepted = False
        assert not accepted or status in (R.BAD_FILTER, R.OUTPUT_SHORT, R.OUTPUT_LONG), name
    assert seen >= set(range(1, 11)), sorted(seen)


# ---- csrc/png_inflate.h on the host, under the sanitizers ----
def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm clang++ with a host address-sanitizer runtime found")
    exe = str(tmp_path_factory.mktemp("png_inflate") / "png_inflate_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "transformerupscaler_amd", "csrc"), os.path.join(HERE, "png_inflate_main.cpp"), "-o", exe], check=True)

    def run(lines, path=exe + ".in"):
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [tuple(int(v) for v in l.split()) for l in r.stdout.strip().split("\n")]
    return run


def _inflate_line(stream, total):
    return f"I {total} {stream.hex() or '-'}"


def _expected(stream, total):
    raw, status = R.inflate(stream, total)
    return status, zlib.crc32(raw + bytes(total - len(raw)))


def test_host_walker_on_every_case(walker):
    streams = []
    for c in C.files() + [C.Case("logo", open(LOGO, "rb").read())]:
        H, W, ct, _, stream = R.split(c.data)
        streams.append((stream, H * (1 + R.CHANNELS[ct] * W)))
    got = walker([_inflate_line(s, t) for s, t in streams])
    for c, (s, t), g in zip(C.files() + [None], streams, got):
        assert g == (R.OK, zlib.crc32(zlib.decompress(s))), c and c.name
    # the unfilter arithmetic, every filter and every pixel size
    lines, want = [], []
    for c in C.files():
        if c.name.startswith("own_5x3") or c.name.startswith("own_65x67"):
            H, W, ct, _, stream = R.split(c.data)
            raw = zlib.decompress(stream)
            lines.append(f"U {H} {W} {R.CHANNELS[ct]} {raw.hex()}")
            want.append((0, zlib.crc32(R.unfilter(raw, H, W, R.CHANNELS[ct])[0].tobytes())))
    assert walker(lines) == want


def test_host_walker_on_damaged_streams(walker):
    cases = C.damaged()
    got = walker([_inflate_line(s, H * (1 + W)) for _, H, W, s in cases])
    assert len(got) == len(cases)
    for (name, H, W, s), g in zip(cases, got):
        want = _expected(s, H * (1 + W))
        assert g == want, (name, g, want)


def test_drivers_keep_the_host_decoder_by_default():
    import inference
    import train
    assert train.build_parser().parse_args([]).png_decoder == "host"
    assert train.build_parser().parse_args(["--png_decoder", "gpu"]).png_decoder == "gpu"
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--png_decoder", "fast"])
    assert inference.take_png_decoder(["--scale", "2"]) == ("host", ["--scale", "2"])
    assert inference.take_png_decoder(["--png_decoder", "gpu", "--scale", "2"]) == ("gpu", ["--scale", "2"])
    assert inference.take_png_decoder(["--scale", "2", "--png_decoder=gpu"]) == ("gpu", ["--scale", "2"])
    with pytest.raises(SystemExit):
        inference.take_png_decoder(["--png_decoder", "fast"])
    with pytest.raises(SystemExit):
        inference.take_png_decoder(["--png_decoder"])
