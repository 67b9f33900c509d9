"""TEST INFRASTRUCTURE ONLY -- the files shared by tests/test_jpeg_decode_cpu.py and tests/test_hip_jpeg_decode.py beyond those of
tests/_jpeg_cases.py: Pillow's files with other settings, and damaged scans made from one good file."""
import functools
import io
import struct

import numpy as np

import _jpeg_cases as C
import _jpeg_ref as REF

EOI = b"\xff\xd9"


def save(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.asarray(a)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def repack_dqt(data):
    """The same file with its DQT segments merged into one that carries every table."""
    i, out, tables, at = 2, bytearray(data[:2]), b"", None
    while True:
        m, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if m == 0xDB:
            tables += data[i + 4:i + 2 + length]
            at = len(out) if at is None else at
        else:
            out += data[i:i + 2 + length]
        i += 2 + length
        if m == 0xDA:
            break
    merged = b"\xff\xdb" + (len(tables) + 2).to_bytes(2, "big") + tables
    return bytes(out[:at]) + merged + bytes(out[at:]) + data[i:]


@functools.lru_cache(maxsize=None)
def extra_files():
    """(name, file bytes): segments that begin mid-row, custom Huffman tables, one component, EXIF and COM, two tables in one DQT."""
    out = []
    for sub in (0, 2):
        out.append((f"blocks5-40x72-{sub}", save(C.image((40, 72), "smooth"), quality=75, subsampling=sub, restart_marker_blocks=5)))
        out.append((f"blocks1-17x23-{sub}", save(C.image((17, 23), "noise"), quality=75, subsampling=sub, restart_marker_blocks=1)))
        for hw, kind, q in (((40, 72), "smooth", 75), ((17, 23), "noise", 100), ((16, 1000), "smooth", 75)):
            out.append((f"optimize-{hw[0]}x{hw[1]}-{sub}", save(C.image(hw, kind), quality=q, subsampling=sub, optimize=True, restart_marker_rows=1)))
    for hw in ((1, 1), (17, 23), (40, 72)):
        out.append((f"grey-{hw[0]}x{hw[1]}", save(C.image(hw, "smooth")[..., 1], quality=75, restart_marker_rows=hw[0] // 20)))
    from PIL import Image
    exif = Image.Exif()
    exif[0x010E] = "a description"
    out.append(("exif-com", save(C.image((17, 23), "smooth"), quality=75, exif=exif.tobytes(), comment=b"a comment")))
    out.append(("dqt-merged", repack_dqt(save(C.image((40, 72), "smooth"), quality=75))))
    return tuple(out)


def program_input(info, scan, record):
    """What tests/jpeg_entropy_main.cpp reads: the geometry, the image record (`record(info, file, scan_off)` = ops._jpeg_decode_record)
    and the scan."""
    layout = {"4:4:4": 0, "4:2:0": 2, "grey": 4}[info["subsampling"]]
    info = dict(info, scan=(0, len(scan)))
    return struct.pack("<4i", info["H"], info["W"], layout, info["restart_interval"]) + record(info, scan, 0) + bytes(scan)


def strip_restart_markers(scan):
    out, i = bytearray(), 0
    while i < len(scan):
        if scan[i] == 0xFF and i + 1 < len(scan) and 0xD0 <= scan[i + 1] <= 0xD7:
            i += 2
        else:
            out.append(scan[i])
            i += 1
    return bytes(out)


@functools.lru_cache(maxsize=None)
def good():
    """The 40 x 72 file the damaged ones are made from: 4:2:0, a restart marker per MCU row."""
    return C.pillow(C.image((40, 72), "smooth"), 75, 2, 1)


@functools.lru_cache(maxsize=None)
def damaged():
    """(name, head, scan, restart interval): the head is the good file's up to SOS (for "no-dri" without its DRI segment)."""
    head, scan = REF.split(good())
    interval = 5
    out = [(f"cut-{t}", head, scan[:t], interval) for t in range(0, len(scan), 7)]
    rng = np.random.default_rng(7)
    for p, v in zip(rng.integers(0, len(scan), 64), rng.integers(0, 256, 64)):
        out.append((f"byte-{int(p)}-{int(v)}", head, scan[:p] + bytes([int(v)]) + scan[p + 1:], interval))
    out.append(("no-markers", head, strip_restart_markers(scan), interval))
    dri = head.index(b"\xff\xdd\x00\x04")
    out.append(("no-dri", head[:dri] + head[dri + 6:], scan, 0))
    return tuple(out)


def gpu_damaged(parse):
    """The handful the GPU test runs beside a good image: two truncations, two byte changes, the file without its markers; all of them
    files `parse` (ops.jpeg_parse) takes, as every one of them walked under the sanitizers on the host."""
    picked, want = [], {"cut": 2, "byte": 2}
    cases = damaged()
    for name, head, scan, _ in cases[len(cases) // 9::5]:
        kind = name.split("-")[0]
        if want.get(kind, 0) == 0:
            continue
        data = head + scan + EOI
        try:
            parse(data)
        except ValueError:
            continue
        want[kind] -= 1
        picked.append((name, data))
    for name, head, scan, _ in cases:
        if name == "no-markers":
            picked.append((name, head + scan + EOI))
    return picked
