"""TEST INFRASTRUCTURE ONLY -- the images and parameter sets shared by tests/test_jpeg_cpu.py and tests/test_hip_jpeg.py, and the
reference files of tests/_jpeg_ref.py computed once per case."""
import functools
import io

import numpy as np

import _jpeg_ref as REF

# what one workgroup of csrc/jpeg_encode.hip codes at a time: 96 blocks = 16 MCUs of 4:2:0 (256 pixels of a row) or 32 of 4:4:4 (256 too)
CHUNK_BLOCKS = 96
CHUNK_PIXELS = 256
WIDE = (16, 1000)                       # 16 rows; 63 / 125 MCUs a row: four / five chunks, the last one partial
SIZES = ((1, 1), (7, 13), (16, 16), (17, 23), (33, 16), (40, 72), WIDE)
KINDS = ("smooth", "noise", "flat0", "flat255")


@functools.lru_cache(maxsize=None)
def image(hw, kind):
    """uint8 [H][W][3], read-only.  smooth: gradients, a sinusoid and mild noise; noise: random bytes; checker: 8 x 8 blocks that
    alternate between dark and bright noise (DC differences of the largest size category); flat0 / flat255."""
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w + len(kind))
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3))
    elif kind == "checker":
        a = (((y // 8 + x // 8) & 1) * 215)[..., None] + rng.integers(0, 41, (h, w, 3))
    elif kind == "smooth":
        a = np.stack([x * 255 // max(w - 1, 1), 128 + 100 * np.sin(x / 3.0 + y / 5.0), (y * 7 + x * 3) % 256], -1) + rng.integers(-20, 21, (h, w, 3))
    else:
        a = np.full((h, w, 3), {"flat0": 0, "flat255": 255}[kind])
    a = np.clip(a, 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(hw, kind, quality, sub, restart_rows):
    """(file bytes, coder statistics) of tests/_jpeg_ref.py for one case."""
    stats = {}
    data = REF.encode(image(hw, kind), quality, sub, restart_rows, stats)
    return data, stats


def pillow(a, quality, sub, restart_rows):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.asarray(a)).save(buf, "JPEG", quality=quality, subsampling=sub, restart_marker_rows=restart_rows)
    return buf.getvalue()


def cases():
    """(hw, kind, quality, subsampling, restart_rows): every size with both subsamplings, the three qualities and the three restart
    settings spread over the contents, so that each value of each parameter meets each size at least once."""
    out = []
    for si, hw in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            if hw == WIDE and kind.startswith("flat"):
                continue
            for sub in (0, 2):
                for qi, q in enumerate((5, 75, 100)):
                    r = (1, 2, 50)[(si + ki + qi + sub // 2) % 3]
                    out.append((hw, kind, q, sub, r))
    out += [((40, 72), "checker", 100, 0, 1), ((40, 72), "checker", 100, 2, 2), ((17, 23), "checker", 100, 2, 1)]
    return out
