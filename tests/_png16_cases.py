"""TEST INFRASTRUCTURE ONLY -- the 16-bit images and parameter sets shared by tests/test_png16_cpu.py and tests/test_hip_png16.py, and
the reference files of tests/_png16_ref.py computed once per case.

Sizes (H, W), a row being 1 + 6 W filtered bytes: (1, 1) one pixel, 7 bytes; (1, 7) one row; (5, 1) rows of one pixel, where "left" never
exists; (3, 5) 93 bytes; (40, 72) 17 320 bytes: 68 / 17 / 2 / 1 blocks of 256 / 1024 / 16384 / 32768, rows of 433 bytes that straddle every
cut; (64, 683) 262 336 bytes, rows of 4099: 1025 blocks of 256 (five sweeps of the scan kernel), 9 of 32768."""
import functools

import numpy as np

import _png16_ref as REF

SMALL = ((1, 1), (1, 7), (5, 1), (3, 5), (40, 72))
BIG = (64, 683)
SIZES = SMALL + (BIG,)
KINDS = ("noise", "flat0", "flat65535", "lowbyte", "ramp")
BLOCKS = (256, 1024, 16384, 32768)
FILTERS = ("adaptive", "none", "sub", "up", "average", "paeth")


@functools.lru_cache(maxsize=None)
def image(hw, kind):
    """uint16 [H][W][3], read-only.  "lowbyte": every sample is 0x80xx with a random low byte, so a writer that keeps only high bytes,
    or swaps the two, shows (Pillow's 8-bit view of such a file is flat).  "ramp": smooth in x, y and channel, crossing many high bytes."""
    h, w = hw
    rng = np.random.default_rng(h * 100003 + w * 101 + len(kind))
    if kind == "noise":
        a = rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)
        a.reshape(-1)[[0, -1]] = (0, 65535)
    elif kind == "flat0":
        a = np.zeros((h, w, 3), np.uint16)
    elif kind == "flat65535":
        a = np.full((h, w, 3), 65535, np.uint16)
    elif kind == "lowbyte":
        a = (0x8000 + rng.integers(0, 256, (h, w, 3))).astype(np.uint16)
    elif kind == "ramp":
        y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
        a = ((x * 61 + y * 977 + c * 4099 + 300) % 65536).astype(np.uint16)
    else:
        raise KeyError(kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(hw, kind, block_bytes, filter):
    """(file bytes, coder statistics) of tests/_png16_ref.py for one case"""
    stats = {}
    data = REF.encode(image(hw, kind), block_bytes, filter, stats)
    return data, stats


@functools.lru_cache(maxsize=None)
def cases():
    """(hw, kind, block_bytes, filter).  Every small size with every kind and every block size, the six filters in turn (so each meets
    every size and kind and several block sizes); the big size, whose Python reference is slow, with one case per kind that between them
    take every block size and five filters."""
    out, i = [], 0
    for hw in SMALL:
        for kind in KINDS:
            for bb in BLOCKS:
                out.append((hw, kind, bb, FILTERS[i % 6]))
                i += 1
            i += 1                                           # 4 block sizes and 6 filters: shift, so that a kind does not pin a filter
    out += [(BIG, "noise", 256, "adaptive"), (BIG, "ramp", 16384, "paeth"), (BIG, "lowbyte", 32768, "sub"), (BIG, "flat65535", 1024, "up"),
            (BIG, "flat0", 32768, "average"), (BIG, "ramp", 1024, "adaptive")]
    # every filter on the image whose rows straddle the cuts, at the two middle block sizes
    out += [((40, 72), "ramp", bb, f) for f in FILTERS for bb in (1024, 16384)]
    return tuple(dict.fromkeys(out))
