"""TEST INFRASTRUCTURE ONLY -- the images and parameter sets shared by tests/test_png_cpu.py and tests/test_hip_png.py, and the reference
files of tests/_png_ref.py computed once per case."""
import functools

import numpy as np

import _jpeg_cases as J
import _png_ref as REF

# (1, 1): a block of 4 bytes; (17, 23) is 1190 bytes: five blocks of 256; every row of (16, 1000) is 3001 bytes: split over three blocks
# of 1024; (3, 4000) is 36003 bytes: cut once by 32768, in the middle of its last row
SIZES = ((1, 1), (1, 7), (7, 13), (17, 23), (33, 16), (40, 72), (16, 1000), (3, 4000))
KINDS = ("smooth", "noise", "flat0", "flat255", "checker")
BLOCKS = (256, 1024, 32768)
FIXED = ("none", "sub", "up", "average", "paeth")
DEEP = (8, 740)                         # 8 x 2221 = 17768 filtered bytes: one block of 32768
MANY = (64, 350)                        # 67264 bytes = 263 blocks of 256: more blocks than the scan kernel takes in one sweep of 256
EXTRA = (DEEP, MANY)


@functools.lru_cache(maxsize=None)
def image(hw, kind):
    """uint8 [H][W][3], read-only.  The kinds of tests/_jpeg_cases.py, and "deep" (for filter "none"): an image whose one block has a
    Fibonacci histogram, 1, 1, 2, 3, 5, 8, ... 4181, 6765, so that its minimum-redundancy code is 19 bits deep and the 15-bit limit acts.
    The histogram is the block's, not the pixels': end-of-block is the first 1 and the eight filter bytes (value 0) are the 8, so byte
    value k = 1..19 occurs F(k + 1) times with F(6) = 8 left out, and the 59 bytes that 8 x 740 x 3 has beyond that sum go to value
    19.  (Value k occurring F(k) times, k = 1..20, gives a code of only 11 bits once end-of-block and the filter bytes join: three
    counts of 1 and two of 8 split the chain.)  Ordered so that no two neighbours are equal: no match anywhere."""
    if kind != "deep":
        return J.image(hw, kind)
    assert hw == DEEP
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    counts = {k: fib[k] for k in range(1, 20) if fib[k] != 8}
    counts[19] += hw[0] * hw[1] * 3 - sum(counts.values())
    values = np.concatenate([np.full(c, k, np.uint8) for k, c in counts.items()])
    assert len(values) == hw[0] * hw[1] * 3 and counts[19] == 6765 + 59
    values = np.sort(values)[::-1]
    half = (len(values) + 1) // 2
    a = np.empty(len(values), np.uint8)
    a[0::2] = values[:half]
    a[1::2] = values[half:]
    assert (a[1:] != a[:-1]).all()
    a = a.reshape(hw + (3,))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(hw, kind, block_bytes, filter):
    """(file bytes, coder statistics) of tests/_png_ref.py for one case"""
    stats = {}
    data = REF.encode(image(hw, kind), block_bytes, filter, stats)
    return data, stats


@functools.lru_cache(maxsize=None)
def cases():
    """(hw, kind, block_bytes, filter): every size with every kind and every block size; adaptive filtering for half of them and the
    five fixed filters spread over the other half, so that each fixed filter meets several sizes, kinds and block sizes."""
    out = []
    i = 0
    for hw in SIZES:
        for kind in KINDS:
            for bb in BLOCKS:
                out.append((hw, kind, bb, "adaptive" if i % 2 == 0 else FIXED[(i // 2) % 5]))
                i += 1
    for bb in BLOCKS:
        out.append((DEEP, "deep", bb, "none"))
    # every fixed filter across a row split over blocks, a cut inside a row, and the smallest image
    for f in FIXED:
        out += [((16, 1000), "smooth", 1024, f), ((3, 4000), "checker", 32768, f), ((1, 1), "noise", 256, f), ((17, 23), "smooth", 256, f)]
    out += [(MANY, "smooth", 256, "adaptive"), (MANY, "flat255", 256, "sub"),
            ((17, 23), "smooth", 256, "adaptive"), ((16, 1000), "smooth", 1024, "adaptive"), ((3, 4000), "smooth", 32768, "adaptive"),
            ((40, 72), "smooth", 300, "adaptive"), ((40, 72), "checker", 32767, "paeth")]
    return tuple(dict.fromkeys(out))
