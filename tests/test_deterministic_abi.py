"""CPU checks of the deterministic training mode's surface: the *_det entries and the slab-size query are declared, bound and
exported, the ABI version is unchanged, the slab sizes are positive and repeatable, and ops.deterministic is explicit-only."""
import ctypes
import os
import re

import pytest
import torch

from _abi import ABI          # tests/ is on sys.path (rootdir-less test modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DET_ENTRIES = ["tup_conv_wgrad_slab", "tup_slab_reduce", "tup_conv3x3_c64_wgrad_det", "tup_conv3x3_c64_wgrad_s2d_det",
               "tup_conv3x3_thin_wgrad_det", "tup_conv3x3_planar_wgrad_det"]

# (B, H, W): config 3's maps (4 x 720p), ResidualTransformer's 720p training map, and an odd B = 1 shape
SHAPES = [(4, 720, 1280), (2, 720, 1280), (1, 36, 44)]


def test_det_entries_are_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|long long)\s+(tup_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in DET_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"\blong long\s+tup_conv_wgrad_slab\s*\(", hdr)
    assert _lib.RESTYPES["tup_conv_wgrad_slab"] is ctypes.c_longlong is lib.tup_conv_wgrad_slab.restype          # a count, not a hipError_t
    assert lib.tup_abi_version() == ABI == _lib.ABI_VERSION


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_slab_sizes_are_positive_repeatable_and_what_the_wrappers_allocate(B, H, W):
    from transformerupscaler_amd import _lib, ops
    lib = _lib.load()
    # the grids: one persistent workgroup per CU (c64), two (thin; planar r <= 2) or four (planar r >= 3), capped by the tile count
    tiles8 = ((W + 31) // 32) * ((H + 7) // 8) * B
    expect = {(0, 1): min(tiles8, 256) * (64 * 9 * 64 + 64), (1, 1): min(tiles8, 512) * (3 * 9 * 64 + 12)}
    for r, th, per_cu in ((1, 32, 2), (2, 16, 2), (3, 4, 4)):
        expect[(2, r)] = min(((W + 31) // 32) * ((H + th - 1) // th) * B, 256 * per_cu) * 3 * r * r * 28
    for (kind, r), n in expect.items():
        got = lib.tup_conv_wgrad_slab(kind, B, H, W, r)
        assert got == lib.tup_conv_wgrad_slab(kind, B, H, W, r) == n, (kind, r, got, n)
        assert ops.conv_wgrad_slab_floats(kind, B, H, W, r) == n
    assert lib.tup_conv_wgrad_slab(2, B, H, W, 7) == 0
    with pytest.raises(ValueError):
        ops.conv_wgrad_slab_floats(3, B, H, W)


def test_deterministic_attribute_is_explicit_only():
    """Only part of the backward has deterministic forms, so the mode must not switch on with torch's flag (a user would get
    different kernels but still a non-reproducible step): ops.deterministic alone decides."""
    from transformerupscaler_amd import ops
    assert ops.deterministic is False
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert not ops.deterministic_enabled()
        ops.deterministic = True
        assert ops.deterministic_enabled()
        torch.use_deterministic_algorithms(False)
        assert ops.deterministic_enabled()
        ops.deterministic = False
        assert not ops.deterministic_enabled()
    finally:
        ops.deterministic = False
        torch.use_deterministic_algorithms(was, warn_only=warn)
