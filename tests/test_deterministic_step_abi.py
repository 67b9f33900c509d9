"""CPU checks of the second stage of the deterministic training mode: the *_det entries of the token-path reductions (weight-
gradient GEMMs, column sums, LayerNorm backward) and their slab-size query are declared, bound and exported, the ABI version is
unchanged, the slab sizes are positive, repeatable and a function of their arguments only, and ops.deterministic_mode restores
the previous value."""
import ctypes
import os
import re

import pytest

from _abi import ABI          # tests/ is on sys.path (rootdir-less test modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DET_ENTRIES = ["tup_wgrad_slab", "tup_gemm_wgrad_bias_det", "tup_patch_wgrad_det", "tup_patch_wgrad_bf16_det",
               "tup_rt_patch_wgrad_det", "tup_wt_patch_wgrad_det", "tup_colsum_det", "tup_layernorm_bwd_det",
               "tup_layernorm128_bwd_det"]
# every atomic twin keeps its argument list; the deterministic form has `float* slab` before `stream`
TWINS = {"tup_gemm_wgrad_bias_det": "tup_gemm_wgrad_bias", "tup_patch_wgrad_det": "tup_patch_wgrad",
         "tup_patch_wgrad_bf16_det": "tup_patch_wgrad_bf16", "tup_rt_patch_wgrad_det": "tup_rt_patch_wgrad",
         "tup_wt_patch_wgrad_det": "tup_wt_patch_wgrad", "tup_colsum_det": "tup_colsum",
         "tup_layernorm_bwd_det": "tup_layernorm_bwd", "tup_layernorm128_bwd_det": "tup_layernorm128_bwd"}

KIND_GEMM, KIND_WIDE, KIND_COLSUM, KIND_LN = 0, 1, 2, 3
M3, MRT, M1 = 61440, 7200, 64          # config 3 (4 x 720p: 960 windows), ResidualTransformer x6 720p batch 2, one window
# (kind, M, NI, NJ)
REQUESTS = ([(KIND_GEMM, M3, ni, nj) for ni, nj in ((576, 192), (192, 192), (768, 192), (192, 768), (192, 4096))]
            + [(KIND_WIDE, M3, 192, 4096), (KIND_COLSUM, M3, 192, 0), (KIND_COLSUM, 4 * 720 * 1280, 64, 0), (KIND_LN, M3, 192, 0)]
            + [(KIND_GEMM, MRT, ni, nj) for ni, nj in ((384, 128), (128, 128), (512, 128), (128, 512), (128, 4096))]
            + [(KIND_COLSUM, MRT, 128, 0), (KIND_LN, MRT, 128, 0)]
            + [(KIND_GEMM, M1, 192, 192), (KIND_GEMM, M1, 192, 4096), (KIND_WIDE, M1, 192, 4096), (KIND_COLSUM, M1, 192, 0),
               (KIND_LN, M1, 192, 0), (KIND_LN, M1, 128, 0)])


def test_det_step_entries_are_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|long long)\s+(tup_\w+)\s*\(", hdr))
    for name in DET_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in DET_ENTRIES:
        assert hasattr(lib, name), name
    assert re.search(r"\blong long\s+tup_wgrad_slab\s*\(", hdr)
    assert _lib.RESTYPES["tup_wgrad_slab"] is ctypes.c_longlong is lib.tup_wgrad_slab.restype          # a count, not a hipError_t
    for det, twin in TWINS.items():
        a, b = _lib.SIGNATURES[det], _lib.SIGNATURES[twin]
        assert a[:-2] == b[:-1] and a[-2:] == [_lib.P, _lib.P], (det, twin)
    assert lib.tup_abi_version() == ABI == _lib.ABI_VERSION


@pytest.mark.parametrize("kind,M,NI,NJ", REQUESTS)
def test_wgrad_slab_is_positive_repeatable_and_a_function_of_its_arguments(kind, M, NI, NJ, monkeypatch):
    from transformerupscaler_amd import _lib, ops
    lib = _lib.load()
    n = lib.tup_wgrad_slab(kind, M, NI, NJ)
    assert n > 0
    # the tuning knobs of the diagnostic build must not reach the slicing (the product build does not read them at all)
    for knob in ("TUP_WGRAD_NO_XCD", "TUP_COLSUM_BLOCKS", "TUP_PATCH_WGRAD_FORM", "TUP_LN_BWD_BLOCKS"):
        monkeypatch.setenv(knob, "7")
    for other in REQUESTS[:3]:
        lib.tup_wgrad_slab(*other)          # no state carried from one request to the next
    assert lib.tup_wgrad_slab(kind, M, NI, NJ) == n == ops.wgrad_slab_floats(kind, M, NI, NJ)
    # whole slices: NI x NJ (+ NI column sums) per M slice, NI per row chunk, 2 x NI per LayerNorm workgroup
    per = {KIND_GEMM: NI * NJ + NI, KIND_WIDE: NI * NJ, KIND_COLSUM: NI, KIND_LN: 2 * NI}[kind]
    assert n % per == 0 and 1 <= n // per <= (M + 15) // 16
    if kind == KIND_LN:
        assert n // per <= 256


def test_wgrad_slab_refuses_invalid_requests():
    from transformerupscaler_amd import _lib, ops
    lib = _lib.load()
    assert lib.tup_wgrad_slab(4, M3, 192, 192) == 0 and lib.tup_wgrad_slab(-1, M3, 192, 192) == 0
    assert lib.tup_wgrad_slab(KIND_GEMM, M3, 100, 192) == 0 and lib.tup_wgrad_slab(KIND_GEMM, 0, 192, 192) == 0
    assert lib.tup_wgrad_slab(KIND_WIDE, M3, 128, 4096) == 0 and lib.tup_wgrad_slab(KIND_LN, M3, 64, 0) == 0
    with pytest.raises(ValueError):
        ops.wgrad_slab_floats(4, M3, 192, 192)


def test_deterministic_mode_restores_the_previous_value():
    from transformerupscaler_amd import ops
    assert ops.deterministic is False
    with ops.deterministic_mode():
        assert ops.deterministic_enabled()
        with ops.deterministic_mode(False):
            assert not ops.deterministic_enabled()
        assert ops.deterministic_enabled()
    assert ops.deterministic is False
    with pytest.raises(KeyError):
        with ops.deterministic_mode():
            raise KeyError("body")
    assert ops.deterministic is False
    ops.deterministic = True
    try:
        with ops.deterministic_mode(False):
            assert not ops.deterministic_enabled()
        assert ops.deterministic is True
    finally:
        ops.deterministic = False
