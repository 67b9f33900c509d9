"""CPU checks of the 4:2:0 JPEG round trip of the training degradations: the numpy statement tests/_degrade420_ref.py
against Pillow's subsampling=2 round trip, the stage's place in the chain, the flag's validation in `ops.degrade` ahead of any library
call, `data.DegradeSpec(jpeg_420_prob=...)`, the `tup_degrade_lr_sub` entry through header / binding / library, train.py's argument
rules, and csrc/jpeg_420.h on the host under the address and undefined-behaviour sanitizers.  Images are synthesised here."""
import ctypes
import functools
import glob
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _degrade420_ref as REF
import _degrade_ref as D
from _abi import ABI

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "transformerupscaler_amd", "csrc")
SIZES = ((1, 1), (2, 3), (3, 3), (5, 4), (4, 5), (7, 13), (17, 23), (20, 28), (21, 21), (33, 47), (40, 72), (96, 96))
QUALITIES = (5, 10, 30, 50, 75, 90, 95, 100)


@functools.lru_cache(maxsize=None)
def image(hw, kind):
    """uint8 [H][W][3]: a gradient plus a sinusoid plus mild noise ("smooth"), or random bytes ("random")."""
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    if kind == "random":
        a = rng.integers(0, 256, (h, w, 3))
    else:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([x * 255 // max(w - 1, 1), 128 + 100 * np.sin(x / 3.0 + y / 5.0), (y * 7 + x * 3) % 256], -1) + rng.integers(-20, 21, (h, w, 3))
    a = np.clip(a, 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


# ---- the 4:2:0 round trip is Pillow's ----
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("kind", ("smooth", "random"))
def test_jpeg_roundtrip_420_equals_pillow(hw, kind):
    Image = pytest.importorskip("PIL.Image")
    a = image(hw, kind)
    for q in QUALITIES:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=q, subsampling=2)
        pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        ref = REF.jpeg_roundtrip_420(a.transpose(2, 0, 1).astype(np.int64), q).transpose(1, 2, 0)
        assert ref.shape == pil.shape and int((ref != pil).sum()) == 0, (hw, kind, q)


def test_front_half_is_the_encoders():
    """The downsampled planes are the ones `_jpeg_ref.coefficients(frame, quality, 2)` transforms: same coefficients."""
    import _jpeg_ref as J
    for hw in ((7, 13), (17, 23), (33, 47)):
        a = image(hw, "random")
        blocks, _ = J.coefficients(a, 75, 2)
        _, Cb, Cr = REF.rgb_to_ycc(a.transpose(2, 0, 1))
        mine = J._fdct_quant(np.stack([REF.downsample(Cb), REF.downsample(Cr)]), D.quant_table(D.CHROMA, 75))
        assert np.array_equal(mine[0], blocks[:, :, 4]) and np.array_equal(mine[1], blocks[:, :, 5])


def test_narrow_rule_and_fancy_filter():
    import _jpeg_decode_ref as DEC
    p = np.random.default_rng(1).integers(0, 256, (5, 7))
    assert np.array_equal(REF.upsample(p, 10, 14), DEC.fancy_upsample(p)) and np.array_equal(REF.upsample(p, 9, 13), DEC.fancy_upsample(p)[:9, :13])
    for w in (1, 2):                                                                   # W <= 4: plain replication
        q = p[:, :w]
        assert np.array_equal(REF.upsample(q, 10, 2 * w), q.repeat(2, 0).repeat(2, 1))
        assert not np.array_equal(REF.upsample(q, 10, 2 * w), DEC.fancy_upsample(q))
    assert np.array_equal(REF.upsample(p[:, :3], 10, 5), DEC.fancy_upsample(p[:, :3])[:, :5])      # W = 5: the filter again


# ---- the stage in the chain ----
def test_420_differs_from_444_on_a_colour_edge():
    u = np.zeros((3, 32, 32), np.int64)
    u[0, :, :15], u[2, :, 15:] = 255, 255                                             # red | blue, the edge off the chroma grid
    a, b = D.jpeg_roundtrip(u, 95), REF.jpeg_roundtrip_420(u, 95)
    assert not np.array_equal(a, b)
    err = lambda v: np.abs(v - u)[:, :, 12:18].mean()
    assert err(b) > 2 * err(a)                                                         # the colour bleeds across the edge
    assert np.abs(b - u)[:, :, :8].mean() < 4 and np.abs(b - u)[:, :, 24:].mean() < 4  # ... and only there


def test_the_order_is_blur_noise_jpeg_and_the_flag_selects_the_sampling():
    x = np.random.default_rng(0).random((2, 3, 20, 28), dtype=np.float32) * 1.2 - 0.1
    full = (D.blur_taps(1.0), D.noise_amp(5), 3, 60, 1 | REF.FLAG_JPEG_420)
    u = D.quantise(x[0])
    want = REF.jpeg_roundtrip_420(D.noise(D.blur(u, full[0]), full[1], 3, True), 60)
    assert np.array_equal(REF.degrade_bytes(u, full), want)
    assert np.array_equal(REF.degrade_bytes(u, full[:4] + (1,)), D.degrade_bytes(u, full[:4] + (1,)))      # without the flag: 4:4:4, as before
    assert not np.array_equal(REF.degrade_bytes(u, full), D.degrade_bytes(u, full[:4] + (1,)))
    out = REF.degrade(x, [full, D.RECORD_OFF])
    assert out.dtype == np.float32 and np.array_equal(out[0], want.astype(np.float32) / np.float32(255))
    assert np.array_equal(out[1], D.quantise(x[1]).astype(np.float32) / np.float32(255))


def test_flag_checks_happen_before_any_library_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("a library call was reached")
    monkeypatch.setattr(_lib, "call", reached)
    monkeypatch.setattr(ops._RecordStager, "upload", reached)
    assert ops.DEGRADE_JPEG_420 == 4 == REF.FLAG_JPEG_420 and ops.DEGRADE_GREY_NOISE == 1
    x = torch.zeros((2, 3, 9, 11))
    good, taps = ops.DEGRADE_OFF, ops.blur_taps(1.0)
    for flags, quality in ((4, 1), (5, 1), (4, 100), (5, 50)):
        assert ops._degrade_record(1, (taps, 0, 0, quality, flags)) == taps + (0, 0, quality, flags)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                      # valid, on the CPU: refused after the checks, no call
            ops.degrade(x, [good, (taps, 0, 0, quality, flags)])
    for flags, quality in ((2, 50), (6, 50), (8, 50), (-1, 50), (4, 0), (5, 0)):
        with pytest.raises(ValueError, match="sample 1"):
            ops.degrade(x, [good, (taps, 0, 0, quality, flags)])
    with pytest.raises(ValueError, match="sample 0.*DEGRADE_JPEG_420.*quality 0"):
        ops.degrade(x, [(taps, 0, 0, 0, 4), good])
    assert ops._DEGRADE_REC.size == 32                                                  # the record keeps its layout


# ---- the spec and the sampler ----
def test_degrade_spec_jpeg_420_prob():
    from transformerupscaler_amd import data, ops
    default = data.DegradeSpec()
    assert default.jpeg_420_prob == 0.0
    assert default.as_dict() == {"blur_prob": 0.5, "blur_sigma": [0.2, 1.5], "noise_prob": 0.5, "noise_sigma": [1.0, 10.0],
                                 "grey_noise_prob": 0.4, "jpeg_prob": 0.7, "jpeg_quality": [30, 95]}
    assert "jpeg_420" not in repr(default) and data.DegradeSpec(jpeg_420_prob=0).as_dict() == default.as_dict()
    half = data.DegradeSpec(jpeg_420_prob=0.5)
    assert half.as_dict() == {**default.as_dict(), "jpeg_420_prob": 0.5} and "jpeg_420_prob=0.5" in repr(half)
    for bad in (-0.1, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError, match="jpeg_420_prob"):
            data.DegradeSpec(jpeg_420_prob=bad)
    always = data.DegradeSpec(jpeg_420_prob=1)
    stream = lambda g: np.random.default_rng([5, g, data.DEGRADE_STREAM])
    base = [default.draw(stream(g)) for g in range(300)]
    for spec in (always, half):
        recs = [spec.draw(stream(g)) for g in range(300)]
        assert [r[:4] for r in recs] == [r[:4] for r in base]                           # the ninth draw moves none of the eight
        assert [r[4] & 1 for r in recs] == [r[4] for r in base]
        for g, r in enumerate(recs):
            assert ops._degrade_record(g, r) == r[0] + r[1:]                            # every record passes the op's checks
            assert not (r[4] & 4 and r[3] == 0)
    assert all(bool(r[4] & 4) == (r[3] != 0) for r in (always.draw(stream(g)) for g in range(300)))
    on = [r for r in (half.draw(stream(g)) for g in range(300)) if r[3] != 0]
    share = sum(1 for r in on if r[4] & 4) / len(on)
    print(f"jpeg_420_prob 0.5: {len(on)} JPEG records of 300, flagged share {share:.3f}")
    assert abs(share - 0.5) < 0.1
    assert all(r[4] in (0, 1) for r in base)


def test_draw_is_untouched_by_the_spec(tmp_path):
    from PIL import Image
    from transformerupscaler_amd import data
    for i, hw in enumerate([(40, 64), (64, 40), (100, 120)]):
        Image.fromarray(np.full(tuple(hw) + (3,), 10 * i, np.uint8)).save(os.path.join(str(tmp_path), f"img_{i}.png"))
    kw = dict(patch=8, scales=(2, 4), seed=5, device="cpu")
    plain = data.PatchSampler(str(tmp_path), **kw)
    s = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(jpeg_420_prob=1), **kw)
    old = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(), **kw)
    assert [s.draw(g) for g in range(200)] == [plain.draw(g) for g in range(200)]
    assert [s.draw_degrade(g)[:4] for g in range(200)] == [old.draw_degrade(g)[:4] for g in range(200)]
    assert any(s.draw_degrade(g)[4] & 4 for g in range(20))


# ---- build and ABI ----
def test_entry_is_declared_bound_exported_and_guarded():
    from transformerupscaler_amd import _lib, ops
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tupscale_hip.h")).read())
    assert "int tup_degrade_lr_sub(const float* in, const void* recs, int B, int H, int W, float* out, void* stream);" in header
    P, I = _lib.P, _lib.I
    assert _lib.SIGNATURES["tup_degrade_lr_sub"] == [P, P, I, I, I, P, P] == _lib.SIGNATURES["tup_degrade_lr"]
    assert _lib.ABI_VERSION == ABI                                                      # a new entry, the same ABI number
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tup_degrade_lr_sub") and hasattr(lib, "tup_degrade_lr") and lib.tup_abi_version() == ABI
    assert _lib.load() is not None
    guard = open(os.path.join(CSRC, "check_resources.py")).read()
    assert '("degrade420.hip", ["degrade_sub_kernel"])' in guard and '("degrade.hip", ["degrade_lr_kernel"])' in guard
    src = open(os.path.join(CSRC, "degrade420.hip")).read()
    assert "degrade_lr_kernel<<<" not in src and len(re.findall(r"__global__", src)) == 1                  # one kernel, one launch
    assert '#include "jpeg_420.h"' in src and "atomic" not in src.split("#include")[1]
    shared = open(os.path.join(CSRC, "jpeg_420.h")).read()
    assert all(name in shared for name in ("j420_down_src", "j420_down", "j420_narrow", "j420_up_src", "j420_up"))
    assert "jpeg_420.h" in re.search(r"^HDRS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    usage = os.path.join(CSRC, "build", "resource_usage.json")
    if os.path.exists(usage):                                                           # written by the build
        kernels = json.load(open(usage))["kernels"]
        mine = {k: v for k, v in kernels.items() if "degrade_sub_kernel" in k}
        assert len(mine) == 1 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] and v["source"] == "degrade420.hip" for v in mine.values())
        assert len([k for k in kernels if "degrade_lr_kernel" in k]) == 1
    assert "tup_degrade_lr_sub" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_entry_refuses_bad_arguments_before_it_launches():
    from transformerupscaler_amd import _lib
    fn = _lib.load().tup_degrade_lr_sub
    invalid = 1                                         # hipErrorInvalidValue
    buf = (ctypes.c_float * (2 * 3 * 8 * 8 * 2))()      # host memory: never dereferenced by a refused call
    a = ctypes.addressof(buf)
    n = 2 * 3 * 8 * 8 * 4                               # bytes of one [2][3][8][8] tensor
    recs = a                                            # any non-null pointer
    assert fn(None, recs, 2, 8, 8, a + n, None) == invalid
    assert fn(a, None, 2, 8, 8, a + n, None) == invalid
    assert fn(a, recs, 2, 8, 8, None, None) == invalid
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, 0), (2, -8, 8), (65536, 8, 8)):
        assert fn(a, recs, B, H, W, a + n, None) == invalid
    assert fn(a, recs, 2, 8, 8, a, None) == invalid                     # out is in
    assert fn(a, recs, 2, 8, 8, a + n - 4, None) == invalid             # out overlaps in's last element
    assert fn(a + n - 4, recs, 2, 8, 8, a, None) == invalid             # ... and the other way round


# ---- the driver's argument rules ----
def _refused(argv):
    import train
    with pytest.raises(SystemExit) as e:
        train.main(argv)
    assert isinstance(e.value.code, str)                # a message, not a status: nothing ran
    return e.value.code


def test_train_py_degrade_jpeg_420_argument_rules(tmp_path):
    import train
    d = str(tmp_path)
    assert "need --patch_size" in _refused(["--data_dir", d, "--degrade_jpeg_420", "0.5"])
    base = ["--data_dir", d, "--patch_size", "16"]
    for v in ("x", "1.5", "-0.1", "0.5,0.5", "nan", ""):
        if v:
            assert "--degrade_jpeg_420" in _refused(base + [f"--degrade_jpeg_420={v}"]), v      # "=": a value may start with a minus sign
    parse = train.build_parser().parse_args
    assert train.degrade_options(parse(base)) is None
    assert train.degrade_options(parse(base + ["--degrade"])) == {}                              # the default stays 0
    assert train.degrade_options(parse(base + ["--degrade_jpeg_420", "0.25"])) == {"jpeg_420_prob": 0.25}      # implies --degrade
    assert train.degrade_options(parse(base + ["--degrade_jpeg_420", "0"])) == {"jpeg_420_prob": 0.0}
    assert train.degrade_options(parse(base + ["--degrade_prob", "1,0,1", "--degrade_jpeg_420", "1"])) == {
        "blur_prob": 1.0, "noise_prob": 0.0, "jpeg_prob": 1.0, "jpeg_420_prob": 1.0}
    assert "--degrade_jpeg_420" in train.__doc__


# ---- csrc/jpeg_420.h on the host, under the sanitizers ----
def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(c) and glob.glob(os.path.join(os.path.dirname(os.path.dirname(c)), "lib", "clang", "*", "lib", "linux", "*asan*")):
            return c
    return None


@pytest.fixture(scope="module")
def halves(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm clang++ with a host address-sanitizer runtime found")
    exe = str(tmp_path_factory.mktemp("degrade420") / "degrade420_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "degrade420_main.cpp"), "-o", exe], check=True)

    def run(full, real):
        H, W = full.shape
        with open(exe + ".in", "wb") as fh:
            fh.write(np.array([H, W], np.int32).tobytes() + full.astype(np.uint8).tobytes() + real.astype(np.uint8).tobytes())
        p = subprocess.run([exe, exe + ".in", exe + ".out"], capture_output=True, text=True)      # a plain child process
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        raw = np.fromfile(exe + ".out", dtype=np.uint8)
        dh, dw = (H + 15) // 16 * 8, (W + 15) // 16 * 8
        assert raw.size == dh * dw + H * W
        return raw[:dh * dw].reshape(dh, dw).astype(np.int64), raw[dh * dw:].reshape(H, W).astype(np.int64)
    return run


@pytest.mark.parametrize("hw", SIZES + ((3, 4), (16, 16), (32, 64), (64, 65)))
def test_host_halves_equal_the_reference(halves, hw):
    H, W = hw
    rng = np.random.default_rng(H * 77 + W)
    for q in (5, 100):
        u = image(hw, "random").transpose(2, 0, 1).astype(np.int64)
        _, Cb, _ = REF.rgb_to_ycc(u)
        _, cb, _ = REF.decoded_planes(u, q)                                             # what a decoder holds: the real samples
        down, up = halves(Cb, cb)
        assert np.array_equal(down, REF.downsample(Cb)), (hw, q)
        assert np.array_equal(up, REF.upsample(cb, H, W)), (hw, q)
    extreme = rng.integers(0, 2, (H, W)) * 255                                          # the rounding biases at both ends of the range
    down, up = halves(extreme, extreme[::2, ::2])
    assert np.array_equal(down, REF.downsample(extreme)) and np.array_equal(up, REF.upsample(extreme[::2, ::2], H, W))
