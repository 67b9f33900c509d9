"""CPU checks of the training degradations: the numpy statement tests/_degrade_ref.py against Pillow's 4:4:4 JPEG round
trip, the blur taps and the noise statistics, `data.DegradeSpec` and `PatchSampler.draw_degrade` as a pure function on a stream of
its own, `ops.degrade`'s validation ahead of any library call, the `tup_degrade_lr` entry through header / binding / library, and
train.py's argument rules.  Images are synthesised here."""
import ctypes
import functools
import io
import os
import re

import numpy as np
import pytest
import torch

import _degrade_ref as REF
from _abi import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((96, 96), (20, 28), (7, 13), (21, 21))
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


# ---- the JPEG stage is Pillow's ----
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("kind", ("smooth", "random"))
def test_jpeg_roundtrip_equals_pillow(hw, kind):
    Image = pytest.importorskip("PIL.Image")
    a = image(hw, kind)
    for q in QUALITIES:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=q, subsampling=0)
        pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        ref = REF.jpeg_roundtrip(a.transpose(2, 0, 1).astype(np.int64), q).transpose(1, 2, 0)
        assert ref.shape == pil.shape and int((ref != pil).sum()) == 0, (hw, kind, q)
    assert not np.array_equal(REF.jpeg_roundtrip(a.transpose(2, 0, 1), 30), a.transpose(2, 0, 1))     # ... and it does something


def test_quantiser_tables():
    assert REF.quant_table(REF.LUMA, 50).tolist() == REF.LUMA.tolist()                      # quality 50 is Annex K itself
    assert REF.quant_table(REF.CHROMA, 100).tolist() == [[1] * 8] * 8
    assert REF.quant_table(REF.LUMA, 1).max() == 255 and REF.quant_table(REF.LUMA, 5)[0, 0] == 160


# ---- blur ----
def test_blur_taps_sum_symmetry_identity_and_constants():
    from transformerupscaler_amd import ops
    assert ops.blur_taps(0) == ops.DEGRADE_TAPS_OFF == REF.TAPS_OFF == (1 << 22, 0, 0, 0)
    for sigma in (0.05, 0.2, 0.5, 0.8, 1.0, 1.5, 2.0, ops.DEGRADE_MAX_BLUR_SIGMA):
        k = ops.blur_taps(sigma)
        assert k == REF.blur_taps(sigma)
        assert len(k) == 4 and all(type(v) is int and v >= 0 for v in k)
        assert k[0] + 2 * (k[1] + k[2] + k[3]) == 1 << 22                                   # the seven taps {k3 k2 k1 k0 k1 k2 k3} sum to one
        assert k[0] >= k[1] >= k[2] >= k[3]
    assert ops.blur_taps(1.5)[3] > 0 and ops.blur_taps(0.05) == (1 << 22, 0, 0, 0)
    for bad in (-0.1, 3.01, float("nan")):
        with pytest.raises(ValueError):
            ops.blur_taps(bad)
    u = image((20, 28), "random").transpose(2, 0, 1).astype(np.int64)
    assert np.array_equal(REF.blur(u, REF.TAPS_OFF), u)                                     # off: an exact identity
    for sigma in (0.5, 1.5, 3.0):
        for v in (0, 1, 77, 254, 255):
            const = np.full((3, 9, 11), v, np.int64)
            assert np.array_equal(REF.blur(const, REF.blur_taps(sigma)), const)             # edge replication keeps a constant
    b = REF.blur(u, REF.blur_taps(1.5))
    assert b.min() >= 0 and b.max() <= 255 and b.std() < 0.7 * u.std()
    # the horizontal pass comes first and is rounded: the transposed order differs by single LSBs somewhere
    bt = REF.blur(u.transpose(0, 2, 1), REF.blur_taps(1.5)).transpose(0, 2, 1)
    assert 0 < np.abs(b - bt).max() <= 1


# ---- noise ----
def test_noise_statistics_grey_and_hash():
    from transformerupscaler_amd import ops
    import test_hip_dropout
    idx = np.arange(5000) * 977
    assert np.array_equal(REF.drop_hash(12345, idx), test_hip_dropout.drop_hash(12345, idx))
    assert ops.noise_amp(0) == 0 == REF.noise_amp(0)
    with pytest.raises(ValueError):
        ops.noise_amp(-1)
    n = REF.noise_values(99, 96, 96, False)
    assert n.min() >= -510 and n.max() <= 510 and abs(n.std() - 147.80) < 0.03 * 147.80
    u = np.full((3, 96, 96), 128, np.int64)
    for sigma in (2, 8):
        amp = ops.noise_amp(sigma)
        assert amp == REF.noise_amp(sigma) == round(sigma * 65536 / 147.80054)
        d = REF.noise(u, amp, 12345, False) - 128
        print(f"sigma {sigma}: mean {d.mean():.4f} std {d.std():.4f}")
        assert abs(d.mean()) <= 0.1
        assert abs(d.std() / np.sqrt(sigma ** 2 + 1 / 12) - 1) <= 0.03                      # + 1/12: the rounding to integers
    colour = REF.noise(u, ops.noise_amp(8), 7, False)
    grey = REF.noise(u, ops.noise_amp(8), 7, True)
    assert np.array_equal(grey[0], grey[1]) and np.array_equal(grey[0], grey[2])
    assert not np.array_equal(colour[0], colour[1]) and not np.array_equal(grey[0], colour[0])
    assert np.array_equal(REF.noise(u, 0, 7, False), u)
    assert not np.array_equal(REF.noise(u, ops.noise_amp(8), 8, False), colour)             # another seed, another field
    assert REF.noise(np.zeros((3, 8, 8), np.int64), ops.noise_amp(40), 1, False).min() == 0  # clipped


# ---- the chain ----
def test_identity_record_returns_the_quantised_input():
    from transformerupscaler_amd import ops
    assert ops.DEGRADE_OFF == REF.RECORD_OFF
    x = np.random.default_rng(0).random((2, 3, 20, 28), dtype=np.float32) * 1.2 - 0.1
    out = REF.degrade(x, [REF.RECORD_OFF] * 2)
    assert out.dtype == np.float32 and np.array_equal(out, REF.quantise(x).astype(np.float32) / np.float32(255))
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(REF.quantise(k), np.arange(256))                                  # patch_pairs' values come back exactly
    full = (REF.blur_taps(1.0), REF.noise_amp(5), 3, 60, 1)
    a, b = REF.degrade(x, [full, REF.RECORD_OFF]), REF.degrade(x, [REF.RECORD_OFF, full])
    assert np.array_equal(a[1], out[1]) and np.array_equal(b[0], out[0]) and not np.array_equal(a[0], out[0])
    # the order is blur, noise, JPEG: the JPEG stage sees the noisy image
    u = REF.quantise(x[0])
    assert np.array_equal(REF.degrade_bytes(u, full), REF.jpeg_roundtrip(REF.noise(REF.blur(u, full[0]), full[1], 3, True), 60))


# ---- the spec and the sampler ----
def test_degrade_spec_validation():
    from transformerupscaler_amd import data
    spec = data.DegradeSpec()
    assert spec.as_dict() == {"blur_prob": 0.5, "blur_sigma": [0.2, 1.5], "noise_prob": 0.5, "noise_sigma": [1.0, 10.0],
                              "grey_noise_prob": 0.4, "jpeg_prob": 0.7, "jpeg_quality": [30, 95]}
    for kw, word in (({"blur_prob": 1.5}, "blur_prob"), ({"noise_prob": -0.1}, "noise_prob"), ({"jpeg_prob": "x"}, "jpeg_prob"),
                     ({"grey_noise_prob": 2}, "grey_noise_prob"), ({"blur_sigma": (1.0, 0.5)}, "blur_sigma"),
                     ({"blur_sigma": (0.2, 3.5)}, "blur_sigma"), ({"blur_sigma": 1.0}, "blur_sigma"), ({"noise_sigma": (-1, 2)}, "noise_sigma"),
                     ({"noise_sigma": (1, 2, 3)}, "noise_sigma"), ({"jpeg_quality": (0, 50)}, "jpeg_quality"),
                     ({"jpeg_quality": (50, 101)}, "jpeg_quality"), ({"jpeg_quality": (60, 50)}, "jpeg_quality"),
                     ({"jpeg_quality": (30.5, 95)}, "jpeg_quality")):
        with pytest.raises(ValueError, match=word):
            data.DegradeSpec(**kw)


def _write_pngs(d, sizes):
    from PIL import Image
    for i, hw in enumerate(sizes):
        Image.fromarray(np.full(tuple(hw) + (3,), 10 * i, np.uint8)).save(os.path.join(d, f"img_{i}.png"))


def test_draw_degrade_is_pure_and_leaves_draw_alone(tmp_path):
    from transformerupscaler_amd import data, ops
    _write_pngs(str(tmp_path), [(40, 64), (64, 40), (100, 120)])
    kw = dict(patch=8, scales=(2, 4), seed=5, device="cpu")
    plain = data.PatchSampler(str(tmp_path), **kw)
    s = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(), **kw)
    again = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(), **kw)
    other = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(), **dict(kw, seed=6))
    assert plain.degrade is None and plain.draw_degrade(3) is None
    assert [s.draw(g) for g in range(300)] == [plain.draw(g) for g in range(300)]           # a stream of its own
    recs = [s.draw_degrade(g) for g in range(300)]
    assert recs == [again.draw_degrade(g) for g in range(300)]
    assert recs[::-1] == [s.draw_degrade(g) for g in reversed(range(300))]                  # no state: any order
    assert recs != [other.draw_degrade(g) for g in range(300)]
    for g, rec in enumerate(recs):
        assert ops._degrade_record(g, rec) == rec[0] + rec[1:]                              # every record passes the op's checks
        taps, amp, seed, quality, flags = rec
        assert quality == 0 or 30 <= quality <= 95
        assert amp == 0 or ops.noise_amp(1.0) <= amp <= ops.noise_amp(10.0)
        assert (amp != 0 or (seed == 0 and flags == 0)) and flags in (0, 1)
        assert taps == ops.DEGRADE_TAPS_OFF or ops.blur_taps(1.5)[0] <= taps[0] <= ops.blur_taps(0.2)[0]
    frac = lambda f: sum(1 for r in recs if f(r)) / len(recs)
    assert abs(frac(lambda r: r[0] != ops.DEGRADE_TAPS_OFF) - 0.5) < 0.1 and abs(frac(lambda r: r[1] != 0) - 0.5) < 0.1
    assert abs(frac(lambda r: r[3] != 0) - 0.7) < 0.1 and 0.1 < frac(lambda r: r[4] == 1) < 0.3
    assert len({r[2] for r in recs if r[1]}) > 100                                          # the noise seed comes from the stream too
    # one stage's setting does not move another's draws
    no_blur = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(blur_prob=0.0), **kw)
    assert [no_blur.draw_degrade(g)[1:] for g in range(50)] == [r[1:] for r in recs[:50]]
    assert all(no_blur.draw_degrade(g)[0] == ops.DEGRADE_TAPS_OFF for g in range(50))
    off = data.PatchSampler(str(tmp_path), degrade=data.DegradeSpec(blur_prob=0, noise_prob=0, jpeg_prob=0), **kw)
    assert all(off.draw_degrade(g) == ops.DEGRADE_OFF for g in range(50))
    with pytest.raises(IndexError):
        s.draw_degrade(-1)
    with pytest.raises(ValueError, match="DegradeSpec"):
        data.PatchSampler(str(tmp_path), degrade={"blur_prob": 1}, **kw)


# ---- the op's host checks ----
def test_degrade_validates_before_any_library_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("a library call was reached")
    monkeypatch.setattr(_lib, "call", reached)
    monkeypatch.setattr(ops._RecordStager, "upload", reached)
    x = torch.zeros((2, 3, 9, 11))
    good = ops.DEGRADE_OFF
    taps = ops.blur_taps(1.0)
    for bad in ((taps[:3] + (taps[3] + 1,), 0, 0, 0, 0),           # the taps do not sum to 1 << 22
                ((1 << 22) + 2, -1, 0, 0), ((-2, 1 << 21, 1, 0), 0, 0, 0, 0),
                (taps[:3], 0, 0, 0, 0), (taps, -1, 0, 0, 0), (taps, (1 << 20) + 1, 0, 0, 0), (taps, 0, -1, 0, 0), (taps, 0, 1 << 32, 0, 0),
                (taps, 0, 0, -1, 0), (taps, 0, 0, 101, 0), (taps, 0, 0, 50.5, 0), (taps, 0, 0, 50, 2), (taps, 0, 0, 50, -1),
                (taps, 0, 0, 50), None, "record"):
        with pytest.raises(ValueError, match="sample 1"):
            ops.degrade(x, [good, bad])
    with pytest.raises(ValueError, match="sample 0"):
        ops.degrade(x, [(taps, 0, 0, 200, 0), good])
    with pytest.raises(ValueError, match="2 samples but 1 records"):
        ops.degrade(x, [good])
    with pytest.raises(TypeError):
        ops.degrade(x.double(), [good, good])
    with pytest.raises(TypeError):
        ops.degrade(x.numpy(), [good, good])
    for shaped in (x[:, :2], x[0], x[:, :, :, ::2], x.new_zeros((2, 3, 0, 4))):
        with pytest.raises(ValueError):
            ops.degrade(shaped, [good, good])
    with pytest.raises(ValueError, match="overlap"):
        ops.degrade(x, [good, good], out=x)
    big = torch.zeros(2 * x.numel())
    with pytest.raises(ValueError, match="overlap"):                                        # a view that starts inside x's storage
        ops.degrade(big[:x.numel()].view_as(x), [good, good], out=big[5:5 + x.numel()].view_as(x))
    with pytest.raises(ValueError):
        ops.degrade(x, [good, good], out=torch.zeros((2, 3, 9, 12)))
    with pytest.raises(TypeError):
        ops.degrade(x, [good, good], out=torch.zeros((2, 3, 9, 11), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                              # all valid, on the CPU: refused, still no call
        ops.degrade(x, [good, (taps, ops.noise_amp(3), 9, 75, 1)], out=torch.zeros_like(x))

    class Packs:
        def pack(self):
            return (taps, 0, 0, 101, 0)
    with pytest.raises(ValueError, match="sample 1.*quality"):
        ops.degrade(x, [good, Packs()])


# ---- ABI ----
def test_degrade_is_declared_bound_and_exported():
    from transformerupscaler_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    assert re.search(r"int tup_degrade_lr\(const float\* in, const void\* recs, int B, int H, int W, float\* out, void\* stream\);", header)
    P, I = _lib.P, _lib.I
    assert _lib.SIGNATURES["tup_degrade_lr"] == [P, P, I, I, I, P, P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tup_degrade_lr")
    assert lib.tup_abi_version() == ABI
    assert _lib.load() is not None                      # every bound symbol resolves
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("degrade.hip", ["degrade_lr_kernel"])' in guard
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "degrade.hip")).read()
    assert "sizeof(DegradeRec) == 32" in src and ops._DEGRADE_REC.size == 32
    assert "atomic" not in src.split("#include")[1]     # every element has one writer
    usage = os.path.join(ROOT, "transformerupscaler_amd", "csrc", "build", "resource_usage.json")
    if os.path.exists(usage):                           # written by the build
        import json
        mine = {k: v for k, v in json.load(open(usage))["kernels"].items() if "degrade_lr_kernel" in k}
        assert len(mine) == 1 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] for v in mine.values())


def test_entry_refuses_bad_arguments_before_it_launches():
    from transformerupscaler_amd import _lib
    fn = _lib.load().tup_degrade_lr
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


def test_train_py_degrade_argument_rules(tmp_path):
    import train
    d = str(tmp_path)
    for extra in (["--degrade"], ["--degrade_blur", "0.2,1"], ["--degrade_noise", "1,5"], ["--degrade_jpeg", "30,90"], ["--degrade_prob", "1,1,1"]):
        assert "need --patch_size" in _refused(["--data_dir", d] + extra)
    base = ["--data_dir", d, "--patch_size", "16"]
    for flag, values in (("--degrade_blur", ("1", "1,x", "2,1", "0.5,3.5", "1,2,3")), ("--degrade_noise", ("5", "-1,2", "9,3", "a,b")),
                         ("--degrade_jpeg", ("0,50", "50,101", "90,30", "30.5,90", "75")), ("--degrade_prob", ("0.5,0.5", "0.5,0.5,1.5", "x,0,0", "-1,0,0"))):
        for v in values:
            assert flag in _refused(base + [f"{flag}={v}"]), (flag, v)      # "=": a value may start with a minus sign
    parse = train.build_parser().parse_args
    args = parse(base)
    assert train.degrade_options(args) is None and train.patch_options(args) == (16, (2, 3, 4, 6))
    args = parse(base + ["--degrade"])
    assert train.degrade_options(args) == {} and train.patch_options(args) == (16, (2, 3, 4, 6))      # the spec's defaults
    args = parse(base + ["--degrade_blur", "0.5,2", "--degrade_noise", "2,4", "--degrade_jpeg", "40,80", "--degrade_prob", "1,0,0.25"])
    assert train.degrade_options(args) == {"blur_sigma": (0.5, 2.0), "noise_sigma": (2.0, 4.0), "jpeg_quality": (40, 80),
                                           "blur_prob": 1.0, "noise_prob": 0.0, "jpeg_prob": 0.25}
    doc = train.__doc__
    assert all(flag in doc for flag in ("--degrade", "--degrade_blur", "--degrade_noise", "--degrade_jpeg", "--degrade_prob"))
