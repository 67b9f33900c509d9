"""CPU checks of patch training: the numpy statement of a sample (tests/_patch_pairs_ref.py) against Pillow itself, and that the
order of transpose and resize matters; `data.PatchSampler.draw` as a pure function; construction errors; `ops.patch_pairs`'s box
validation ahead of any library call; the `tup_patch_pairs` entry through header / binding / library; train.py's argument rules."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _patch_pairs_ref as REF
from _abi import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (2, 3, 4, 6)


def _frame(hw, seed):
    return np.random.default_rng(seed).integers(0, 256, hw + (3,), dtype=np.uint8)


# ---- the reference ----
@pytest.mark.parametrize("scale", SCALES)
def test_reference_equals_pillow_for_all_ops(scale):
    Image = pytest.importorskip("PIL.Image")
    frame, p = _frame((131, 149), 1), 20
    P = p * scale
    y0, x0 = 131 - P, 149 - P - (3 if 149 - P >= 3 else 0)
    flips = (Image.Transpose.FLIP_LEFT_RIGHT, Image.Transpose.FLIP_TOP_BOTTOM, Image.Transpose.TRANSPOSE)
    for op in range(8):
        im = Image.fromarray(frame).crop((x0, y0, x0 + P, y0 + P))
        for bit, how in enumerate(flips):
            if op & (1 << bit):
                im = im.transpose(how)
        hr = np.asarray(im)
        lr = np.asarray(im.resize((p, p), Image.BILINEAR))
        ref_lr, ref_hr = REF.patch_pair(frame, y0, x0, op, p, scale)
        assert np.array_equal(ref_hr, hr.transpose(2, 0, 1).astype(np.float32) / np.float32(255)), (scale, op)
        assert np.array_equal(ref_lr, lr.transpose(2, 0, 1).astype(np.float32) / np.float32(255)), (scale, op)


@pytest.mark.parametrize("scale", SCALES)
def test_transpose_does_not_commute_with_the_resize(scale):
    frame, p = _frame((131, 149), 2), 20
    for op in range(8):
        lr, _ = REF.patch_pair(frame, 3, 5, op, p, scale)
        other = REF.resize_then_transpose(frame, 3, 5, op, p, scale)
        if op < 4:                                                   # flips commute to the bit
            flipped, _ = REF.patch_pair(frame, 3, 5, 0, p, scale)
            if op & 1:
                flipped = flipped[:, :, ::-1]
            if op & 2:
                flipped = flipped[:, ::-1]
            assert np.array_equal(lr, flipped) and np.array_equal(lr, other), (scale, op)
        else:
            diff = np.abs(lr - other) * 255
            assert diff.max() > 0.5, (scale, op)                    # the order is visible ...
            assert diff.max() < 1.5, (scale, op)                    # ... as single LSBs


# ---- the sampler ----
def _write_pngs(d, sizes):
    from PIL import Image
    for i, hw in enumerate(sizes):
        Image.fromarray(np.full(tuple(hw) + (3,), 10 * i, np.uint8)).save(os.path.join(d, f"img_{i}.png"))


def test_draw_is_a_pure_function_of_seed_and_index(tmp_path):
    from transformerupscaler_amd import data
    sizes = [(40, 64), (64, 40), (100, 120), (30, 30)]
    _write_pngs(str(tmp_path), sizes)
    s = data.PatchSampler(str(tmp_path), patch=8, scales=(2, 4, 6), seed=5, device="cpu")
    assert s.sizes == sizes                                          # from the PNG headers
    assert s.decodes == 0                                            # ... without a decode
    assert s.eligible == {2: [0, 1, 2, 3], 4: [0, 1, 2], 6: [2]}
    again = data.PatchSampler(str(tmp_path), patch=8, scales=(2, 4, 6), seed=5, device="cpu")
    other = data.PatchSampler(str(tmp_path), patch=8, scales=(2, 4, 6), seed=6, device="cpu")
    draws = [s.draw(g) for g in range(400)]
    assert draws == [again.draw(g) for g in range(400)]
    assert draws[::-1] == [s.draw(g) for g in reversed(range(400))]  # no state: any order
    assert draws != [other.draw(g) for g in range(400)]
    assert len(set(draws)) > 390
    for image, scale, y0, x0, op in draws:
        h, w = sizes[image]
        assert scale in (2, 4, 6) and image in s.eligible[scale]
        assert 0 <= y0 and y0 + 8 * scale <= h and 0 <= x0 and x0 + 8 * scale <= w
        assert 0 <= op < 8
        assert all(type(v) is int for v in (image, scale, y0, x0, op))
    assert {d[1] for d in draws} == {2, 4, 6} and {d[4] for d in draws} == set(range(8))
    assert {d[0] for d in draws if d[1] == 2} == {0, 1, 2, 3}
    assert any(d[2] == 0 for d in draws) and any(d[2] + 8 * d[1] == sizes[d[0]][0] for d in draws)     # both ends are reachable
    plain = data.PatchSampler(str(tmp_path), patch=8, scales=(2, 4, 6), seed=5, augment=False, device="cpu")
    assert all(plain.draw(g)[4] == 0 for g in range(100))
    assert [plain.draw(g)[:4] for g in range(100)] == [d[:4] for d in draws[:100]]                     # op is drawn last
    with pytest.raises(IndexError):
        s.draw(-1)


def test_rank_slices_partition_a_batch_and_epoch_length_matches_pair_dataset(tmp_path):
    from transformerupscaler_amd import data
    _write_pngs(str(tmp_path), [(40, 40)] * 3)
    s = data.PatchSampler(str(tmp_path), patch=8, scales=(2,), device="cpu")
    assert len(s) == s.samples_per_epoch == len(data.PairDataset(str(tmp_path), device="cpu")) == 30
    assert len(data.PatchSampler(str(tmp_path), patch=8, scales=(2,), samples_per_epoch=7, device="cpu")) == 7
    batch = [2 * len(s) + i for i in (5, 17, 3, 29, 11, 0, 8)]          # global indices of one step of epoch 2
    for world in (1, 2, 3, 8):
        parts = [batch[r::world] for r in range(world)]
        assert sorted(g for part in parts for g in part) == sorted(batch)
        assert sum(len(part) for part in parts) == len(batch)
        assert [s.draw(g) for part in parts for g in part] == [s.draw(g) for g in sum(parts, [])]


def test_construction_errors(tmp_path):
    from transformerupscaler_amd import data
    for bad in (None, ""):
        with pytest.raises(ValueError, match="data_dir"):
            data.PatchSampler(bad)
    with pytest.raises(FileNotFoundError):
        data.PatchSampler(str(tmp_path / "missing"), device="cpu")
    with pytest.raises(FileNotFoundError, match="no .png"):
        data.PatchSampler(str(tmp_path), device="cpu")
    _write_pngs(str(tmp_path), [(40, 64), (64, 40)])
    with pytest.raises(ValueError, match=r"scale 6.*48 x 48"):           # names the scale and the size it needs
        data.PatchSampler(str(tmp_path), patch=8, scales=(2, 6), device="cpu")
    for bad in ((), (0,), (2, 2), (9,), (2.5,), ("x",), None):
        with pytest.raises(ValueError, match="scales"):
            data.PatchSampler(str(tmp_path), patch=8, scales=bad, device="cpu")
    with pytest.raises(ValueError, match="patch"):
        data.PatchSampler(str(tmp_path), patch=0, device="cpu")
    with pytest.raises(ValueError, match="samples_per_epoch"):
        data.PatchSampler(str(tmp_path), patch=8, scales=(2,), samples_per_epoch=0, device="cpu")
    (tmp_path / "broken.png").write_bytes(b"not a png")
    with pytest.raises(ValueError, match="not a PNG"):
        data.PatchSampler(str(tmp_path), patch=8, scales=(2,), device="cpu")


# ---- the op's host checks ----
def test_patch_pairs_validates_before_any_library_call(monkeypatch):
    from transformerupscaler_amd import _lib, ops

    def reached(*a, **k):
        raise AssertionError("a library call was reached")
    monkeypatch.setattr(_lib, "call", reached)
    monkeypatch.setattr(ops, "_pil_taps_on", reached)
    f = torch.zeros((40, 50, 3), dtype=torch.uint8)
    good = (0, 0, 0)
    for bad in ((-1, 0, 0), (0, -1, 0), (9, 0, 0), (0, 19, 0), (8, 18, 8), (0, 0, -1), (0, 0, 0.5), (0, 0)):
        with pytest.raises(ValueError, match="sample 1"):                # 16 x 2 = 32: y0 <= 8, x0 <= 18
            ops.patch_pairs([f, f], [good, bad], 16, 2)
    with pytest.raises(ValueError, match="sample 0"):
        ops.patch_pairs([f], [(8, 18, 7)], 16, 3)                        # fits at scale 2, not at 3
    with pytest.raises(ValueError):
        ops.patch_pairs([f, f], [good], 16, 2)
    with pytest.raises(ValueError):
        ops.patch_pairs([f], [good], 16, 9)
    with pytest.raises(ValueError):
        ops.patch_pairs([f], [good], 0, 2)
    with pytest.raises(TypeError, match="sample 0"):
        ops.patch_pairs([f.float()], [good], 16, 2)
    with pytest.raises(ValueError, match="sample 0"):
        ops.patch_pairs([f[:, ::2]], [good], 8, 2)                       # not contiguous
    with pytest.raises(ValueError, match="sample 0"):
        ops.patch_pairs([f[..., 0]], [good], 8, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # a valid box on a CPU tensor: refused, still no call
        ops.patch_pairs([f], [(8, 18, 7)], 16, 2)


# ---- ABI ----
def test_patch_pairs_is_declared_bound_and_exported():
    from transformerupscaler_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    assert re.search(r"int tup_patch_pairs\(const void\* recs, int B, int P, int p, const int\* xmin, const int\* xsize, "
                     r"const int\* k, int ksize,\s+float\* hr, float\* lr, void\* stream\);", header)
    P, I = _lib.P, _lib.I
    assert _lib.SIGNATURES["tup_patch_pairs"] == [P, I, I, I, P, P, P, I, P, P, P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tup_patch_pairs")
    assert lib.tup_abi_version() == ABI
    assert _lib.load() is not None                      # every bound symbol resolves
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("patch_pairs.hip", ["patch_pairs_kernel"])' in guard
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "patch_pairs.hip")).read()
    assert "sizeof(PatchRec) == 32" in src and ops._PATCH_REC.size == 32
    assert "atomic" not in src.split("#include")[1]     # every element has one writer


def test_entry_refuses_bad_sizes_before_it_launches():
    from transformerupscaler_amd import _lib
    fn = _lib.load().tup_patch_pairs
    invalid = 1                                         # hipErrorInvalidValue
    ok = (None, 4, 40, 20, None, None, None, 5, None, None, None)          # recs, B, P, p, xmin, xsize, k, ksize, hr, lr, stream

    def with_(**kw):
        names = ("recs", "B", "P", "p", "xmin", "xsize", "k", "ksize", "hr", "lr", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    assert fn(*with_(B=0)) == 0 and fn(*with_(B=-3)) == 0                   # a no-op, whatever else is passed
    assert fn(*with_(B=0, p=0, ksize=0)) == 0
    assert fn(*with_(B=65536)) == invalid
    assert fn(*with_(ksize=0)) == invalid
    assert fn(*with_(P=19)) == invalid                                      # P < p
    assert fn(*with_(p=0)) == invalid and fn(*with_(p=-1, P=-1)) == invalid
    assert fn(*with_(P=41)) == invalid                                      # not a multiple of p
    assert fn(*with_(P=180, ksize=19)) == invalid                           # scale 9: beyond the LDS window


# ---- the driver's argument rules ----
def _refused(argv):
    import train
    with pytest.raises(SystemExit) as e:
        train.main(argv)
    assert isinstance(e.value.code, str)                # a message, not a status: nothing ran
    return e.value.code


def test_train_py_patch_argument_rules(tmp_path):
    import train
    d = str(tmp_path)
    assert "--pairs" in _refused(["--data_dir", d, "--patch_size", "16", "--pairs", "8x8:16x16"])
    msg = _refused(["--data_dir", d, "--patch_size", "16", "--model", "ResidualTransformer"])
    assert "ResidualTransformer" in msg and "720x1280" in msg
    assert "WindowTransformer" in _refused(["--data_dir", d, "--patch_size", "14", "--model", "WindowTransformer"])
    for scales in ("2,5", "2,2", "1", "2,x", ""):
        assert "--patch_scales" in _refused(["--data_dir", d, "--patch_size", "16", "--patch_scales", scales])
    assert "--patch_size" in _refused(["--data_dir", d, "--patch_size", "0"])
    assert "--patches_per_epoch" in _refused(["--data_dir", d, "--patch_size", "16", "--patches_per_epoch", "0"])
    for extra in (["--no_augment"], ["--patches_per_epoch", "5"], ["--patch_scales", "2"]):
        assert "need --patch_size" in _refused(["--data_dir", d] + extra)
    args = train.build_parser().parse_args(["--data_dir", d])
    assert args.patch_size is None and train.patch_options(args) is None          # without the flag: today's program
    args = train.build_parser().parse_args(["--data_dir", d, "--patch_size", "24", "--patch_scales", "3,2"])
    assert train.patch_options(args) == (24, (3, 2))
    args = train.build_parser().parse_args(["--data_dir", d, "--patch_size", "16", "--patch_scales", "5,8", "--model", "WindowTransformer"])
    assert train.patch_options(args) == (16, (5, 8))
