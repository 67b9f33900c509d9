"""`tup_degrade_lr_sub` (csrc/degrade420.hip) through `ops.degrade` with `flags & ops.DEGRADE_JPEG_420`, through
`data.PatchSampler(degrade=DegradeSpec(jpeg_420_prob=...)).batch` and through `train.py --degrade_jpeg_420` on the MI355X, bit-exact
against the numpy statement tests/_degrade420_ref.py (itself pinned to Pillow in tests/test_degrade420_cpu.py).

Sizes: 3 x 4 and 5 x 4 (libjpeg's rule for narrow images on and off), 7 x 13 (one partial MCU), 16 x 16, 17 x 23, 33 x 47 (the second
tile is 1 pixel wide, its ring mostly outside, both sizes odd), 32 x 64 and 64 x 65 (a tile seam exactly on an MCU seam, and one pixel
past it), 40 x 72 (three tiles across), 96 x 96 (nine whole tiles: the centre one has its whole ring).  Inputs are random floats in
[-0.1, 1.1]: off the k / 255 grid, and clipped at both ends."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _degrade420_ref as REF
import _degrade_ref as D
import _patch_pairs_ref as PAIRS
from transformerupscaler_amd import _lib, data, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((3, 4), (5, 4), (7, 13), (16, 16), (17, 23), (33, 47), (32, 64), (64, 65), (40, 72), (96, 96))
SUB = ops.DEGRADE_JPEG_420

JPEG = {q: (D.TAPS_OFF, 0, 0, q, SUB) for q in (5, 50, 75, 100)}
ALL = (D.blur_taps(3.0), D.noise_amp(6), 42, 75, SUB)                            # radius 3, every tap large; colour noise
ALL_GREY = (D.blur_taps(3.0), D.noise_amp(10), 7, 30, SUB | 1)
SINGLE = {"jpeg5": JPEG[5], "jpeg50": JPEG[50], "jpeg75": JPEG[75], "jpeg100": JPEG[100], "all": ALL, "all_grey": ALL_GREY}
PLAIN_JPEG = (D.TAPS_OFF, 0, 0, 75, 0)
PLAIN_ALL = (D.blur_taps(0.8), D.noise_amp(5), 4000000000, 60, 1)
SIX = [ALL, D.RECORD_OFF, PLAIN_JPEG, JPEG[5], ALL_GREY, PLAIN_ALL]              # flagged, all off, unflagged: one launch
UNFLAGGED = (1, 2, 5)


@functools.lru_cache(maxsize=None)
def x_np(hw, B):
    """fp32 [B][3][H][W]: the first sample smooth with a colour edge, the others random, all off the byte grid."""
    h, w = hw
    rng = np.random.default_rng(h * 100 + w + B)
    x = rng.random((B, 3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    yy, xx = np.mgrid[0:h, 0:w]
    x[0] = (0.5 + 0.45 * np.sin(xx / 5.0 + yy / 7.0 + np.arange(3).reshape(3, 1, 1)) + 0.02 * x[0]).astype(np.float32)
    x[0, 0, :, w // 2:] = np.float32(0.97)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def x_gpu(hw, B):
    return torch.from_numpy(x_np(hw, B).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def ref(hw, records):
    out = REF.degrade(x_np(hw, len(records)), list(records))
    out.setflags(write=False)
    return out


def check(hw, records, out=None):
    records = tuple(records)
    got = ops.degrade(x_gpu(hw, len(records)), list(records), out=out)
    assert got.shape == (len(records), 3) + hw and got.dtype == torch.float32
    want = ref(hw, records)
    host = got.cpu()
    for b, rec in enumerate(records):          # per sample, so that a failure names its record
        w = torch.from_numpy(want[b].copy())
        bad = (host[b] != w).nonzero()
        assert torch.equal(host[b], w), (hw, b, rec[1:], len(bad), bad[:4].tolist(), float((host[b] - w).abs().max() * 255))
    return got


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("name", list(SINGLE))
def test_jpeg_alone_and_all_stages_single_sample(hw, name):
    check(hw, [SINGLE[name]])


@pytest.mark.parametrize("hw", SIZES)
def test_six_samples_flagged_unflagged_and_off_in_one_launch(hw, monkeypatch):
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    got = check(hw, SIX)
    assert calls == ["tup_degrade_lr_sub"]                                        # one library call for the mixed batch
    # the rows without the flag are tup_degrade_lr's, bit for bit
    plain = ops.degrade(x_gpu(hw, 6), [r if i in UNFLAGGED else D.RECORD_OFF for i, r in enumerate(SIX)])
    assert calls == ["tup_degrade_lr_sub", "tup_degrade_lr"]                      # ... and a batch without the flag is the old entry's
    for i in UNFLAGGED:
        assert torch.equal(got[i], plain[i]), (hw, i)
    if min(hw) >= 16:
        assert not torch.equal(got[3], ops.degrade(x_gpu(hw, 6)[3:4], [JPEG[5][:4] + (0,)])[0])       # 4:2:0 is not 4:4:4


@pytest.mark.parametrize("hw,pad", [((33, 47), 4), ((33, 47), 1), ((40, 72), 2), ((64, 65), 3), ((40, 72), 4), ((5, 4), 1), ((96, 96), 3)])
def test_no_write_outside_the_output(hw, pad):
    """The output is a view into a larger sentinel-filled allocation; `pad` = 4, 1, 2, 3 floats puts it at each of the four 16-byte
    alignments (40 x 72 at pad 4 takes the 16-byte stores, at pad 2 the scalar ones at a width that would allow the wide ones)."""
    n = 6 * 3 * hw[0] * hw[1]
    sentinel = -7.0
    big = torch.full((pad + n + pad,), sentinel, dtype=torch.float32, device=DEV)
    out = big[pad:pad + n].view(6, 3, *hw)
    got = check(hw, SIX, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((big[:pad] == sentinel).all()) and bool((big[pad + n:] == sentinel).all())
    assert not bool((big[pad:pad + n] == sentinel).any())                         # ... and every element inside was written


def test_capture_and_replay_equal_eager():
    hw = (40, 72)
    x = x_gpu(hw, 6).clone()
    eager = ops.degrade(x, SIX)
    raw = b"".join(ops._DEGRADE_REC.pack(*ops._degrade_record(i, r)) for i, r in enumerate(SIX))
    table = torch.from_numpy(np.frombuffer(raw, dtype=np.int64).copy()).to(DEV)
    out = torch.full_like(x, -7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.call("tup_degrade_lr_sub", x.data_ptr(), table.data_ptr(), 6, hw[0], hw[1], out.data_ptr(), ops._stream())
    out.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(x_gpu(hw, 6).flip(0))                                                 # the replay reads the inputs of its time
    graph.replay()
    assert torch.equal(out, ops.degrade(x, SIX))


def test_launcher_refusals():
    x = x_gpu((20, 28), 6)
    fn = _lib.load().tup_degrade_lr_sub
    table = torch.zeros(6 * 4, dtype=torch.int64, device=DEV)
    out = torch.empty_like(x)
    invalid = 1
    assert fn(x.data_ptr(), table.data_ptr(), 6, 20, 28, x.data_ptr(), None) == invalid
    assert fn(x.data_ptr(), table.data_ptr(), 6, 20, 28, x.data_ptr() + 4 * (x.numel() - 1), None) == invalid
    assert fn(None, table.data_ptr(), 6, 20, 28, out.data_ptr(), None) == invalid
    assert fn(x.data_ptr(), table.data_ptr(), 0, 20, 28, out.data_ptr(), None) == invalid
    assert fn(x.data_ptr(), table.data_ptr(), 6, 20, 0, out.data_ptr(), None) == invalid
    with pytest.raises(ValueError, match="sample 2"):
        ops.degrade(x, [JPEG[5]] * 2 + [(D.TAPS_OFF, 0, 0, 0, SUB)] + [JPEG[5]] * 3)


# ---- the sampler ----
def test_sampler_batch_is_patch_pairs_then_the_reference(tmp_path, monkeypatch):
    from PIL import Image
    frames = [np.random.default_rng(50 + i).integers(0, 256, hw + (3,), dtype=np.uint8) for i, hw in enumerate(((131, 149), (97, 203)))]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(str(tmp_path), f"img_{i}.png"))
    spec = data.DegradeSpec(blur_prob=0.6, noise_prob=0.6, jpeg_prob=1, jpeg_420_prob=1, jpeg_quality=(5, 100), blur_sigma=(0.2, 3.0))
    kw = dict(patch=21, scales=(2, 3), seed=11, device=DEV)
    sampler = data.PatchSampler(str(tmp_path), degrade=spec, **kw)
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    indices = [40, 3, 17, 101, 5, 64, 9, 2, 33, 12]
    lr_list, hr_list = sampler.batch(indices)
    assert calls == ["tup_patch_pairs", "tup_degrade_lr_sub"] * 2                 # one of each per distinct scale
    recs = [sampler.draw_degrade(g) for g in indices]
    assert all(r[3] != 0 and r[4] & SUB for r in recs) and any(r[1] for r in recs) and any(r[0] != D.TAPS_OFF for r in recs)
    for g, rec, lr, hr in zip(indices, recs, lr_list, hr_list):
        image, scale, y0, x0, op = sampler.draw(g)
        ref_lr, ref_hr = PAIRS.patch_pair(frames[image], y0, x0, op, 21, scale)
        assert torch.equal(hr.cpu(), torch.from_numpy(ref_hr))                    # HR is untouched
        assert torch.equal(lr.cpu(), torch.from_numpy(REF.degrade(ref_lr[None], [rec])[0])), (g, rec[1:])


# ---- the driver ----
def _write_images(d, n, hw=(64, 80)):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]].astype(np.float64)
    for i in range(n):
        rng = np.random.RandomState(i)
        planes = [127 + 90 * np.sin(yy / (5 + c + i) + c) * np.cos(xx / (7 + 2 * c - i) + i) + rng.normal(0, 6, hw) for c in range(3)]
        Image.fromarray(np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)).save(os.path.join(d, f"img_{i}.png"))


def test_driver_runs_with_420_are_reproducible_and_differ_from_444(tmp_path):
    images = str(tmp_path / "images")
    _write_images(images, 3)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    records = {}
    for name, extra in (("a", ["--degrade_jpeg_420", "1"]), ("b", ["--degrade_jpeg_420", "1"]), ("plain", [])):
        rec = str(tmp_path / f"{name}.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--data_dir", images, "--patch_size", "16", "--patch_scales", "2,3",
                            "--batch_size", "4", "--max_steps", "3", "--deterministic", "--seed", "3", "--epochs", "1", "--degrade",
                            "--checkpoint_dir", str(tmp_path / f"ck_{name}"), "--json", rec] + extra,
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("jpeg_420_prob=1.0" in r.stdout) == bool(extra), r.stdout
        records[name] = json.load(open(rec))
    a, b, plain = (records[k] for k in ("a", "b", "plain"))
    losses = [s["loss"] for s in a["steps"]]
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses)
    assert losses == [s["loss"] for s in b["steps"]]
    assert losses != [s["loss"] for s in plain["steps"]]
    assert a["degrade"] == data.DegradeSpec(jpeg_420_prob=1).as_dict() == {**plain["degrade"], "jpeg_420_prob": 1.0}
    assert plain["degrade"] == data.DegradeSpec().as_dict()
