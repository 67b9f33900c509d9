"""`tup_degrade_lr` (csrc/degrade.hip) through `ops.degrade` and `data.PatchSampler(degrade=...).batch` on the MI355X, bit-exact
against the numpy statement tests/_degrade_ref.py (itself pinned to Pillow in tests/test_degrade_cpu.py), and through the `train.py`
driver.  Sizes: 7 x 13 (less than one JPEG block), 20 x 28 (partial blocks, one partial tile; the width allows 16-byte stores),
40 x 72 (tile seams cross the blur halo and the block grid both ways) and 96 x 96 (nine whole tiles); 21 x 21 in the sampler test
(the path without 16-byte stores).  Inputs are random floats in [-0.1, 1.1]: off the k / 255 grid, and clipped at both ends."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _degrade_ref as REF
import _patch_pairs_ref as PAIRS
from transformerupscaler_amd import _lib, data, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((7, 13), (20, 28), (40, 72), (96, 96))

OFF = REF.RECORD_OFF
BLUR = (REF.blur_taps(1.1), 0, 0, 0, 0)
BLUR_MAX = (REF.blur_taps(ops.DEGRADE_MAX_BLUR_SIGMA), 0, 0, 0, 0)             # radius 3, every tap large
NOISE = (REF.TAPS_OFF, REF.noise_amp(8), 123456789, 0, 0)
NOISE_GREY = (REF.TAPS_OFF, REF.noise_amp(5), 4000000000, 0, 1)
JPEG = {q: (REF.TAPS_OFF, 0, 0, q, 0) for q in (5, 50, 75, 100)}
ALL = (REF.blur_taps(0.8), REF.noise_amp(6), 42, 75, 0)
ALL_GREY = (REF.blur_taps(3.0), REF.noise_amp(10), 7, 30, 1)
SINGLE = {"off": OFF, "blur": BLUR, "blur_max": BLUR_MAX, "noise": NOISE, "noise_grey": NOISE_GREY, "jpeg5": JPEG[5], "jpeg50": JPEG[50],
          "jpeg75": JPEG[75], "jpeg100": JPEG[100], "all": ALL, "all_grey": ALL_GREY}
FIVE = [ALL, OFF, JPEG[5], NOISE_GREY, ALL_GREY]                                 # a different record per sample, one of them all off


@functools.lru_cache(maxsize=None)
def x_np(hw, B):
    """fp32 [B][3][H][W]: the first sample smooth (large low-frequency coefficients), the others random, all off the byte grid."""
    h, w = hw
    rng = np.random.default_rng(h * 100 + w + B)
    x = rng.random((B, 3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    yy, xx = np.mgrid[0:h, 0:w]
    x[0] = (0.5 + 0.45 * np.sin(xx / 5.0 + yy / 7.0 + np.arange(3).reshape(3, 1, 1)) + 0.02 * x[0]).astype(np.float32)
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
        assert torch.equal(host[b], torch.from_numpy(want[b].copy())), (hw, b, rec[1:], float((host[b] - torch.from_numpy(want[b].copy())).abs().max() * 255))
    return got


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("name", list(SINGLE))
def test_each_stage_alone_and_together_single_sample(hw, name):
    check(hw, [SINGLE[name]])


@pytest.mark.parametrize("hw", SIZES)
def test_five_samples_with_different_records_in_one_launch(hw):
    got = check(hw, FIVE)
    q = torch.from_numpy(REF.quantise(x_np(hw, 5)[1]).astype(np.float32) / np.float32(255))
    assert torch.equal(got[1].cpu(), q)                                           # the all-off record: the quantised input
    assert not torch.equal(got[0].cpu(), torch.from_numpy(REF.degrade(x_np(hw, 5)[:1], [OFF])[0]))


def test_values_on_the_byte_grid_come_back_exactly():
    k = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255))      # what patch_pairs writes: (float)k / 255.0f, rounded once
    x = k.repeat(3 * 4).view(1, 3, 32, 32).contiguous().to(DEV)
    assert torch.equal(ops.degrade(x, [OFF]), x)


@pytest.mark.parametrize("hw,pad", [((20, 28), 4), ((20, 28), 1), ((40, 72), 3), ((7, 13), 16), ((96, 96), 2)])
def test_no_write_outside_the_output(hw, pad):
    """The output is a view into a larger sentinel-filled allocation; a `pad` that is no multiple of 4 moves it off 16-byte
    alignment (the scalar store path at a width that would allow the wide one)."""
    n = 5 * 3 * hw[0] * hw[1]
    sentinel = -7.0
    big = torch.full((pad + n + pad,), sentinel, dtype=torch.float32, device=DEV)
    out = big[pad:pad + n].view(5, 3, *hw)
    got = check(hw, FIVE, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((big[:pad] == sentinel).all()) and bool((big[pad + n:] == sentinel).all())
    assert not bool((big[pad:pad + n] == sentinel).any())                         # ... and every element inside was written


def test_capture_and_replay_equal_eager():
    """The launch itself is captured on the capturing stream (the record table is uploaded beforehand: `ops.degrade` stages it
    through pinned memory per call, which is not a thing to capture)."""
    hw = (40, 72)
    x = x_gpu(hw, 5).clone()
    eager = ops.degrade(x, FIVE)
    raw = b"".join(ops._DEGRADE_REC.pack(*ops._degrade_record(i, r)) for i, r in enumerate(FIVE))
    table = torch.from_numpy(np.frombuffer(raw, dtype=np.int64).copy()).to(DEV)
    out = torch.full_like(x, -7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.call("tup_degrade_lr", x.data_ptr(), table.data_ptr(), 5, hw[0], hw[1], out.data_ptr(), ops._stream())
    out.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(x_gpu(hw, 5).flip(0))                                                 # the replay reads the inputs of its time
    graph.replay()
    assert torch.equal(out, ops.degrade(x, FIVE))


def test_launcher_and_op_refusals():
    x = x_gpu((20, 28), 5)
    fn = _lib.load().tup_degrade_lr
    table = torch.zeros(5 * 4, dtype=torch.int64, device=DEV)
    out = torch.empty_like(x)
    invalid = 1
    assert fn(x.data_ptr(), table.data_ptr(), 5, 20, 28, x.data_ptr(), None) == invalid
    assert fn(x.data_ptr(), table.data_ptr(), 5, 20, 28, x.data_ptr() + 4 * (x.numel() - 1), None) == invalid
    assert fn(None, table.data_ptr(), 5, 20, 28, out.data_ptr(), None) == invalid
    assert fn(x.data_ptr(), table.data_ptr(), 0, 20, 28, out.data_ptr(), None) == invalid
    assert fn(x.data_ptr(), table.data_ptr(), 5, 20, 0, out.data_ptr(), None) == invalid
    with pytest.raises(ValueError, match="overlap"):
        ops.degrade(x, FIVE, out=x)
    with pytest.raises(ValueError, match="sample 2"):
        ops.degrade(x, [OFF, OFF, (REF.TAPS_OFF, 0, 0, 101, 0), OFF, OFF])
    with pytest.raises(ValueError, match="5 samples but 4 records"):
        ops.degrade(x, FIVE[:4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.degrade(x.cpu(), FIVE)
    empty = ops.degrade(x[:0], [])                                                # an empty batch launches nothing
    assert empty.shape == (0, 3, 20, 28)


# ---- the sampler ----
def test_sampler_batch_is_patch_pairs_then_the_reference(tmp_path, monkeypatch):
    from PIL import Image
    frames = [np.random.default_rng(50 + i).integers(0, 256, hw + (3,), dtype=np.uint8) for i, hw in enumerate(((131, 149), (97, 203)))]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(str(tmp_path), f"img_{i}.png"))
    spec = data.DegradeSpec(blur_prob=0.6, noise_prob=0.6, jpeg_prob=0.6, jpeg_quality=(5, 100), blur_sigma=(0.2, 3.0))
    kw = dict(patch=21, scales=(2, 3), seed=11, device=DEV)
    sampler = data.PatchSampler(str(tmp_path), degrade=spec, **kw)
    clean = data.PatchSampler(str(tmp_path), **kw)
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    indices = [40, 3, 17, 101, 5, 64, 9, 2, 33, 12]
    lr_list, hr_list = sampler.batch(indices)
    assert calls == ["tup_patch_pairs", "tup_degrade_lr"] * 2                     # one of each per distinct scale
    _, hr_clean = clean.batch(indices)
    recs = [sampler.draw_degrade(g) for g in indices]
    assert len({r[3] != 0 for r in recs}) == 2 and any(r[1] for r in recs) and any(r[0] != REF.TAPS_OFF for r in recs)
    for g, rec, lr, hr, hr0 in zip(indices, recs, lr_list, hr_list, hr_clean):
        image, scale, y0, x0, op = sampler.draw(g)
        ref_lr, ref_hr = PAIRS.patch_pair(frames[image], y0, x0, op, 21, scale)
        assert torch.equal(hr.cpu(), torch.from_numpy(ref_hr)) and torch.equal(hr, hr0)          # HR is untouched
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


def test_driver_runs_with_degrade_are_reproducible_and_differ_from_clean(tmp_path):
    images = str(tmp_path / "images")
    _write_images(images, 3)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    records = {}
    for name, extra in (("a", ["--degrade"]), ("b", ["--degrade"]), ("clean", [])):
        rec = str(tmp_path / f"{name}.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--data_dir", images, "--patch_size", "16", "--patch_scales", "2,3",
                            "--batch_size", "4", "--max_steps", "3", "--deterministic", "--seed", "3", "--epochs", "1",
                            "--checkpoint_dir", str(tmp_path / f"ck_{name}"), "--json", rec] + extra,
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("LR degraded by DegradeSpec(" in r.stdout) == bool(extra), r.stdout
        records[name] = json.load(open(rec))
    a, b, clean = (records[k] for k in ("a", "b", "clean"))
    losses = [s["loss"] for s in a["steps"]]
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses)
    assert losses == [s["loss"] for s in b["steps"]]
    assert losses != [s["loss"] for s in clean["steps"]]
    assert a["degrade"] == data.DegradeSpec().as_dict() and "degrade" not in clean
    assert a["patch"] == {**clean["patch"], "timing": a["patch"]["timing"]}     # the patch entry itself is as without the flag
