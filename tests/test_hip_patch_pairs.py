"""`tup_patch_pairs` (csrc/patch_pairs.hip) through `ops.patch_pairs` and `data.PatchSampler.batch` on the MI355X, bit-exact against the
numpy statement tests/_patch_pairs_ref.py (itself pinned to Pillow in tests/test_patch_sampler_cpu.py).  Shapes: frames of 131 x 149
and 97 x 203 (odd widths: unaligned row strides), LR sides 20 (a full and a partial 16-tile each way), 8 (one partial tile) and 7 at
scale 3 (HR side 21: the path without 16-byte stores)."""
import functools
import os

import numpy as np
import pytest
import torch

import _patch_pairs_ref as REF
from transformerupscaler_amd import _lib, data, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = ((131, 149), (97, 203))


@functools.lru_cache(maxsize=None)
def frame_np(i):
    a = np.random.default_rng(100 + i).integers(0, 256, SIZES[i] + (3,), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frame_gpu(i):
    return torch.from_numpy(frame_np(i).copy()).to(DEV)


def boxes_for(i, P):
    """The four corners of the frame and two interior odd offsets, each under every op (8 x 6 samples; corners coincide when the
    crop is as tall as the frame)."""
    H, W = SIZES[i]
    places = [(0, 0), (0, W - P), (H - P, 0), (H - P, W - P), (min(3, H - P), min(5, W - P)), ((H - P) // 2 | 1 if H - P > 1 else 0, (W - P) // 2 | 1)]
    return [(y0, x0, op) for op in range(8) for y0, x0 in places]


def check(frames_idx, boxes, p, scale, out=None):
    lr, hr = ops.patch_pairs([frame_gpu(i) for i in frames_idx], boxes, p, scale, out=out)
    ref_lr, ref_hr = REF.patch_pairs([frame_np(i) for i in frames_idx], boxes, p, scale)
    P = p * scale
    assert lr.shape == (len(boxes), 3, p, p) and hr.shape == (len(boxes), 3, P, P) and lr.dtype == hr.dtype == torch.float32
    got_lr, got_hr = lr.cpu(), hr.cpu()
    for b, box in enumerate(boxes):          # per sample, so that a failure names its box
        assert torch.equal(got_hr[b], torch.from_numpy(ref_hr[b])), ("hr", frames_idx[b], box, p, scale)
        assert torch.equal(got_lr[b], torch.from_numpy(ref_lr[b])), ("lr", frames_idx[b], box, p, scale)
    return lr, hr


CASES = [(i, p, s) for i in (0, 1) for p in (20, 8) for s in (2, 3, 4, 6) if p * s <= min(SIZES[i])] + [(0, 7, 3), (1, 7, 3)]


@pytest.mark.parametrize("i,p,scale", CASES)
def test_all_ops_at_corners_and_odd_offsets(i, p, scale):
    assert (0, 20, 6) in CASES and (1, 20, 6) not in CASES          # scale 6 at p = 20 only where the frame is large enough
    boxes = boxes_for(i, p * scale)
    check([i] * len(boxes), boxes, p, scale)


@pytest.mark.parametrize("p,scale", [(20, 2), (20, 6), (8, 3)])
def test_single_sample(p, scale):
    for op in (0, 5, 6):
        check([0], [(7, 9, op)], p, scale)


@pytest.mark.parametrize("p,scale", [(20, 2), (20, 4), (8, 6)])
def test_five_samples_of_two_frames_in_one_launch(p, scale):
    P = p * scale
    boxes = [(1, 3, 4), (97 - P, 203 - P, 3), (131 - P, 0, 7), (0, 1, 0), (5, 149 - P, 6)]
    check([0, 1, 0, 1, 0], boxes, p, scale)                        # frame 0 three times


def test_identity_box_equals_the_existing_resize_and_to_tensor():
    for side, p in ((48, 24), (60, 20), (48, 8), (21, 7)):
        f = torch.from_numpy(np.random.default_rng(side).integers(0, 256, (side, side, 3), dtype=np.uint8)).to(DEV)
        lr, hr = ops.patch_pairs([f], [(0, 0, 0)], p, side // p)
        assert torch.equal(lr, ops.resize_frames(f, (p, p), to_tensor=True))
        assert torch.equal(hr, ops.frames_to_tensor(f))


@pytest.mark.parametrize("i,p,scale,pad", [(0, 20, 3, 13), (1, 8, 4, 16), (0, 7, 3, 5), (0, 20, 6, 1)])
def test_no_write_outside_the_outputs(i, p, scale, pad):
    """The outputs are views into larger sentinel-filled allocations; an odd `pad` also moves them off 16-byte alignment."""
    P = p * scale
    boxes = boxes_for(i, P)[::5]
    B = len(boxes)
    sentinel = -7.0
    big_lr = torch.full((pad + B * 3 * p * p + pad,), sentinel, dtype=torch.float32, device=DEV)
    big_hr = torch.full((pad + B * 3 * P * P + pad,), sentinel, dtype=torch.float32, device=DEV)
    out = (big_lr[pad:pad + B * 3 * p * p].view(B, 3, p, p), big_hr[pad:pad + B * 3 * P * P].view(B, 3, P, P))
    lr, hr = check([i] * B, boxes, p, scale, out=out)
    assert lr.data_ptr() == out[0].data_ptr() and hr.data_ptr() == out[1].data_ptr()
    for big, n in ((big_lr, B * 3 * p * p), (big_hr, B * 3 * P * P)):
        assert bool((big[:pad] == sentinel).all()) and bool((big[pad + n:] == sentinel).all())
        assert not bool((big[pad:pad + n] == sentinel).any())          # ... and every element inside was written
    # an empty batch launches nothing and returns empty outputs
    lr0, hr0 = ops.patch_pairs([], [], p, scale)
    assert lr0.shape == (0, 3, p, p) and hr0.shape == (0, 3, P, P)
    with pytest.raises(ValueError):
        ops.patch_pairs([frame_gpu(i)], [boxes[0]], p, scale, out=out)     # out of another batch size


def test_sampler_batch_is_one_launch_per_scale_in_index_order(tmp_path, monkeypatch):
    from PIL import Image
    for i in (0, 1):
        Image.fromarray(frame_np(i)).save(os.path.join(str(tmp_path), f"img_{i}.png"))
    sampler = data.PatchSampler(str(tmp_path), patch=8, scales=(2, 3, 6), seed=11, device=DEV)
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    indices = [40, 3, 17, 101, 5, 64, 9, 2, 33, 12, 77, 50]
    draws = [sampler.draw(g) for g in indices]
    assert len({d[1] for d in draws}) == 3 and len({d[0] for d in draws}) == 2          # every scale, both images
    lr_list, hr_list = sampler.batch(indices)
    assert calls.count("tup_patch_pairs") == 3 and sampler.decodes == 2
    assert len(lr_list) == len(hr_list) == len(indices)
    for (image, scale, y0, x0, op), lr, hr in zip(draws, lr_list, hr_list):
        ref_lr, ref_hr = REF.patch_pair(frame_np(image), y0, x0, op, 8, scale)
        assert lr.shape == (3, 8, 8) and hr.shape == (3, 8 * scale, 8 * scale)
        assert torch.equal(lr.cpu(), torch.from_numpy(ref_lr)) and torch.equal(hr.cpu(), torch.from_numpy(ref_hr))
    calls.clear()
    one = [g for g, d in zip(indices, draws) if d[1] == draws[0][1]]
    sampler.batch(one)
    assert calls.count("tup_patch_pairs") == 1                                           # one scale: one launch
