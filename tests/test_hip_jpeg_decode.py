"""`ops.jpeg_decode` (csrc/jpeg_decode.hip) on the MI355X, pixel for pixel against the numpy statement tests/_jpeg_decode_ref.py (itself
pinned to Pillow in tests/test_jpeg_decode_cpu.py) and, for a subset, against Pillow directly.  Sizes: 1 x 1; 7 x 13 (less than one
MCU); 16 x 16 (exactly one 4:2:0 MCU); 17 x 23 (partial MCUs both ways, odd chroma extents through the fancy upsampling); 33 x 16;
40 x 72 (3 MCU rows of 4:2:0, 5 of 4:4:4: the index pass of a file without restart markers crosses them); 16 x 1000: a workgroup
walks 96 blocks at a time = 16 MCUs of 4:2:0 or 32 of 4:4:4, so a row's segment is four or five chunks with a partial last one and
the reader's state and the DC predictors are carried."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _jpeg_cases as C
import _jpeg_decode_cases as DC
import _jpeg_decode_ref as R
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def reference(data):
    px, status = R.decode(data)
    assert status == 0
    px.setflags(write=False)
    return px


def decode_one(data, **kw):
    frames, status = ops.jpeg_decode(data, **kw)
    assert status.dtype == torch.int32 and tuple(status.shape) == (1,) and status.is_cuda
    return frames[0].cpu().numpy(), int(status[0])


@pytest.mark.parametrize("hw", C.SIZES)
def test_pixels_equal_the_reference(hw):
    mine = [c for c in C.cases() if c[0] == hw]
    assert {c[3] for c in mine} == {0, 2} and {c[2] for c in mine} == {5, 75, 100} and {c[4] for c in mine} == {1, 2, 50}
    for _, kind, q, sub, r in mine:
        for rr in (r, 0):
            f = C.pillow(C.image(hw, kind), q, sub, rr)
            got, status = decode_one(f)
            assert got.dtype == np.uint8 and got.shape == hw + (3,)
            assert status == 0 and np.array_equal(got, reference(f)), (hw, kind, q, sub, rr, status, int((got != reference(f)).sum()))


@pytest.mark.parametrize("name,data", DC.extra_files(), ids=[n for n, _ in DC.extra_files()])
def test_other_files_equal_the_reference_and_pillow(name, data):
    got, status = decode_one(data)
    assert status == 0 and np.array_equal(got, reference(data)) and np.array_equal(got, DC.pillow_pixels(data))


@pytest.mark.parametrize("hw", ((17, 23), (40, 72), C.WIDE))
def test_pixels_equal_pillows(hw):
    for kind, q, sub, r in (("smooth", 75, 2, 1), ("noise", 100, 0, 2), ("checker", 100, 2, 1), ("smooth", 5, 0, 50), ("noise", 5, 2, 0)):
        f = C.pillow(C.image(hw, kind), q, sub, r)
        got, status = decode_one(f)
        assert status == 0 and np.array_equal(got, DC.pillow_pixels(f)), (hw, kind, q, sub, r)


def test_a_batch_whose_images_differ():
    hw = (40, 72)
    for sub in (0, 2):
        for r in (1, 0):                                                  # with restart markers, and through the index walk: 5 / 3 MCU rows
            files = [C.pillow(C.image(hw, "smooth"), 75, sub, r), C.pillow(C.image(hw, "noise"), 100, sub, r),
                     DC.save(C.image(hw, "checker"), quality=5, subsampling=sub, optimize=True, restart_marker_rows=r)]
            infos = [ops.jpeg_parse(f) for f in files]
            assert len({i["quant_tables"][0] for i in infos}) == 3 and infos[2]["huffman_tables"] != infos[0]["huffman_tables"]
            assert infos[0]["restart_interval"] == (r and (9 if sub == 0 else 5))
            frames, status = ops.jpeg_decode(files)
            assert frames.shape == (3,) + hw + (3,) and status.cpu().tolist() == [0, 0, 0]
            for b, f in enumerate(files):
                assert np.array_equal(frames[b].cpu().numpy(), reference(f)), (sub, r, b)
            assert np.array_equal(frames[2].cpu().numpy(), DC.pillow_pixels(files[2]))


def test_to_tensor_is_frames_to_tensor_of_the_bytes():
    for hw, sub, r in (((17, 23), 2, 1), ((40, 72), 0, 0), (C.WIDE, 2, 1)):
        files = [C.pillow(C.image(hw, k), 75, sub, r) for k in ("smooth", "noise")]
        u8, s0 = ops.jpeg_decode(files)
        f32, s1 = ops.jpeg_decode(files, to_tensor=True)
        assert f32.dtype == torch.float32 and f32.shape == (2, 3) + hw and s0.cpu().tolist() == s1.cpu().tolist() == [0, 0]
        assert torch.equal(f32, ops.frames_to_tensor(u8))
    grey = dict(DC.extra_files())["grey-17x23"]
    assert torch.equal(ops.jpeg_decode(grey, to_tensor=True)[0], ops.frames_to_tensor(ops.jpeg_decode(grey)[0]))


def test_out_is_written_in_place_between_untouched_guards(monkeypatch):
    hw, guard = (17, 23), 64
    files = [C.pillow(C.image(hw, k), 75, 2, 1) for k in ("smooth", "noise")]
    n = 2 * hw[0] * hw[1] * 3
    for to_tensor, dtype, shape, fill in ((False, torch.uint8, (2,) + hw + (3,), 0xA5), (True, torch.float32, (2, 3) + hw, -7.0)):
        pool = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
        out = pool[guard:guard + n].view(shape)

        def no_readback(*a, **k):
            raise AssertionError("the call read a tensor back")
        for name in ("cpu", "item", "tolist"):                          # no read-back and no synchronisation inside the call
            monkeypatch.setattr(torch.Tensor, name, no_readback)
        monkeypatch.setattr(torch.cuda, "synchronize", no_readback)
        frames, status = ops.jpeg_decode(files, to_tensor=to_tensor, out=out)
        monkeypatch.undo()
        assert frames is out and status.cpu().tolist() == [0, 0]
        host = pool.cpu()
        assert (host[:guard] == fill).all() and (host[-guard:] == fill).all()
        want = torch.from_numpy(np.stack([reference(f) for f in files]))
        assert torch.equal(out.cpu(), want.permute(0, 3, 1, 2).float() / 255.0 if to_tensor else want)
    with pytest.raises(ValueError, match="out must be"):
        ops.jpeg_decode(files, out=torch.zeros((2,) + hw + (3,), dtype=torch.uint8, device=DEV)[:, :, ::2])


def test_round_trip_through_the_encoder():
    for hw in ((17, 23), (40, 72)):
        u8 = torch.stack([torch.from_numpy(C.image(hw, k).copy()) for k in ("smooth", "noise")]).to(DEV)
        f32 = ops.frames_to_tensor(u8)
        for x in (u8, f32):
            for sub in ("4:4:4", "4:2:0"):
                files = ops.jpeg_files(*ops.jpeg_encode(x, quality=75, subsampling=sub))
                frames, status = ops.jpeg_decode(files)
                assert status.cpu().tolist() == [0, 0]
                for b, f in enumerate(files):
                    assert np.array_equal(frames[b].cpu().numpy(), DC.pillow_pixels(f)), (hw, sub, b)
        # 4:4:4: the JPEG stage of the training degradations is the same round trip
        files = ops.jpeg_files(*ops.jpeg_encode(u8, quality=30, subsampling="4:4:4"))
        got = ops.jpeg_decode(files, to_tensor=True)[0]
        assert torch.equal(got, ops.degrade(f32, [(ops.DEGRADE_TAPS_OFF, 0, 0, 30, 0)] * 2))


def test_one_call_is_three_launches(monkeypatch):
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    grey = dict(DC.extra_files())["grey-40x72"]
    for files, kw in ((C.pillow(C.image((17, 23), "smooth"), 75, 2, 1), {}), ([C.pillow(C.image(C.WIDE, "noise"), 75, 0, 0)] * 3, {}),
                      ([C.pillow(C.image((40, 72), "smooth"), 75, 0, 2)] * 2, {"to_tensor": True}), (grey, {})):
        del calls[:]
        ops.jpeg_decode(files, **kw)
        assert calls == ["tup_jpeg_decode_index", "tup_jpeg_decode_blocks", "tup_jpeg_decode_finish"]      # whatever the size, the batch, the layout


def test_kernels_use_no_scratch():
    usage = os.path.join(ROOT, "transformerupscaler_amd", "csrc", "build", "resource_usage.json")
    if not os.path.exists(usage):
        pytest.fail(f"{usage} is not there: the build writes it")
    mine = {k: v for k, v in json.load(open(usage))["kernels"].items() if v["source"] == "jpeg_decode.hip"}
    assert len(mine) == 3 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] for v in mine.values()), mine


def test_damaged_scans_beside_a_good_image():
    """The handful of tests/_jpeg_decode_cases.gpu_damaged: inputs the same walker handled on the host under the sanitizers
    (tests/test_jpeg_decode_cpu.py).  Not a search: five fixed files, once."""
    picked = DC.gpu_damaged(ops.jpeg_parse)
    assert [n.split("-")[0] for n, _ in picked] == ["cut", "cut", "byte", "byte", "no"]
    good, hw, guard = DC.good(), (40, 72), 256
    files = [good] + [d for _, d in picked] + [good]
    n = len(files) * hw[0] * hw[1] * 3
    pool = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out = pool[guard:guard + n].view((len(files),) + hw + (3,))
    frames, status = ops.jpeg_decode(files, out=out)
    status = status.cpu().tolist()
    host = pool.cpu()
    assert (host[:guard] == 0xA5).all() and (host[-guard:] == 0xA5).all()
    assert status[0] == 0 and status[-1] == 0
    assert np.array_equal(frames[0].cpu().numpy(), reference(good)) and np.array_equal(frames[-1].cpu().numpy(), reference(good))
    for i, (name, data) in enumerate(picked):
        px, ref_status = R.decode(data)
        assert (status[1 + i] != 0) == (ref_status != 0), (name, status[1 + i], ref_status)      # a non-zero status ...
        if status[1 + i] == 0:
            assert np.array_equal(frames[1 + i].cpu().numpy(), px), name                          # ... or a complete decode
    assert status[1] != 0 and status[2] != 0 and status[5] != 0                   # the truncations and the file without its markers


def test_driver_scores_are_those_of_the_host_decode(tmp_path):
    """inference.py end to end in a child process (as tests/test_inference_driver.py runs it), on a JPEG input with restart markers:
    the files it wrote and its input are decoded on the GPU; its scores equal those computed here with `decode_image` forced to Pillow."""
    import inference
    src = str(tmp_path / "in.jpg")
    with open(src, "wb") as f:
        f.write(C.pillow(C.image((40, 72), "smooth"), 90, 2, 1))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--image_path", src, "--model", "BicubicInterpolation", "--scale", "2",
                        "--no-checkpoint", "--json", "rec.json", "--inp", "lr.jpg", "--out", "sr.jpg"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(tmp_path / "rec.json"))
    host = lambda p: inference.decode_image(str(tmp_path / p), DEV, gpu=False)
    for p in ("in.jpg", "lr.jpg", "sr.jpg"):                             # each of them goes to the GPU decoder, and gives Pillow's pixels
        data = open(tmp_path / p, "rb").read()
        assert ops.jpeg_parse(data)["restart_interval"] > 0
        assert torch.equal(inference.decode_image(str(tmp_path / p), DEV), host(p)) and torch.equal(inference.decode_image(data, DEV), host(p))
    scores = inference.score(host("in.jpg"), host("sr.jpg"), host("lr.jpg"))
    assert rec["scores"] == {k: {m: float(v) for m, v in d.items()} for k, d in scores.items()}
    png = str(tmp_path / "in.png")                                       # what the parser refuses still goes to Pillow
    from PIL import Image
    Image.fromarray(C.image((17, 23), "smooth")).save(png)
    assert torch.equal(inference.decode_image(png, DEV), torch.from_numpy(C.image((17, 23), "smooth").copy()).to(DEV))
