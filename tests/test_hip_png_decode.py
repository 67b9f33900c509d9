"""`ops.png_decode` (csrc/png_decode.hip) on the MI355X, bit for bit against the Python statement tests/_png_decode_ref.py (itself
pinned to Pillow and zlib in tests/test_png_decode_cpu.py) and against Pillow directly, for both walks.  The case files
(tests/_png_decode_cases.py) are decoded in batches of equal H x W, which also mixes colour types and stream lengths in one call.
Damaged streams are the ones csrc/png_inflate.h already walked on the host under the sanitizers."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import _png_decode_cases as C
import _png_decode_ref as R
from transformerupscaler_amd import _lib, data, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
WALKS = ("token", "wave")


@functools.lru_cache(maxsize=None)
def reference(file):
    px, status = R.decode(file)
    if px is not None:
        px.setflags(write=False)
    return px, status


@functools.lru_cache(maxsize=None)
def groups():
    """{(H, W): [Case]}"""
    out = {}
    for c in C.files():
        info = ops.png_parse(c.data)
        out.setdefault((info["H"], info["W"]), []).append(c)
    return out


@pytest.mark.parametrize("walk", WALKS)
def test_every_case_equals_reference_and_pillow(walk):
    assert {(1, 1), (1, 70), (70, 1), (5, 3), (65, 67), (150, 150), (300, 255)} <= set(groups())
    for (H, W), cases in groups().items():
        frames, status = ops.png_decode([c.data for c in cases], walk=walk)
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (len(cases), H, W, 3) and frames.is_cuda
        assert status.dtype == torch.int32 and tuple(status.shape) == (len(cases),) and status.is_cuda
        got, st = frames.cpu().numpy(), status.cpu().tolist()
        for b, c in enumerate(cases):
            want, _ = reference(c.data)
            assert st[b] == 0 and np.array_equal(got[b], want), (c.name, walk, st[b], int((got[b] != want).sum()))
            if C.claimed(c):
                assert np.array_equal(got[b], C.pillow_rgb(c.data)), (c.name, walk)


def test_one_file_as_bytes_and_auto():
    c = dict(C.files())["pillow_150x150_rgb_l6"]
    frames, status = ops.png_decode(c)
    assert tuple(frames.shape) == (1, 150, 150, 3) and int(status[0]) == 0
    assert np.array_equal(frames[0].cpu().numpy(), C.pillow_rgb(c))
    assert ops.PNG_AUTO_WALK in WALKS


@pytest.mark.parametrize("walk", WALKS)
def test_three_colour_types_in_one_call(walk):
    by_name = dict(C.files())
    files = [by_name["own_65x67_ct0"], by_name["pillow_P_l6"], by_name["own_65x67_ct6"]]
    assert len({len(f) for f in files}) == 3 and [ops.png_parse(f)["channels"] for f in files] == [1, 1, 4]
    frames, status = ops.png_decode(files, walk=walk)
    assert status.cpu().tolist() == [0, 0, 0]
    for b, f in enumerate(files):
        assert np.array_equal(frames[b].cpu().numpy(), C.pillow_rgb(f))


@pytest.mark.parametrize("walk", WALKS)
def test_to_tensor_and_out(walk):
    files = [c.data for c in groups()[(65, 67)][:5]]
    frames, _ = ops.png_decode(files, walk=walk)
    t, status = ops.png_decode(files, to_tensor=True, walk=walk)
    assert t.dtype == torch.float32 and tuple(t.shape) == (5, 3, 65, 67) and status.cpu().tolist() == [0] * 5
    assert torch.equal(t, ops.frames_to_tensor(frames))
    # out= is the tensor that is written: rows of guard around it stay as they were
    big = torch.full((7, 65, 67, 3), 0x5a, dtype=torch.uint8, device=DEV)
    got, _ = ops.png_decode(files, out=big[1:6], walk=walk)
    assert got.data_ptr() == big[1:6].data_ptr() and torch.equal(big[1:6], frames)
    assert bool((big[0] == 0x5a).all()) and bool((big[6] == 0x5a).all())
    bigf = torch.full((7, 3, 65, 67), -3.0, dtype=torch.float32, device=DEV)
    ops.png_decode(files, to_tensor=True, out=bigf[1:6], walk=walk)
    assert torch.equal(bigf[1:6], t) and bool((bigf[0] == -3.0).all()) and bool((bigf[6] == -3.0).all())
    for bad in (torch.empty((5, 65, 67, 3), dtype=torch.float32, device=DEV), torch.empty((4, 65, 67, 3), dtype=torch.uint8, device=DEV),
                torch.empty((5, 67, 65, 3), dtype=torch.uint8, device=DEV), torch.empty((5, 65, 67, 6), dtype=torch.uint8, device=DEV)[..., ::2]):
        with pytest.raises(ValueError, match="out must be"):
            ops.png_decode(files, out=bad)
    with pytest.raises(ValueError, match="out must be"):
        ops.png_decode(files, to_tensor=True, out=torch.empty((5, 65, 67, 3), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("walk", WALKS)
def test_logo(walk):
    logo = open(os.path.join(HERE, "golden", "logo_rgba.png"), "rb").read()
    frames, status = ops.png_decode(logo, walk=walk)
    assert int(status[0]) == 0 and np.array_equal(frames[0].cpu().numpy(), C.pillow_rgb(logo))


@pytest.mark.parametrize("walk", WALKS)
def test_damaged_streams(walk):
    """Every damaged stream between sound ones, through the C entries with guard rows around the workspace and the frames: its status
    is the reference's, its neighbours are exact, and nothing outside the call's own rows is touched."""
    cases = C.damaged()
    H, W = cases[0][1], cases[0][2]
    good = C.own(H, W, 0, (1, 4, 3, 2))
    good_px = torch.from_numpy(C.pillow_rgb(good).copy()).to(DEV)
    files, names = [good], ["good"]
    for n, (name, h, w, stream) in enumerate(cases):
        assert (h, w) == (H, W)
        files.append(C.png(H, W, 0, stream))
        names.append(name)
        if n % 7 == 6:
            files.append(good)
            names.append("good")
    files.append(good)
    names.append("good")
    B = len(files)
    infos = [ops.png_parse(f) for f in files]
    ws = _lib.load().tup_png_decode_workspace(H, W, 1)
    assert ws >= H * (1 + W) + 8 * W
    up, streams_bytes = ops._png_decode_upload(files, infos, torch.device(DEV))
    work = torch.full((B + 2, ws), 0xa5, dtype=torch.uint8, device=DEV)
    out = torch.full((B + 2, H, W, 3), 0x5a, dtype=torch.uint8, device=DEV)
    status = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("tup_png_decode_inflate", up.data_ptr(), up.data_ptr() + B * 784, streams_bytes, B, H, W, 1, int(walk == "wave"),
              work[1].data_ptr(), ws, status[1:].data_ptr(), stream)
    _lib.call("tup_png_decode_finish", up.data_ptr(), work[1].data_ptr(), ws, B, H, W, 1, out[1].data_ptr(), None, status[1:].data_ptr(), stream)
    st = status.cpu().tolist()
    assert st[0] == -7 and st[-1] == -7
    assert bool((work[0] == 0xa5).all()) and bool((work[-1] == 0xa5).all()) and bool((out[0] == 0x5a).all()) and bool((out[-1] == 0x5a).all())
    seen = set()
    for b, (name, f) in enumerate(zip(names, files)):
        if name == "good":
            assert st[1 + b] == 0 and torch.equal(out[1 + b], good_px), (b, st[1 + b])
        else:
            want = reference(f)[1]
            assert want != 0 and st[1 + b] == want, (name, st[1 + b], want)
            seen.add(want)
    assert seen == set(range(1, 11))
    # the same through ops.png_decode: one damaged image between two good ones
    frames, status = ops.png_decode([good, files[names.index("adler")], good], walk=walk)
    assert status.cpu().tolist() == [0, R.BAD_ADLER, 0] and torch.equal(frames[0], good_px) and torch.equal(frames[2], good_px)


def test_round_trip_with_the_encoder():
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (2, 40, 72, 3), dtype=torch.uint8, generator=g)
    frames[1] = torch.from_numpy(C.content(40, 72, 3, seed=4))
    frames = frames.to(DEV)
    for walk in WALKS:
        back, status = ops.png_decode(ops.png_files(*ops.png_encode(frames)), walk=walk)
        assert status.cpu().tolist() == [0, 0] and torch.equal(back, frames)
    deep = (frames.to(torch.int32) * 257).to(torch.uint16)
    with pytest.raises(ValueError, match="bit depth 16"):
        ops.png_decode(ops.png_files(*ops.png_encode(deep, bits=16)))


def test_data_path(tmp_path):
    by_name = dict(C.files())
    names = ["own_65x67_ct2", "pillow_P_l6", "own_5x3_ct6_adaptive", "pillow_RGBA_l9"]
    paths = []
    for k, n in enumerate(names):
        paths.append(str(tmp_path / f"{k:02d}_{n}.png"))
        open(paths[-1], "wb").write(by_name[n])
    from PIL import Image
    laced = str(tmp_path / "04_interlaced.png")
    # Pillow writes no Adam7 files: one pass of a 1 x 1 image is its own interlaced form
    open(laced, "wb").write(C.png(1, 1, 2, R.split(C.own(1, 1, 2, (0,)))[4], interlace=1))
    assert Image.open(laced).convert("RGB").size == (1, 1)
    paths.append(laced)
    host = data.decode_pngs(paths, DEV, "host")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        gpu = data.decode_pngs(paths, DEV, "gpu")
    assert len(caught) == 1 and "04_interlaced.png" in str(caught[0].message)
    for p, a, b in zip(paths, host, gpu):
        one = data.decode_png(p, DEV)
        assert b.dtype == torch.uint8 and b.is_cuda and torch.equal(a, one) and torch.equal(b, one), p
    with pytest.raises(ValueError, match="decoder"):
        data.decode_pngs(paths, DEV, "fast")

    # FrameCache.preload: index order, stops where the next image would not fit, counts its decodes
    ds = data.PairDataset(str(tmp_path), scale_pairs=[{"lr": (8, 8), "hr": (16, 16)}], cache_bytes=65 * 67 * 3 * 2 + 5 * 3 * 3 + 3, device=DEV)
    assert [os.path.basename(f) for f in ds.files] == [os.path.basename(p) for p in paths]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert ds.preload() == 3 and (ds.gpu_decodes, ds.decodes) == (3, 0)        # the fourth, 65 x 67 again, does not fit
        for i in range(3):
            assert torch.equal(ds.frame(i), host[i])
        assert (ds.gpu_decodes, ds.decodes) == (3, 0)
        assert ds.preload([4, 0]) == 1 and (ds.gpu_decodes, ds.decodes) == (3, 1)  # the interlaced file falls back to the host
        assert torch.equal(ds.frame(4), host[4]) and torch.equal(ds.frame(3), host[3]) and ds.decodes == 2
    other = data.PairDataset(str(tmp_path), scale_pairs=[{"lr": (8, 8), "hr": (16, 16)}], device=DEV)
    assert other.preload(decoder="host") == 5 and (other.gpu_decodes, other.decodes) == (0, 5)


def test_inference_decodes_a_png_on_request():
    import inference
    by_name = dict(C.files())
    f = by_name["pillow_RGBA_l6"]
    host, name = inference.decode_image_named(f, DEV)
    assert name == "pillow"
    gpu, name = inference.decode_image_named(f, DEV, png_decoder="gpu")
    assert name == "gpu:png" and torch.equal(gpu, host)
    laced = C.png(1, 1, 2, R.split(C.own(1, 1, 2, (0,)))[4], interlace=1)      # refused by png_parse: the host decodes it
    assert inference.decode_image_named(laced, DEV, png_decoder="gpu")[1] == "pillow"
