"""The self-synchronising index of `ops.jpeg_decode` for files without restart markers (csrc/jpeg_sync.hip) on the MI355X:
`ops.jpeg_scan_index(index="sync")` against `index="serial"` row by row (status, first MCU, predictors and the logical bit a record
denotes: 8 x the payload bytes before `pos`, stuffed zeros not counted, minus `n`), and `ops.jpeg_decode(index="sync")` bit for bit
against `index="serial"` and against Pillow.  The files are those of tests/_jpeg_sync_ref.cases(), which tests/test_jpeg_sync_cpu.py
walks on the host: less than one subsequence, cropped MCUs, many row starts in one subsequence, more than one span of 256
subsequences with stuffed bytes and a boundary on a stuffed zero, custom tables, scans of k T - 1, k T and k T + 1 bytes, and a flat
image with one-symbol tables (two bits a block, the most block ends a span can hold)."""
import numpy as np
import pytest
import torch

import _jpeg_decode_cases as DC
import _jpeg_sync_ref as S
from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu
T = ops.JPEG_SYNC_BYTES


def logical_bits(scan, segs):
    """segs int [S][8] of a scan that decodes completely -> the logical bit of every record"""
    raw = np.frombuffer(scan, dtype=np.uint8)
    stuffed = np.zeros(len(raw) + 1, dtype=np.int64)
    stuffed[2:] = np.cumsum((raw[1:] == 0) & (raw[:-1] == 0xFF))       # stuffed zeros at an index below pos
    pos, n = segs[:, 0].astype(np.int64), segs[:, 3].astype(np.int64)
    assert (n >= 0).all() and (n <= 32).all() and (pos >= 0).all() and (pos <= len(raw)).all()
    return 8 * (pos - stuffed[pos]) - n


@pytest.mark.parametrize("name,data", S.cases(), ids=[n for n, _ in S.cases()])
def test_sync_index_and_decode_equal_the_serial_ones(name, data):
    info = ops.jpeg_parse(data)
    scan = data[info["scan"][0]:info["scan"][1]]
    assert info["restart_interval"] == 0
    if name == "noise-256x256-q95":                                     # what this case is for (the seed was found by search on the CPU)
        assert len(scan) > 256 * T and scan.count(b"\xff\x00") > 0
        assert any(scan[k - 1] == 0xFF and scan[k] == 0 for k in range(T, len(scan), T))     # a boundary on the 00 of a pair
    if name == "flat-grey-optimize-4096x4096":                          # two bits a block: more than 2^17 block ends in the first span
        assert len(scan) * 4 == 512 * 512 and 256 * T * 4 > 1 << 17
    got = {}
    for index in ("serial", "sync"):
        segs, status, rounds = ops.jpeg_scan_index(data, index=index)
        assert segs.dtype == status.dtype == rounds.dtype == torch.int32 and segs.is_cuda and tuple(segs.shape[::2]) == (1, 8)
        got[index] = (segs[0].cpu().numpy(), status.cpu().tolist(), int(rounds[0]))
    (a, sa, ra), (b, sb, rb) = got["serial"], got["sync"]
    assert sa == sb == [0] and ra == 0
    nsub = -(-len(scan) // T)
    assert 0 <= rb <= nsub, (rb, nsub)
    assert np.array_equal(a[:, 4:], b[:, 4:])                           # the three predictors and the first MCU of every row
    assert np.array_equal(a[:, 1], b[:, 1]) and (b[:, 1] == len(scan)).all()
    assert np.array_equal(logical_bits(scan, a), logical_bits(scan, b))
    want = DC.pillow_pixels(data)
    frames = {}
    for index in ("serial", "sync"):
        u8, status = ops.jpeg_decode(data, index=index)
        f32, status32 = ops.jpeg_decode(data, to_tensor=True, index=index)
        assert status.cpu().tolist() == status32.cpu().tolist() == [0]
        frames[index] = (u8, f32)
    assert torch.equal(frames["sync"][0], frames["serial"][0]) and torch.equal(frames["sync"][1], frames["serial"][1])
    assert np.array_equal(frames["sync"][0][0].cpu().numpy(), want)
    assert torch.equal(frames["sync"][1], ops.frames_to_tensor(frames["sync"][0]))
    assert torch.equal(ops.jpeg_decode(data)[0], frames["sync"][0])     # index="auto"


def test_a_batch_with_damaged_scans_is_word_for_word_the_serial_index():
    files = S.damaged_batch()
    a, sa, _ = ops.jpeg_scan_index(files, index="serial")
    b, sb, rounds = ops.jpeg_scan_index(files, index="sync")
    sa, sb = sa.cpu().tolist(), sb.cpu().tolist()
    assert sa == sb and sa[0] == sa[2] == 0 and sa[1] != 0 and sa[3] != 0
    a, b = a.cpu().numpy(), b.cpu().numpy()
    for i, f in enumerate(files):
        info = ops.jpeg_parse(f)
        scan = f[info["scan"][0]:info["scan"][1]]
        assert 0 <= int(rounds[i]) <= -(-len(scan) // T)
        if sa[i]:
            assert np.array_equal(a[i], b[i]), i                        # the serial walk of the same launch
        else:
            assert np.array_equal(a[i][:, 4:], b[i][:, 4:]) and np.array_equal(logical_bits(scan, a[i]), logical_bits(scan, b[i])), i
    u8, status = ops.jpeg_decode(files, index="sync")
    u8s, statuss = ops.jpeg_decode(files, index="serial")
    assert status.cpu().tolist() == statuss.cpu().tolist() == sa
    for i in (0, 2):                                                     # the undamaged images are unaffected
        assert np.array_equal(u8[i].cpu().numpy(), DC.pillow_pixels(files[i])) and torch.equal(u8[i], u8s[i])


def test_one_call_is_three_launches_by_either_index(monkeypatch):
    calls = []
    real = _lib.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)

    def no_readback(*a, **k):
        raise AssertionError("the call read a tensor back")
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, no_readback)
    monkeypatch.setattr(torch.cuda, "synchronize", no_readback)
    data = dict(S.cases())["gradient-optimize"]
    for index, first in (("sync", "tup_jpeg_decode_index_sync"), ("serial", "tup_jpeg_decode_index")):
        del calls[:]
        ops.jpeg_decode([data, data], index=index)
        assert calls == [first, "tup_jpeg_decode_blocks", "tup_jpeg_decode_finish"]
        del calls[:]
        ops.jpeg_scan_index(data, index=index)
        assert calls == [first]


def test_sync_is_refused_for_files_with_restart_markers_before_any_launch(monkeypatch):
    marked = DC.save(np.zeros((16, 16, 3), np.uint8), quality=75, subsampling=2, restart_marker_rows=1)
    plain = dict(S.cases())["420-16x16"]

    def no_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", no_call)
    for fn in (ops.jpeg_decode, ops.jpeg_scan_index):
        with pytest.raises(ValueError, match="without restart markers"):
            fn(marked, index="sync")
        with pytest.raises(ValueError, match="index must be one of"):
            fn(plain, index="fast")


def test_driver_sends_a_file_without_restart_markers_to_the_sync_index(monkeypatch):
    import io
    import inference
    from PIL import Image
    seen = []
    real = ops.jpeg_decode
    monkeypatch.setattr(ops, "jpeg_decode", lambda data, **kw: (seen.append(kw.get("index")), real(data, **kw))[1])
    plain = dict(S.cases())["gradient-optimize"]
    marked = DC.save(np.full((16, 16, 3), 77, np.uint8), quality=75, subsampling=2, restart_marker_rows=1)
    png = io.BytesIO()
    Image.fromarray(np.full((9, 5, 3), 200, np.uint8)).save(png, "PNG")
    for data, index, name in ((plain, "sync", "gpu:sync-index"), (marked, "serial", "gpu:restart-intervals"), (png.getvalue(), None, "pillow")):
        del seen[:]
        got, decoder = inference.decode_image_named(data, "cuda")
        assert seen == ([index] if index else []) and decoder == name
        assert np.array_equal(got.cpu().numpy(), DC.pillow_pixels(data))
        assert torch.equal(inference.decode_image(data, "cuda"), got) and inference.decode_image(data, "cuda").decoder == name
    assert inference.decode_image_named(plain, "cuda", gpu=False)[1] == "pillow"


def test_kernel_uses_no_scratch():
    import json
    import os
    usage = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transformerupscaler_amd", "csrc", "build", "resource_usage.json")
    if not os.path.exists(usage):
        pytest.fail(f"{usage} is not there: the build writes it")
    mine = {k: v for k, v in json.load(open(usage))["kernels"].items() if v["source"] == "jpeg_sync.hip"}
    assert len(mine) == 1 and all(v["scratch_bytes_per_lane"] == 0 and v["guarded_no_scratch"] for v in mine.values()), mine
