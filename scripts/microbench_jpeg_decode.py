"""Timing of the GPU JPEG decoder, after scripts/microbench_jpeg.py's method: alternating rounds after warm-up,
device-synchronised, median [range].

One 2160 x 3840 and one 4320 x 7680 frame, "smooth" and "natural" content (as in microbench_jpeg.py), saved by Pillow at quality 75,
4:2:0, (a) with a restart marker per MCU row and (b) without restart markers.  Printed per file:

  launches   the three launches of `ops.jpeg_decode` on an upload made beforehand, together and each alone (`tup_jpeg_decode_index`,
             `tup_jpeg_decode_blocks`, `tup_jpeg_decode_finish`), device time;
  op         `ops.jpeg_decode(file, out=...)` as a caller pays for it: the parse on the host, the upload, the launches, and a
             synchronisation at the end, wall clock;
  host       in the same session, what it replaces: Pillow's `Image.open().convert("RGB")` plus `torch.from_numpy().to(device)`,
             wall clock, three runs.

The status and the equality of the pixels with Pillow's are printed too.  --index {serial,sync} chooses launch 1 of case (b): "serial"
(the default) is one lane's walk per image, "sync" the self-synchronising index (`tup_jpeg_decode_index_sync`), whose sync rounds are
printed; with "sync" only case (b) is run, since launch 1 of case (a) is the same on either.  Compare the two from one session.
inference.py sends a file without restart markers to the GPU decoder only if "op" with --index sync lies below "host" for both
2160 x 3840 files.  Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, io, statistics, time, numpy as np, torch
from PIL import Image
from transformerupscaler_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--index", choices=("serial", "sync"), default="serial", help="launch 1 of the files without restart markers")
INDEX = ap.parse_args().index
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"
Q, SUB = 75, 2


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000          # us per call


def alternate(arms, n, rounds=5, warmup=2):
    res = {k: [] for k in arms}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, n))
    return res


def wall(fn, runs=3):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def show(label, v, unit="us", extra=""):
    print(f"{label}: median {statistics.median(v):.1f} {unit} [{min(v):.1f}-{max(v):.1f}]{extra}", flush=True)


def content(h, w, kind):
    rng = np.random.default_rng(h + len(kind))
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([x * (255.0 / (w - 1)), 128 + 100 * np.sin(x / 97.0 + y / 61.0), y * (255.0 / (h - 1))], -1)
    if kind == "natural":
        levels = rng.integers(-60, 61, (h // 120 + 1, w // 160 + 1, 3)).astype(np.float32)
        a += np.repeat(np.repeat(levels, 120, 0), 160, 1)[:h, :w]
        a += rng.normal(0, 4, a.shape).astype(np.float32)
    return np.clip(a, 0, 255).astype(np.uint8)


def host_decode(data):
    return torch.from_numpy(np.array(Image.open(io.BytesIO(data)).convert("RGB"))).to(dev)


for h, w in ((2160, 3840), (4320, 7680)):
    for kind in ("smooth", "natural"):
        pixels = content(h, w, kind)
        for case, rows in (("(a) a restart marker per MCU row", 1), ("(b) no restart markers", 0)):
            if rows and INDEX == "sync":
                continue
            buf = io.BytesIO()
            Image.fromarray(pixels).save(buf, "JPEG", quality=Q, subsampling=SUB, restart_marker_rows=rows)
            data = buf.getvalue()
            info = ops.jpeg_parse(data)
            layout, interval = ops._JPEG_LAYOUT[info["subsampling"]], info["restart_interval"]
            S, ws = ops._jpeg_decode_geometry(h, w, layout, interval)
            start, end = info["scan"]
            rec = ops._JPEG_DEC_REC.size
            blob = bytearray(rec + ((end - start + 15) & ~15))
            blob[:rec] = ops._jpeg_decode_record(info, data, 0)
            blob[rec:rec + end - start] = data[start:end]
            up = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
            segs = torch.empty((1, S, 8), dtype=torch.int32, device=dev)
            status = torch.empty((1,), dtype=torch.int32, device=dev)
            work = torch.empty((1, ws), dtype=torch.uint8, device=dev)
            out = torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev)
            st = ops._stream
            front = (up.data_ptr(), up.data_ptr() + rec, len(blob) - rec, 1, h, w, layout, interval, S, segs.data_ptr(), status.data_ptr())
            rounds = torch.zeros((1,), dtype=torch.int32, device=dev)
            sync = INDEX == "sync" and not rows
            index_name = "tup_jpeg_decode_index_sync" if sync else "tup_jpeg_decode_index"
            index = (lambda: _lib.call(index_name, *front[:7], segs.data_ptr(), status.data_ptr(), rounds.data_ptr(), st())) if sync else \
                (lambda: _lib.call(index_name, *front, st()))
            blocks = lambda: _lib.call("tup_jpeg_decode_blocks", *front, work.data_ptr(), ws, st())
            finish = lambda: _lib.call("tup_jpeg_decode_finish", work.data_ptr(), ws, 1, h, w, layout, out.data_ptr(), None, st())
            arms = {"all": lambda: (index(), blocks(), finish()), "index": index, "blocks": blocks, "finish": finish}
            res = alternate(arms, n=5, rounds=5, warmup=2) if rows or sync else alternate(arms, n=1, rounds=3, warmup=1)
            title = f"{h} x {w}, {kind}, {case}" + (f", index {INDEX}" if not rows else "")
            show(f"{title}, three launches", res["all"], extra=f"  file {len(data) / 1e6:.2f} MB, {S} segments")
            for name, what in (("index", index_name + (f" ({int(rounds[0])} sync rounds, {-(-(end - start) // ops.JPEG_SYNC_BYTES)} subsequences of "
                                                       f"{ops.JPEG_SYNC_BYTES} bytes)" if sync else "")), ("blocks", "tup_jpeg_decode_blocks"), ("finish", "tup_jpeg_decode_finish")):
                show(f"{title}, {what}", res[name])
            show(f"{title}, ops.jpeg_decode(out=...) with parse, upload and a final synchronisation", wall(lambda: ops.jpeg_decode(data, out=out, index=INDEX if not rows else "auto")), unit="ms")
            want = host_decode(data)
            show(f"{title}, Pillow open().convert('RGB') + upload", wall(lambda: host_decode(data)), unit="ms",
                 extra=f"  status {int(status[0])}, pixels equal to Pillow's: {bool(torch.equal(out[0], want))}")
            del up, segs, work, out, want
        torch.cuda.empty_cache()
