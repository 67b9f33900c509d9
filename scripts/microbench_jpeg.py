"""Timing of the GPU JPEG encoder: alternating rounds after warm-up, device-synchronised, median [range].

One 2160 x 3840 and one 4320 x 7680 uint8 frame at quality 75, 4:2:0, a restart marker per MCU row, under two contents:

  smooth    gradients and a slow sinusoid: few coefficients survive the quantiser;
  natural   the same plus edges (a grid of rectangles of random level) and sensor-like noise of sigma 4: what a photograph costs.

Printed per frame and content: `ops.jpeg_encode` with out= given (its three launches, no synchronisation), each launch alone
(`tup_jpeg_sizes`, `tup_jpeg_offsets`, `tup_jpeg_write`), and in the same session what the host path costs: the copy of the uint8
frame to the host plus Pillow's `save()` of it (wall clock, three runs).  Last, for the 2160 x 3840 frame, the FastTransformer
forward at scale 2 that produces a frame of that size (deterministic weights, fp32 in and out; an 8K output is beyond the sizes the
model's kernels are run at).  The file's length and its equality with Pillow's file are printed too.
There is no threshold: nothing earlier does this work.  Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib, io, statistics, time, numpy as np, torch
from PIL import Image
from transformerupscaler_amd import _lib, ops

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"
Q, SUB, R = 75, 2, 1


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


model = importlib.import_module("models.FastTransformer.model").TransformerModel()
from transformerupscaler_amd.weights import deterministic_state_dict
model.load_state_dict(deterministic_state_dict(0), strict=False)
model = model.to(dev).eval()

for h, w in ((2160, 3840), (4320, 7680)):
    for kind in ("smooth", "natural"):
        host = content(h, w, kind)
        frame = torch.from_numpy(host).to(dev)[None]
        data, lengths = ops.jpeg_encode(frame, Q, SUB, R)
        n = int(lengths[0])
        S = _lib.load().tup_jpeg_segments(h, w, SUB, R)
        work = torch.empty((2, 1, S), dtype=torch.int32, device=dev)
        header = ops._jpeg_header_on(frame.device, (h, w, Q, SUB, R))
        st = ops._stream
        arms = {
            "op": lambda: ops.jpeg_encode(frame, Q, SUB, R, out=(data, lengths)),
            "sizes": lambda: _lib.call("tup_jpeg_sizes", frame.data_ptr(), None, 1, h, w, Q, SUB, R, work[0].data_ptr(), st()),
            "offsets": lambda: _lib.call("tup_jpeg_offsets", work[0].data_ptr(), 1, S, header.numel(), n, work[1].data_ptr(), lengths.data_ptr(), st()),
            "write": lambda: _lib.call("tup_jpeg_write", frame.data_ptr(), None, 1, h, w, Q, SUB, R, header.data_ptr(), header.numel(),
                                       work[1].data_ptr(), lengths.data_ptr(), data.data_ptr(), n, st()),
        }
        res = alternate(arms, n=5)
        title = f"{h} x {w}, {kind}"
        show(f"{title}, ops.jpeg_encode(out=...), three launches", res["op"], extra=f"  file {n / 1e6:.2f} MB")
        for name, what in (("sizes", "tup_jpeg_sizes (sizing pass)"), ("offsets", "tup_jpeg_offsets (scan)"), ("write", "tup_jpeg_write (writing pass)")):
            show(f"{title}, {what}", res[name])
        pil = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(frame[0].cpu().numpy()).save(buf, "JPEG", quality=Q, subsampling=SUB, restart_marker_rows=R)
            pil.append((time.perf_counter() - t) * 1e3)
        same = ops.jpeg_files(data, lengths)[0] == buf.getvalue()
        show(f"{title}, copy to the host + Pillow save()", pil, unit="ms", extra=f"  file equal to the GPU's: {same}")
    if h == 2160:                                   # the largest output the model's kernels are run and tested at
        x = torch.rand((1, 3, h // 2, w // 2), device=dev)
        with torch.no_grad():
            fwd = alternate({"forward": lambda: model(x, upscale_factor=2)}, n=2, rounds=3, warmup=1)
        show(f"{h} x {w}, FastTransformer forward x2 from {h // 2} x {w // 2} (B = 1)", [v / 1000 for v in fwd["forward"]], unit="ms")
        del x
    torch.cuda.empty_cache()
