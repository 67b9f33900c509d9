"""Timing and file sizes of the GPU PNG encoder: alternating rounds after warm-up, device-synchronised, median [range].

One 2160 x 3840 and one 4320 x 7680 frame under the two contents of scripts/microbench_jpeg.py (smooth; natural = smooth plus edges and
sensor-like noise), adaptive filtering, at three values of `block_bytes` (what picks the default).  Printed per frame, content and
block size: `ops.png_encode` with out= given from the uint8 frame and from the fp32 tensor (four launches, no synchronisation), each
launch alone (uint8 input), and the file's length.  Then, wall clock, three runs each:

  GPU path    ops.png_encode(fp32 tensor, out=...) at the default block size + the read-back of the file's bytes;
  host path   ops.tensor_to_frames + the copy of the uint8 frame to the host + Pillow's save(..., "PNG", compress_level=1), and the
              same at compress_level=6 (one run: it takes seconds);

with the three files' lengths, and `ops.jpeg_encode` of the same frame for scale.  The GPU's file is decoded by Pillow and compared with
the frame.  There is no threshold: nothing earlier does this work.  Needs a GPU.

`--bits16` runs only the comparison of the two depths instead: per 2160 x 3840 content, an fp32 frame with more than 8 bits in it (the
8-bit content plus a sub-level dither, so that the low bytes of the 16-bit samples are busy, as a model's output's are) encoded by
`ops.png_encode(x, out=...)` at bits=8 and at bits=16, default block size, alternating; time and file length of both.  The 16-bit
stream is twice as long, so about twice the time is the figure to compare with."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import io, statistics, time, numpy as np, torch
from PIL import Image
from transformerupscaler_amd import _lib, ops

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"
BITS16 = "--bits16" in sys.argv[1:]
BLOCKS = (4096, 16384, 32768)
ADAPTIVE = ops.PNG_FILTERS["adaptive"]


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


def wall(fn, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out, r


print(f"default block_bytes = {ops.PNG_BLOCK_BYTES}", flush=True)
if BITS16:
    h, w = 2160, 3840
    for kind in ("smooth", "natural"):
        x8 = ops.frames_to_tensor(torch.from_numpy(content(h, w, kind)).to(dev)[None])
        x = (x8 + torch.rand(x8.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 255.0).clamp_(0.0, 1.0)
        out = {b: (torch.empty((1, ops.png_max_bytes(h, w, bits=b)), dtype=torch.uint8, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
               for b in (8, 16)}
        res = alternate({b: (lambda b=b: ops.png_encode(x, out=out[b], bits=b)) for b in (8, 16)}, n=3)
        size = {b: int(out[b][1][0]) for b in (8, 16)}
        for b in (8, 16):
            show(f"{h} x {w}, {kind} + dither, ops.png_encode(fp32, out=..., bits={b}), four launches", res[b], extra=f"  file {size[b] / 1e6:.2f} MB")
        print(f"{h} x {w}, {kind} + dither: 16 / 8 bits = {statistics.median(res[16]) / statistics.median(res[8]):.2f} x the time, "
              f"{size[16] / size[8]:.2f} x the bytes", flush=True)
    sys.exit(0)
for h, w in ((2160, 3840), (4320, 7680)):
    for kind in ("smooth", "natural"):
        host = content(h, w, kind)
        frame = torch.from_numpy(host).to(dev)[None]
        x = ops.frames_to_tensor(frame)
        title = f"{h} x {w}, {kind}"
        st = ops._stream
        for bb in BLOCKS:
            N = _lib.load().tup_png_blocks(h, w, bb)
            data = torch.empty((1, ops.png_max_bytes(h, w, bb)), dtype=torch.uint8, device=dev)
            lengths = torch.empty((1,), dtype=torch.int32, device=dev)
            ops.png_encode(frame, block_bytes=bb, out=(data, lengths))
            n, cap = int(lengths[0]), int(data.shape[1])
            work = torch.empty((3, 1, N), dtype=torch.int32, device=dev)
            adlers = torch.empty((1,), dtype=torch.int32, device=dev)
            rows = torch.empty((1, h), dtype=torch.uint8, device=dev)
            p = frame.data_ptr()
            arms = {
                "op_u8": lambda: ops.png_encode(frame, block_bytes=bb, out=(data, lengths)),
                "op_f32": lambda: ops.png_encode(x, block_bytes=bb, out=(data, lengths)),
                "filters": lambda: _lib.call("tup_png_filters", p, None, 1, h, w, rows.data_ptr(), st()),
                "sizes": lambda: _lib.call("tup_png_sizes", p, None, 1, h, w, ADAPTIVE, bb, rows.data_ptr(), work[0].data_ptr(), work[2].data_ptr(), st()),
                "offsets": lambda: _lib.call("tup_png_offsets", work[0].data_ptr(), work[2].data_ptr(), 1, h, w, bb, cap, work[1].data_ptr(),
                                             lengths.data_ptr(), adlers.data_ptr(), st()),
                "write": lambda: _lib.call("tup_png_write", p, None, 1, h, w, ADAPTIVE, bb, rows.data_ptr(), work[1].data_ptr(), lengths.data_ptr(),
                                           adlers.data_ptr(), data.data_ptr(), cap, st()),
            }
            res = alternate(arms, n=3)
            tag = f"{title}, block_bytes {bb} ({N} blocks)"
            show(f"{tag}, ops.png_encode(uint8, out=...), four launches", res["op_u8"], extra=f"  file {n / 1e6:.2f} MB")
            show(f"{tag}, ops.png_encode(fp32, out=...), four launches", res["op_f32"])
            for name, what in (("filters", "tup_png_filters (row filters)"), ("sizes", "tup_png_sizes (sizing pass)"), ("offsets", "tup_png_offsets (scan)"),
                               ("write", "tup_png_write (writing pass)")):
                show(f"{tag}, {what}", res[name])
            del data, work
        bb = ops.PNG_BLOCK_BYTES
        data = torch.empty((1, ops.png_max_bytes(h, w, bb)), dtype=torch.uint8, device=dev)
        lengths = torch.empty((1,), dtype=torch.int32, device=dev)

        def gpu_path():
            ops.png_encode(x, out=(data, lengths))
            return data[0, :int(lengths[0])].cpu().numpy().tobytes()

        def host_path(level):
            buf = io.BytesIO()
            Image.fromarray(ops.tensor_to_frames(x)[0].cpu().numpy()).save(buf, "PNG", compress_level=level)
            return buf.getvalue()
        gpu_path()
        t_gpu, mine = wall(gpu_path, 3)
        t1, pil1 = wall(lambda: host_path(1), 3)
        t6, pil6 = wall(lambda: host_path(6), 1)
        ok = np.array_equal(np.asarray(Image.open(io.BytesIO(mine)).convert("RGB")), host)
        show(f"{title}, GPU path: ops.png_encode(fp32, out=...) + read-back of the bytes", t_gpu, unit="ms",
             extra=f"  file {len(mine) / 1e6:.2f} MB, Pillow decodes it to the frame: {ok}")
        show(f"{title}, host path: tensor_to_frames + copy + Pillow save(compress_level=1)", t1, unit="ms",
             extra=f"  file {len(pil1) / 1e6:.2f} MB, GPU file / this = {len(mine) / len(pil1):.3f}")
        show(f"{title}, host path: tensor_to_frames + copy + Pillow save(compress_level=6)", t6, unit="ms",
             extra=f"  file {len(pil6) / 1e6:.2f} MB, GPU file / this = {len(mine) / len(pil6):.3f}")
        jd, jl = ops.jpeg_encode(frame)
        jres = alternate({"jpeg": lambda: ops.jpeg_encode(frame, out=(jd, jl))}, n=3, rounds=3, warmup=1)
        show(f"{title}, for scale: ops.jpeg_encode(uint8, out=...) at quality 75", jres["jpeg"], extra=f"  file {int(jl[0]) / 1e6:.2f} MB")
        del data, x, frame
        torch.cuda.empty_cache()
