"""Timing of the GPU PNG decoder: alternating rounds after warm-up, device-synchronised, median [range].

2160 x 3840 frames of the two contents of scripts/microbench_png.py (smooth; natural = smooth plus edges and sensor-like noise), as files
written by Pillow at compress_level 1 and 6 and by `ops.png_encode`.  Per file and batch size B = 1, 8, 64 (the same file B times: the
work of a call does not depend on what the other images hold):

  GPU path    `ops.png_decode(files, walk=...)` end to end, wall clock: parse + upload + two launches + synchronise, for both walks;
              and each launch alone (stream events), at B = 1;
  host path   what `data.decode_png` does per file, Pillow's decode + convert("RGB") + the upload of the frame, measured on the loop of
              min(B, 8) files and scaled to B (the loop is serial).

A call of a natural 4K file takes seconds, so B = 1 runs one warm-up and two rounds per walk, B = 8 and 64 one round, and the launches
are timed alone at B = 1 only.  The last line says which walk is faster at B = 1: that is what `ops.PNG_AUTO_WALK` is set to.

`--preload` runs the other measurement instead, in a directory of 16 natural 2160 x 3840 files (Pillow level 1): `FrameCache.preload`
with decoder="gpu" against decoder="host", twice each, and `train.py --max_steps 1 --batch_size 1 --pairs 96x96:192x192` as a child
process with `--png_decoder gpu` against `host`, twice each: the process's wall clock to the end of its first step (`host` decodes
the one image that step uses, `gpu` preloads the directory first).

There is no threshold.  Needs a GPU.  --quick: one content, B = 1 and 8 (4 files with --preload)."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import io, statistics, subprocess, tempfile, time, numpy as np, torch
from PIL import Image
from transformerupscaler_amd import _lib, data, ops

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"
QUICK = "--quick" in sys.argv[1:]
PRELOAD = "--preload" in sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 2160, 3840
BATCHES = (1, 8) if QUICK else (1, 8, 64)


def content(h, w, kind):
    rng = np.random.default_rng(h + len(kind))
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([x * (255.0 / (w - 1)), 128 + 100 * np.sin(x / 97.0 + y / 61.0), y * (255.0 / (h - 1))], -1)
    if kind == "natural":
        levels = rng.integers(-60, 61, (h // 120 + 1, w // 160 + 1, 3)).astype(np.float32)
        a += np.repeat(np.repeat(levels, 120, 0), 160, 1)[:h, :w]
        a += rng.normal(0, 4, a.shape).astype(np.float32)
    return np.clip(a, 0, 255).astype(np.uint8)


def show(label, v, unit="ms", extra=""):
    print(f"{label}: median {statistics.median(v):.2f} {unit} [{min(v):.2f}-{max(v):.2f}]{extra}", flush=True)
    return statistics.median(v)


def wall_alternating(arms, rounds, warmup=1):
    res = {k: [] for k in arms}
    for r in range(warmup + rounds):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                res[k].append((time.perf_counter() - t) * 1e3)
    return res


def launches(files, walk):
    """the two launches alone, by stream events -> (inflate ms, finish ms), medians of 2 (the kernels are warm by then)"""
    B = len(files)
    infos = [ops.png_parse(f) for f in files]
    ch = max(s["channels"] for s in infos)
    ws = _lib.load().tup_png_decode_workspace(H, W, ch)
    up, nbytes = ops._png_decode_upload(files, infos, torch.device(dev))
    work = torch.empty((B, ws), dtype=torch.uint8, device=dev)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    st = ops._stream
    times = ([], [])
    for _ in range(2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.call("tup_png_decode_inflate", up.data_ptr(), up.data_ptr() + B * 784, nbytes, B, H, W, ch, int(walk == "wave"), work.data_ptr(), ws,
                  status.data_ptr(), st())
        ev[1].record()
        _lib.call("tup_png_decode_finish", up.data_ptr(), work.data_ptr(), ws, B, H, W, ch, out.data_ptr(), None, status.data_ptr(), st())
        ev[2].record()
        torch.cuda.synchronize()
        times[0].append(ev[0].elapsed_time(ev[1]))
        times[1].append(ev[1].elapsed_time(ev[2]))
    assert status.cpu().tolist() == [0] * B
    return statistics.median(times[0]), statistics.median(times[1])


def host_decode(file):
    with Image.open(io.BytesIO(file)) as im:
        arr = np.asarray(im.convert("RGB"))
    return torch.from_numpy(arr.copy()).to(dev)


def table():
    faster = {}
    for kind in (("natural",) if QUICK else ("natural", "smooth")):
        frame = content(H, W, kind)
        made = {}
        for level in (1, 6):
            buf = io.BytesIO()
            Image.fromarray(frame).save(buf, "PNG", compress_level=level)
            made[f"Pillow level {level}"] = buf.getvalue()
        made["ops.png_encode"] = ops.png_files(*ops.png_encode(torch.from_numpy(frame).to(dev)[None]))[0]
        for writer, file in made.items():
            title = f"{H} x {W}, {kind}, {writer} ({len(file) / 1e6:.2f} MB)"
            got, status = ops.png_decode(file)
            assert int(status[0]) == 0 and np.array_equal(got[0].cpu().numpy(), frame), title
            for B in BATCHES:
                files = [file] * B
                res = wall_alternating({w: (lambda w=w: ops.png_decode(files, walk=w)) for w in ("token", "wave")}, rounds=2 if B == 1 else 1,
                                       warmup=1 if B == 1 else 0)
                med = {w: show(f"{title}, B = {B}, ops.png_decode(walk={w!r}) end to end", res[w], extra=f"  {statistics.median(res[w]) / B:.2f} ms a file") for w in res}
                if B == 1:
                    faster[(kind, writer)] = min(med, key=med.get)
                n = min(B, 8)
                hres = wall_alternating({"host": lambda: [host_decode(f) for f in files[:n]]}, rounds=2, warmup=1 if B == 1 else 0)["host"]
                hmed = show(f"{title}, B = {B}, host path: Pillow decode + upload, loop of {n}", hres, extra=f"  {statistics.median(hres) / n:.2f} ms a file")
                print(f"{title}, B = {B}: host loop / GPU = {hmed / n * B / min(med.values()):.2f} (scaled to {B} files)", flush=True)
                if B == 1:
                    for w in ("token", "wave"):
                        a, b = launches(files, w)
                        print(f"{title}, B = {B}, walk={w!r}: inflate launch {a:.2f} ms, unfilter + finish launch {b:.2f} ms", flush=True)
            torch.cuda.empty_cache()
    print("faster walk at B = 1:", {f"{k[0]} / {k[1]}": v for k, v in faster.items()}, " ops.PNG_AUTO_WALK =", ops.PNG_AUTO_WALK, flush=True)


def preload():
    with tempfile.TemporaryDirectory() as d:
        for i in range(4 if QUICK else 16):
            Image.fromarray(np.roll(content(H, W, "natural"), 37 * i, axis=1)).save(os.path.join(d, f"image_{i:02d}.png"), compress_level=1)
        for decoder in ("gpu", "host", "gpu", "host"):
            ds = data.PairDataset(d, cache_bytes=4 << 30, device=dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = ds.preload(decoder=decoder)
            torch.cuda.synchronize()
            print(f"FrameCache.preload of {n} files of {H} x {W} (Pillow level 1), decoder={decoder!r}: {(time.perf_counter() - t) * 1e3:.0f} ms "
                  f"(gpu_decodes {ds.gpu_decodes}, decodes {ds.decodes})", flush=True)
            del ds
            torch.cuda.empty_cache()
        env = dict(os.environ, PYTHONPATH=ROOT)
        for decoder in ("host", "gpu", "host", "gpu"):
            with tempfile.TemporaryDirectory() as ckpt:
                t = time.perf_counter()
                r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--data_dir", d, "--checkpoint_dir", ckpt, "--epochs", "1",
                                    "--max_steps", "1", "--batch_size", "1", "--pairs", "96x96:192x192", "--png_decoder", decoder],
                                   cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                dt = time.perf_counter() - t
            assert r.returncode == 0, r.stderr[-2000:]
            print(f"train.py --max_steps 1 --batch_size 1 --pairs 96x96:192x192 --png_decoder {decoder}: {dt:.1f} s from start to the end of "
                  f"the first step", flush=True)


(preload if PRELOAD else table)()
