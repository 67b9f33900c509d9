"""Timing of patch-sample construction: five alternating runs after warm-up, device-synchronised, median [range].

B = 64 patches of LR side 96 from four 2160 x 3840 frames, seeded random boxes and flip / rotate variants, at scales 2 and 4:

  (a) the route to the same tensors through the ops that existed before: per sample a slice, the flips and the transpose as torch
      views, one copy to make the crop contiguous, `ops.resize_frames` (two launches) and `ops.frames_to_tensor`;
  (b) `ops.patch_pairs`: one `tup_patch_pairs` launch and its record upload;
  (c) the launch of (b) alone on a table that is already on the device, as GB/s against the bytes it must move,
      B * (3 P^2 read + 12 P^2 + 12 p^2 written).

(a) and (b) are compared bit for bit before they are timed.  `--B N` / `--p N` change the batch.  Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, statistics, numpy as np, torch
from transformerupscaler_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=64)
ap.add_argument("--p", type=int, default=96)
ap.add_argument("--scales", type=str, default="2,4")
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"


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


def show(label, v, extra=""):
    print(f"{label}: median {statistics.median(v):.1f} us [{min(v):.1f}-{max(v):.1f}]{extra}", flush=True)


def existing_route(frames, boxes, p, P):
    lrs, hrs = [], []
    for f, (y0, x0, op) in zip(frames, boxes):
        t = f[y0:y0 + P, x0:x0 + P]
        if op & 1:
            t = t.flip(1)
        if op & 2:
            t = t.flip(0)
        if op & 4:
            t = t.transpose(0, 1)
        t = t.contiguous()
        lrs.append(ops.resize_frames(t, (p, p), to_tensor=True)[0])
        hrs.append(ops.frames_to_tensor(t)[0])
    return lrs, hrs


g = torch.Generator().manual_seed(0)
H, W = 2160, 3840
pool = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(4)]
B, p = args.B, args.p
for scale in (int(v) for v in args.scales.split(",")):
    P = p * scale
    rng = np.random.default_rng(scale)
    frames = [pool[int(rng.integers(len(pool)))] for _ in range(B)]
    boxes = [(int(rng.integers(H - P + 1)), int(rng.integers(W - P + 1)), int(rng.integers(8))) for _ in range(B)]
    lr, hr = ops.patch_pairs(frames, boxes, p, scale)
    lrs, hrs = existing_route(frames, boxes, p, P)
    assert torch.equal(lr, torch.stack(lrs)) and torch.equal(hr, torch.stack(hrs)), "the two routes differ"
    out = (lr, hr)
    # (c): the same launch on a resident table
    table = torch.frombuffer(bytearray(b"".join(ops._PATCH_REC.pack(f.data_ptr(), H, W, y0, x0, op, 0) for f, (y0, x0, op) in zip(frames, boxes))),
                             dtype=torch.int64).to(dev)
    lo, n, k, ks = ops._pil_taps_on(torch.device(dev, torch.cuda.current_device()), P, p)
    launch = lambda: _lib.call("tup_patch_pairs", table.data_ptr(), B, P, p, lo.data_ptr(), n.data_ptr(), k.data_ptr(), ks,
                               hr.data_ptr(), lr.data_ptr(), ops._stream())
    res = alternate({"a": lambda: existing_route(frames, boxes, p, P), "b": lambda: ops.patch_pairs(frames, boxes, p, scale, out=out),
                     "c": launch}, n=20)
    med = {key: statistics.median(v) for key, v in res.items()}
    moved = B * (3 * P * P + 12 * P * P + 12 * p * p)
    title = f"B = {B}, p = {p}, x{scale} (HR {P})"
    show(f"{title}, (a) existing ops: per sample the flips, a copy and three launches", res["a"])
    show(f"{title}, (b) ops.patch_pairs, one launch + record upload", res["b"], f"  = (a) / {med['a'] / med['b']:.1f}")
    show(f"{title}, (c) tup_patch_pairs alone", res["c"], f"  = {moved / (med['c'] * 1e-6) / 1e9:.0f} GB/s of {moved / 1e6:.1f} MB")
