"""Timing of the training degradations: five alternating runs after warm-up, device-synchronised, median [range].

B = 64 LR patches of side 96 (what `ops.patch_pairs` makes at scale 2 from four 2160 x 3840 frames, seeded boxes), one
`tup_degrade_lr` launch on a record table that is already on the device, under three tables:

  all       every stage on for every sample: blur of sigma 1.2, colour noise of sigma 6, JPEG at quality 75;
  jpeg      the JPEG round trip alone, quality 75;
  identity  every stage off: the quantisation to bytes and back.

Then one `tup_degrade_lr_sub` launch (csrc/degrade420.hip) on the same batch in the same alternating rounds: "all" and "jpeg" with
every record flagged 4:2:0 (`ops.DEGRADE_JPEG_420`), and "all" without the flag, which runs the 4:4:4 stages inside that kernel.

Printed: us per launch and GB/s against the bytes a launch must move, B * 24 * p^2 (fp32 in, fp32 out).  Beside them, for scale, the
`tup_patch_pairs` launch that builds the same batch, and `ops.degrade` itself (the launch plus the record upload) under "all".
There is no threshold: nothing earlier does this work.  `--B N` / `--p N` change the batch.  Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, statistics, numpy as np, torch
from transformerupscaler_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=64)
ap.add_argument("--p", type=int, default=96)
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


def resident(records):
    raw = b"".join(ops._DEGRADE_REC.pack(*ops._degrade_record(i, r)) for i, r in enumerate(records))
    return torch.frombuffer(bytearray(raw), dtype=torch.int64).to(dev)


g = torch.Generator().manual_seed(0)
H, W, scale = 2160, 3840, 2
pool = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(4)]
B, p = args.B, args.p
P = p * scale
rng = np.random.default_rng(scale)
frames = [pool[int(rng.integers(len(pool)))] for _ in range(B)]
boxes = [(int(rng.integers(H - P + 1)), int(rng.integers(W - P + 1)), int(rng.integers(8))) for _ in range(B)]
lr, hr = ops.patch_pairs(frames, boxes, p, scale)
out = torch.empty_like(lr)

every = [(ops.blur_taps(1.2), ops.noise_amp(6), 1000 + i, 75, 0) for i in range(B)]
tables = {"all": resident(every), "jpeg": resident([(ops.DEGRADE_TAPS_OFF, 0, 0, 75, 0)] * B), "identity": resident([ops.DEGRADE_OFF] * B)}
ptable = torch.frombuffer(bytearray(b"".join(ops._PATCH_REC.pack(f.data_ptr(), H, W, y0, x0, op, 0) for f, (y0, x0, op) in zip(frames, boxes))),
                          dtype=torch.int64).to(dev)
lo, n, k, ks = ops._pil_taps_on(torch.device(dev, torch.cuda.current_device()), P, p)


def launch(table, entry="tup_degrade_lr"):
    return lambda: _lib.call(entry, lr.data_ptr(), table.data_ptr(), B, p, p, out.data_ptr(), ops._stream())


assert torch.equal(ops.degrade(lr, [ops.DEGRADE_OFF] * B), lr), "the identity table changes patch_pairs' output"
arms = {name: launch(t) for name, t in tables.items()}
sub = ops.DEGRADE_JPEG_420
arms["all420"] = launch(resident([r[:4] + (r[4] | sub,) for r in every]), "tup_degrade_lr_sub")
arms["jpeg420"] = launch(resident([(ops.DEGRADE_TAPS_OFF, 0, 0, 75, sub)] * B), "tup_degrade_lr_sub")
arms["all444sub"] = launch(tables["all"], "tup_degrade_lr_sub")
arms["pairs"] = lambda: _lib.call("tup_patch_pairs", ptable.data_ptr(), B, P, p, lo.data_ptr(), n.data_ptr(), k.data_ptr(), ks,
                                  hr.data_ptr(), lr.data_ptr(), ops._stream())
arms["op"] = lambda: ops.degrade(lr, every, out=out)
res = alternate(arms, n=20)
moved = B * 24 * p * p
title = f"B = {B}, p = {p}"
for name, what in (("all", "blur + noise + JPEG"), ("jpeg", "JPEG alone"), ("identity", "every stage off")):
    med = statistics.median(res[name])
    show(f"{title}, tup_degrade_lr, {what}", res[name], f"  = {moved / (med * 1e-6) / 1e9:.0f} GB/s of {moved / 1e6:.1f} MB")
for name, what in (("all420", "blur + noise + JPEG 4:2:0"), ("jpeg420", "JPEG 4:2:0 alone"), ("all444sub", "blur + noise + JPEG, no record flagged")):
    show(f"{title}, tup_degrade_lr_sub, {what}", res[name], f"  = {statistics.median(res[name]) / statistics.median(res['all']):.2f} x tup_degrade_lr's blur + noise + JPEG")
show(f"{title}, ops.degrade, blur + noise + JPEG, launch + record upload", res["op"])
show(f"{title}, tup_patch_pairs at x{scale} (builds the batch)", res["pairs"])
