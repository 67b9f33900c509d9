"""Timing of the NV12 and P010 frame conversions beside their RGB24 neighbours ("NV12 frames", "P010 frames"): alternating
rounds after warm-up, device events around many launches, median [range] per launch.

Per shape (H x W, B frames) six arms, each one C-ABI launch into preallocated buffers:

  nv12 -> f32   `tup_nv12_to_f32chw`    reads 1.5 B, writes 12 B per pixel
  rgb24 -> f32  `tup_u8hwc_to_f32chw`   reads 3 B,   writes 12 B per pixel
  f32 -> nv12   `tup_f32chw_to_nv12`    reads 12 B,  writes 1.5 B per pixel
  f32 -> rgb24  `tup_f32chw_to_u8hwc`   reads 12 B,  writes 3 B per pixel
  p010 -> f32   `tup_p010_to_f32chw`    reads 3 B,   writes 12 B per pixel
  f32 -> p010   `tup_f32chw_to_p010`    reads 12 B,  writes 3 B per pixel

Every launch works on the next of a ring of buffer sets whose total exceeds the 256 MB last-level cache several times, so that no
launch finds its operands cached by the one before.  The NV12 surfaces are single buffers [B][3H/2][W] (Y on top, UV below).
Effective bandwidth = the bytes above over the median time.  The expectation is stated by the byte counts: an NV12 arm moves the
same fp32 bytes and half the uint8 bytes of its RGB24 neighbour, so it should take no longer; a P010 arm moves exactly its RGB24
neighbour's 15 B per pixel, so it should take as long; the allowance is the neighbour's own spread (max - min over its rounds).  The
P010 surfaces are uint16 [B][3H/2][W] with random codes in the high ten bits.  `--shapes 720x1280x1,...` changes the list.  Needs a GPU.

`--once` times nothing: per shape it launches each arm three times on one buffer set and goes on, which is the run to put under
`rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <dir> -- python3 scripts/microbench_nv12.py --once --shapes 2160x3840x8`
(and again with `WRITE_SIZE`, a pass each; `Counter_Value` is in KB and reads count x 2 on gfx950, scripts/pmc_traffic.py): the source of
profiles/r09_pmc_traffic_nv12.txt."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, statistics, torch
from transformerupscaler_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=str, default="720x1280x1,720x1280x8,2160x3840x1,2160x3840x8")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--once", action="store_true", help="no timing: three launches of each arm per shape, for a counter pass")
ap.add_argument("--ring_mb", type=int, default=1024, help="least total size of the rotated buffer sets")
args = ap.parse_args()

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", torch.cuda.current_device())


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000          # us per launch


def alternate(arms, n, rounds, warmup=2):
    res = {k: [] for k in arms}
    for _ in range(warmup):
        for fn in arms.values():
            for _ in range(n):
                fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, n))
    return res


def rotating(launch, nsets):
    state = [0]

    def fn():
        state[0] = (state[0] + 1) % nsets
        launch(state[0])
    return fn


for spec in args.shapes.split(","):
    H, W, B = (int(v) for v in spec.split("x"))
    px = B * H * W
    set_bytes = px * (12 + 12 + 3 + 3 + 1.5 + 1.5 + 3 + 3)
    nsets = 1 if args.once else max(3, -(-args.ring_mb * 2 ** 20 // int(set_bytes)))
    g = torch.Generator(device=dev).manual_seed(H + B)
    sets = []
    for _ in range(nsets):
        surf = torch.randint(0, 256, (B, H + H // 2, W), dtype=torch.uint8, device=dev, generator=g)
        rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        x = torch.rand((B, 3, H, W), device=dev, generator=g)
        surf10 = (torch.randint(0, 1024, (B, H + H // 2, W), dtype=torch.int32, device=dev, generator=g) << 6).to(torch.int16).view(torch.uint16)
        sets.append({"surf": surf, "rgb": rgb, "x": x, "f_out": torch.empty_like(x), "surf_out": torch.empty_like(surf),
                     "rgb_out": torch.empty_like(rgb), "surf10": surf10, "surf10_out": torch.empty_like(surf10)})
    st = ops._stream()
    pitch, bs = W, (H + H // 2) * W

    def nv12_dec(i):
        s = sets[i]
        p = s["surf"].data_ptr()
        _lib.call("tup_nv12_to_f32chw", p, p + H * pitch, bs, pitch, bs, pitch, s["f_out"].data_ptr(), B, H, W, 1, 0, st)

    def rgb_dec(i):
        s = sets[i]
        _lib.call("tup_u8hwc_to_f32chw", s["rgb"].data_ptr(), s["f_out"].data_ptr(), B, H, W, 0, st)

    def nv12_enc(i):
        s = sets[i]
        p = s["surf_out"].data_ptr()
        _lib.call("tup_f32chw_to_nv12", s["x"].data_ptr(), p, p + H * pitch, bs, pitch, bs, pitch, B, H, W, 1, 0, st)

    def rgb_enc(i):
        s = sets[i]
        _lib.call("tup_f32chw_to_u8hwc", s["x"].data_ptr(), s["rgb_out"].data_ptr(), B, H, W, 0, st)

    def p010_dec(i):
        s = sets[i]
        p = s["surf10"].data_ptr()
        _lib.call("tup_p010_to_f32chw", p, p + 2 * H * pitch, 2 * bs, 2 * pitch, 2 * bs, 2 * pitch, s["f_out"].data_ptr(), B, H, W, 1, 0, st)

    def p010_enc(i):
        s = sets[i]
        p = s["surf10_out"].data_ptr()
        _lib.call("tup_f32chw_to_p010", s["x"].data_ptr(), p, p + 2 * H * pitch, 2 * bs, 2 * pitch, 2 * bs, 2 * pitch, B, H, W, 1, 0, st)

    # the launch above and the ops wrapper agree (same planes, same bytes) before anything is timed
    if not args.once:
        nv12_dec(0); nv12_enc(0)
        assert torch.equal(sets[0]["f_out"], ops.nv12_to_tensor(*ops.nv12_planes(sets[0]["surf"], H, W)))
        y, uv = ops.tensor_to_nv12(sets[0]["x"])
        yo, uvo = ops.nv12_planes(sets[0]["surf_out"], H, W)
        assert torch.equal(y, yo) and torch.equal(uv, uvo)
        same16 = lambda a, b: torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
        p010_dec(0); p010_enc(0)
        assert torch.equal(sets[0]["f_out"], ops.p010_to_tensor(*ops.p010_planes(sets[0]["surf10"], H, W)))
        y, uv = ops.tensor_to_p010(sets[0]["x"])
        yo, uvo = ops.p010_planes(sets[0]["surf10_out"], H, W)
        assert same16(y, yo) and same16(uv, uvo)

    arms = {"nv12 -> f32": (nv12_dec, 13.5), "rgb24 -> f32": (rgb_dec, 15.0), "f32 -> nv12": (nv12_enc, 13.5), "f32 -> rgb24": (rgb_enc, 15.0),
            "p010 -> f32": (p010_dec, 15.0), "f32 -> p010": (p010_enc, 15.0)}
    if args.once:
        for _ in range(3):
            for fn, _ in arms.values():
                fn(0)
        torch.cuda.synchronize()
        print(f"{H} x {W}, B = {B}: three launches of each arm, nothing timed", flush=True)
        del sets
        torch.cuda.empty_cache()
        continue
    n = int(min(3000, max(50, 128e9 // (px * 13.5))))          # tens of milliseconds per timing
    res = alternate({k: rotating(fn, nsets) for k, (fn, _) in arms.items()}, n, args.rounds)
    print(f"{H} x {W}, B = {B}: {nsets} buffer sets of {set_bytes / 2 ** 20:.0f} MB, {n} launches per timing, {args.rounds} rounds", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, (_, bpp) in arms.items():
        v = res[k]
        print(f"  {k:13s} median {med[k]:8.1f} us [{min(v):.1f}-{max(v):.1f}]  = {px * bpp / (med[k] * 1e-6) / 1e12:.2f} TB/s of {px * bpp / 1e6:.1f} MB", flush=True)
    for new, old in (("nv12 -> f32", "rgb24 -> f32"), ("f32 -> nv12", "f32 -> rgb24"), ("p010 -> f32", "rgb24 -> f32"), ("f32 -> p010", "f32 -> rgb24")):
        spread = max(res[old]) - min(res[old])
        verdict = "within" if med[new] <= med[old] + spread else "BEYOND"
        print(f"  {new} / {old} = {med[new] / med[old]:.3f}; {med[new] - med[old]:+.1f} us against the neighbour's spread of {spread:.1f} us: {verdict}", flush=True)
    del sets
    torch.cuda.empty_cache()
