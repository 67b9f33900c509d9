"""Two builds of the library side by side on ops.patch_unembed; run on the MI355X box, one build per process:

    TUP_LIB_PATH=<build A> python3 scripts/ab_unembed.py dump A.json        SHA-256 of the outputs at the comparison shapes, fp32 and
    TUP_LIB_PATH=<build B> python3 scripts/ab_unembed.py dump B.json        bf16 tokens (the 8 x 720p map is 1.2 GB: too large to keep)
    python3 scripts/ab_unembed.py compare A.json B.json                     every pair the same bytes
    TUP_LIB_PATH=<build> [TUP_UNEMBED_WAVES=4|8] python3 scripts/ab_unembed.py time LABEL
                                                                            the kernel alone at 8 x 720p, bf16 tokens
    TUP_LIB_PATH=<diag build> [TUP_UNEMBED_WAVES=4|8] python3 scripts/ab_unembed.py legs LABEL
                                                                            ... and with each leg of the tile loop switched off
                                                                            (TUP_UNEMBED_ABLATE, a -DTUP_DIAG build of gemm_tokens.hip)
profiles/r18_unembed_legs.txt is its output for DESIGN 5l."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 19, 70), (3, 117, 440), (8, 720, 1280)]
BF16 = torch.bfloat16
LEGS = [(0, "full kernel"), (1, "(a) no weight DMA after tile 0"), (2, "(b) no skip loads"), (4, "(c) no output stores"), (8, "(d) no MFMAs")]


def operands(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 + H)
    nwy, nwx = ((H + 7) // 8 + 7) // 8, ((W + 7) // 8 + 7) // 8
    rows = B * nwy * nwx * 64
    x = torch.randn((rows, 192), generator=g)
    wt = (torch.randn((4096, 192), generator=g) * 0.05).to(BF16)
    bias = torch.randn((64,), generator=g) * 0.1
    skip = torch.randn((B, H, W, 64), generator=g).to(BF16)
    return x, wt, bias, skip


def digest(t):
    return hashlib.sha256(t.cpu().contiguous().view(torch.int16).numpy().tobytes()).hexdigest()


def dump(outfile):
    from transformerupscaler_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    for shape in SHAPES:
        x, wt, bias, skip = (t.to(dev) for t in operands(shape))
        res["%dx%dx%d f32 tokens" % shape] = digest(ops.patch_unembed(x, wt, bias, skip))
        res["%dx%dx%d bf16 tokens" % shape] = digest(ops.patch_unembed(x.to(BF16), wt, bias, skip))
    with open(outfile, "w") as fh:
        json.dump(res, fh, indent=1)
    print("dumped", outfile)


def compare(fa, fb):
    a, b = json.load(open(fa)), json.load(open(fb))
    ok = a.keys() == b.keys()
    for k in a:
        same = a[k] == b.get(k)
        ok &= same
        print(f"{k}: same bytes {same} (sha256 {a[k][:16]}...)", flush=True)
    print("ALL OK" if ok else "SOME FAILED")
    return 0 if ok else 1


def _median_us(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / 20)
    ts.sort()
    return ts


def time_call(label, legs):
    from transformerupscaler_amd import ops
    dev = torch.device("cuda:0")
    x, wt, bias, skip = (t.to(dev) for t in operands(SHAPES[-1]))
    x = x.to(BF16)
    waves = os.environ.get("TUP_UNEMBED_WAVES", "routed")
    for bits, what in (LEGS if legs else LEGS[:1]):
        os.environ["TUP_UNEMBED_ABLATE"] = str(bits)          # read at every launch by the diagnostic build, by no other
        ts = _median_us(lambda: ops.patch_unembed(x, wt, bias, skip))
        print(f"{label}: waves={waves} {what}: patch_unembed 8x720p bf16 tokens (20 calls back to back, 7 rounds): "
              f"median {ts[3]:.1f} us, min {ts[0]:.1f}, max {ts[-1]:.1f}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        time_call(sys.argv[2], sys.argv[1] == "legs")
