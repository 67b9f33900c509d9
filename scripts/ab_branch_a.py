"""Two builds of the library side by side on the composed branch A (r = 2); run on the MI355X box, one build per process:

    TUP_LIB_PATH=<build A> python3 scripts/ab_branch_a.py dump DIR_A        outputs at the comparison shapes
    TUP_LIB_PATH=<build B> python3 scripts/ab_branch_a.py dump DIR_B
    python3 scripts/ab_branch_a.py compare DIR_A DIR_B                      interior torch.equal; ring error of each against fp64 (CPU)
    TUP_LIB_PATH=<build> [TUP_BRA_ABLATE=n] python3 scripts/ab_branch_a.py time LABEL
                                                                            row kernel + ring kernel at 8 x 720p (the ablation
                                                                            bits need a -DTUP_DIAG build of conv3x3_c64.hip)
profiles/r14_bra_live_taps_ab.txt is its output for the change of DESIGN 5i."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _bra_live_ref as L  # noqa: E402
from transformerupscaler_amd import packing  # noqa: E402

SHAPES = [(2, 19, 70), (3, 117, 440), (2, 720, 1280)]


def weights():
    g = torch.Generator().manual_seed(77)
    wu, bu, w3 = torch.randn((256, 64, 3, 3), generator=g) * 0.04, torch.randn((256,), generator=g) * 0.1, torch.randn((3, 64, 3, 3), generator=g) * 0.04
    return packing.pack_branch_a(wu, bu, w3, 2)


def feat(shape):
    B, H, W = shape
    return torch.randn((B, H, W, 64), generator=torch.Generator().manual_seed(100 + H)).to(torch.bfloat16)


def name(d, shape, relu):
    return os.path.join(d, "y_%d_%d_%d_%d.pt" % (shape + (int(relu),)))


def dump(outdir):
    from transformerupscaler_amd import ops
    dev = torch.device("cuda:0")
    wp, bias, wv, bv = (t.to(dev) for t in weights())
    os.makedirs(outdir, exist_ok=True)
    for shape in SHAPES:
        x = feat(shape).to(dev)
        for relu in (True, False):
            torch.save(ops.branch_a_composed(x, wp, bias, wv, bv, 2, relu=relu).cpu(), name(outdir, shape, relu))
    print("dumped", outdir)


def compare(da, db):
    wp, bias, wv, bv = weights()
    ok = True
    for shape in SHAPES:
        B, H, W = shape
        x = feat(shape)
        Hs, Ws = 2 * H, 2 * W
        ring = torch.zeros((Hs, Ws), dtype=torch.bool)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
        for relu in (True, False):
            ya, yb = torch.load(name(da, shape, relu)), torch.load(name(db, shape, relu))
            same = torch.equal(ya[:, :, ~ring], yb[:, :, ~ring])
            # fp64 ring reference from four three-pixel strips (a strip's own far edge is not used)
            ref = torch.zeros((B, 3, Hs, Ws), dtype=torch.float64)
            k = min(3, H)
            top, bot = (L.apply_fp64(t, wp, bias, wv, bv, 2, relu) for t in (x[:, :k], x[:, H - k:]))
            k = min(3, W)
            lef, rig = (L.apply_fp64(t.contiguous(), wp, bias, wv, bv, 2, relu) for t in (x[:, :, :k], x[:, :, W - k:]))
            ref[:, :, :, 0], ref[:, :, :, -1] = lef[:, :, :, 0], rig[:, :, :, -1]
            ref[:, :, 0], ref[:, :, -1] = top[:, :, 0], bot[:, :, -1]
            ea = (ya.double() - ref)[:, :, ring].abs().max().item()
            eb = (yb.double() - ref)[:, :, ring].abs().max().item()
            good = same and eb <= 2 * ea
            ok &= good
            print(f"{shape} relu={int(relu)}: interior equal {same}; ring max|err| vs fp64: A {ea:.3e} B {eb:.3e} "
                  f"(ring values that differ: {int((ya[:, :, ring] != yb[:, :, ring]).sum())} of {int(ring.sum()) * 3 * B}) -> {'OK' if good else 'FAIL'}",
                  flush=True)
    print("ALL OK" if ok else "SOME FAILED")
    return 0 if ok else 1


def time_call(label):
    from transformerupscaler_amd import ops
    dev = torch.device("cuda:0")
    wp, bias, wv, bv = (t.to(dev) for t in weights())
    x = torch.randn((8, 720, 1280, 64), generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev)
    for _ in range(5):
        ops.branch_a_composed(x, wp, bias, wv, bv, 2)
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            ops.branch_a_composed(x, wp, bias, wv, bv, 2)
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / 20)
    ts.sort()
    print(f"{label}: ablate={os.environ.get('TUP_BRA_ABLATE', '0')} branch_a_composed 8x720p (both kernels, 20 calls back to back): "
          f"median {ts[3]:.1f} us, min {ts[0]:.1f}, max {ts[-1]:.1f}")


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        time_call(sys.argv[2])
