"""The 8-wave form of patch_unembed (gemm_panel2_kernel<A_BF16 | A_F32, E_UNEMBED, 8>: one 256-row workgroup and one weight stream per
CU) at the smallest shapes at which it can go wrong, bit for bit against torch in float64.

launch_panel takes that form only when there is a 256-row workgroup for every CU, which no quick shape reaches, so the GPU cases run
in ONE child process started with TUP_UNEMBED_WAVES=8 (the launcher reads the switch once per process; this process keeps its routed
forms for every other test).  The child writes every output and the guard zones round it to a file; the tests here compare.

Operands are the integers of tests/_gemm_exact_ref.py's unembed_case (amplitude 7, K = 192: every partial sum is an integer below
2**24, so fp32 accumulates exactly in any order and a bf16 output is the round-to-nearest-even of an exact value); the reference is its
float64 evaluation.  test_references_exact shows the precondition without a GPU."""
import contextlib
import functools
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # the child process runs this file as a script
    sys.path.insert(0, ROOT)

import _exact_ref as R          # noqa: E402 -- tests/ is on sys.path (rootdir-less test modules)
import _gemm_exact_ref as G     # noqa: E402

BF16 = torch.bfloat16

# (B, (H, W)): token rows in window layout, and what the shape exercises in a 256-row, 8-wave workgroup
CASES = [
    (3, (40, 56)),        # 192 rows: waves 6 and 7 have no rows but must carry their DMA pieces and barriers
    (5, (40, 56)),        # 320 rows: a second workgroup with two live waves
    (1, (72, 136)),       # 384 rows: 1.5 workgroups, padded token rows and columns inside live waves
    (2, (43, 61)),        # pixel crop inside patches, H and W not multiples of 8
]
WAYS = [(tok, skip) for tok in ("f32", "bf16") for skip in ("skip", "noskip")]
GUARD = 4096              # bf16 elements of sentinel on each side of `out`
SENTINEL = -12288.0       # a bf16 value no output reaches (|out| <= 192 * 49 + 14)


def _cid(case):
    return "%dx%dx%d" % (case[0], case[1][0], case[1][1])


@contextlib.contextmanager
def _batch(b):
    """unembed_case and its references read the batch size from the module (G.B); the cases here vary it."""
    saved, G.B = G.B, b
    try:
        yield
    finally:
        G.B = saved


@functools.lru_cache(maxsize=None)
def build(case):
    """operands (CPU fp32) and, per dtype, the expected maps with and without `skip`; computed once per case, never modified."""
    b, hw = case
    with _batch(b):
        c = G.unembed_case("ft", hw)
        o = dict(c.operands)
        exp = {}
        for dtype in (torch.float32, torch.float64):
            with_skip = c.refs(dtype)["map"]
            c.operands["skip"] = torch.zeros_like(o["skip"])
            exp[dtype] = {"skip": with_skip, "noskip": c.refs(dtype)["map"]}
            c.operands["skip"] = o["skip"]
    return o, exp


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_references_exact(case):
    """float32 and float64 torch agree bit for bit, on integers below 2**24: the reference depends on no association order."""
    b, (H, W) = case
    o, exp = build(case)
    ht, wt = (H + 7) // 8, (W + 7) // 8
    assert o["x"].shape[0] == b * ((ht + 7) // 8) * ((wt + 7) // 8) * 64
    for key in ("skip", "noskip"):
        e32, e64 = exp[torch.float32][key], exp[torch.float64][key]
        assert e32.dtype == torch.float32 and e64.dtype == torch.float64 and e64.shape == (b, H, W, 64)
        assert torch.equal(e32.double(), e64), f"{_cid(case)} {key}: fp32 and fp64 references differ"
        R.assert_exact_preconditions(e64, bf16_out=True, default_case=False)
        assert e64.abs().max().item() < abs(SENTINEL)
    assert not torch.equal(exp[torch.float64]["skip"], exp[torch.float64]["noskip"])


def _worker(outfile):
    """Child process (TUP_UNEMBED_WAVES=8 in its environment): every case four ways, `out` carved from a sentinel-filled allocation."""
    from transformerupscaler_amd import _lib, ops
    assert os.environ.get("TUP_UNEMBED_WAVES") == "8"
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    dev = torch.device("cuda:0")
    from transformerupscaler_amd import packing
    res = {}
    for case in CASES:
        b, (H, W) = case
        o, _ = build(case)
        wp = packing.pack_linear(o["w"].permute(2, 3, 1, 0).reshape(4096, 192)).to(dev)          # n = (i*8+j)*64 + o
        bias, skip = o["b"].to(dev), R.nhwc_bf16(o["skip"]).to(dev)
        n = b * H * W * 64
        for tok, sk in WAYS:
            x = (o["x"].to(BF16) if tok == "bf16" else o["x"]).to(dev)
            big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=BF16, device=dev)
            out = big[GUARD:GUARD + n]
            _lib.call("tup_patch_unembed_fwd", x.data_ptr(), int(tok == "bf16"), wp.data_ptr(), bias.data_ptr(),
                      skip.data_ptr() if sk == "skip" else None, out.data_ptr(), b, H, W, ops._stream())
            torch.cuda.synchronize()
            res[f"{_cid(case)}/{tok}/{sk}"] = big.cpu()
    torch.save(res, outfile)


@pytest.fixture(scope="module")
def wide_outputs(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    outfile = str(tmp_path_factory.mktemp("unembed_wide") / "out.pt")
    env = dict(os.environ, TUP_UNEMBED_WAVES="8")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), outfile], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"the 8-wave child process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return torch.load(outfile)


@pytest.mark.gpu
@pytest.mark.parametrize("way", WAYS, ids=lambda w: "-".join(w))
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_unembed_wide(wide_outputs, case, way):
    b, (H, W) = case
    tok, sk = way
    big = wide_outputs[f"{_cid(case)}/{tok}/{sk}"]
    n = b * H * W * 64
    _, exp = build(case)
    what = f"8-wave patch_unembed {_cid(case)} {tok} tokens, {sk}"
    R.assert_bit_equal(big[GUARD:GUARD + n].view(b, H, W, 64), R.out_of(exp[torch.float64][sk], True), layout=None, what=what)
    guard = torch.full((GUARD,), SENTINEL, dtype=BF16)
    assert torch.equal(big[:GUARD], guard), f"{what}: wrote in front of `out`"
    assert torch.equal(big[GUARD + n:], guard), f"{what}: wrote behind `out`"


if __name__ == "__main__":
    _worker(sys.argv[1])
