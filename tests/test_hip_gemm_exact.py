"""Exact-operand tests of csrc/gemm_tokens.hip on the MI355X: every Linear, patch_embed and patch_unembed entry of the three model
families, forward and backward, against torch on the CPU, bit for bit.

The operands are integers of amplitude 7 (tests/_gemm_exact_ref.py): every partial sum is an integer below 2**24, the fp32 result
is exact in any summation order, a bf16 output is the round-to-nearest-even of an exact value, and an addressing error (a token row
of the wrong window, a reflected line, a padded token that reaches the map, a row beyond M) changes some output by at least 1.
Every comparison is torch.equal with the torch reference, never with another HIP kernel and never within a bound;
tests/test_gemm_exact_cpu.py shows without a GPU that each reference is exact and that the bf16 outputs really round.

Shapes are the smallest at which each path can go wrong; _gemm_exact_ref.py names what each exercises."""
import pytest
import torch

import _exact_ref as R          # tests/ is on sys.path (rootdir-less test modules)
import _gemm_exact_ref as G

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
ids = G._sid


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from transformerupscaler_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _eq(got, exp, what):
    R.assert_bit_equal(got, exp, layout=None, what=what)


def _map(t, dev):
    return R.nhwc_bf16(t).to(dev)


def _pack(w2d, dev):
    from transformerupscaler_amd import packing
    return packing.pack_linear(w2d).to(dev)


def _embed_w(w, dev):
    """conv weight [N][64][8][8] -> [N][4096], k = (i*8+j)*64 + c"""
    return _pack(w.permute(0, 2, 3, 1).reshape(w.shape[0], 4096), dev)


def _unembed_w(w, dev):
    """transposed-conv weight [K][64][8][8] -> [4096][K], n = (i*8+j)*64 + o"""
    return _pack(w.permute(2, 3, 1, 0).reshape(4096, w.shape[0]), dev)


@pytest.mark.parametrize("shape", G.LINEAR_SHAPES + G.BIG_SHAPES, ids=ids)
def test_gemm_tokens(dev, shape):
    """ops.gemm_tokens: 'bf16' with and without bias from bf16 A and from fp32 A, 'res' into a fresh output and in place.  K = 192 is
    the panel kernel, K = 64 / 128 the K-streaming one, (4133, 192, 256) the 256-row tile, (4095, 192, 256) the K-streaming one."""
    from transformerupscaler_amd import ops
    case = G.all_cases()[f"linear-{ids(shape)}"]()
    o, exp = case.operands, case.expected(torch.float64)
    a16, a32, wp, b, res = o["a"].to(BF16).to(dev), o["a"].to(dev), _pack(o["w"], dev), o["b"].to(dev), o["res"].to(dev)
    _eq(ops.gemm_tokens(a16, wp, b, "bf16"), exp["bf16"], f"gemm bf16 {shape}")
    _eq(ops.gemm_tokens(a16, wp, b, "res", res=res), exp["res"], f"gemm res {shape}")
    xs = res.clone()
    assert ops.gemm_tokens(a16, wp, b, "res", res=xs, out=xs) is xs
    _eq(xs, exp["res"], f"gemm res in place {shape}")
    if "nobias" in exp:
        _eq(ops.gemm_tokens(a16, wp, None, "bf16"), exp["nobias"], f"gemm bf16, no bias {shape}")
        _eq(ops.gemm_tokens(a32, wp, b, "bf16"), exp["bf16"], f"gemm bf16, fp32 A {shape}")
        _eq(ops.gemm_tokens(a32, wp, None, "bf16"), exp["nobias"], f"gemm bf16, fp32 A, no bias {shape}")


def _zero_rows(got, kind, hw, what):
    valid = G.valid_rows(*G.token_grid(kind, hw))
    assert bool((got.cpu()[~valid] == 0).all()), f"{what}: rows of padded tokens must be exact zeros"


@pytest.mark.parametrize("hw", G.HW_ODD, ids=ids)
def test_patch_embed_and_unembed_bwd(dev, hw):
    """ops.patch_embed (reflect padding) and ops.patch_unembed_bwd (zeros beyond the map): patch_embed_kernel<3>."""
    from transformerupscaler_amd import ops
    cases = G.all_cases()
    c = cases[f"embed-ft192-{ids(hw)}"]()
    got = ops.patch_embed(_map(c.operands["map"], dev), _embed_w(c.operands["w"], dev), c.operands["b"].to(dev))
    _eq(got, c.expected(torch.float64)["tokens"], f"patch_embed {hw}")
    _zero_rows(got, "ft", hw, "patch_embed")
    c = cases[f"embed-ftb192-{ids(hw)}"]()
    got = ops.patch_unembed_bwd(_map(c.operands["map"], dev), _embed_w(c.operands["w"], dev))
    _eq(got, c.expected(torch.float64)["tokens"], f"patch_unembed_bwd {hw}")
    _zero_rows(got, "ftb", hw, "patch_unembed_bwd")


def test_rt_patch_embed_and_unembed_bwd(dev):
    """ops.rt_patch_embed (+ bias + pos) and ops.rt_patch_unembed_bwd: plain token grid, patch_embed_kernel<2>."""
    from transformerupscaler_amd import ops
    c = G.all_cases()[f"embed-rt128-{ids(G.HW_RT)}"]()
    o, exp = c.operands, c.expected(torch.float64)
    m, w = _map(o["map"], dev), _embed_w(o["w"], dev)
    _eq(ops.rt_patch_embed(m, w, o["b"].to(dev), o["pos"].to(dev)), exp["tokens"], "rt_patch_embed")
    _eq(ops.rt_patch_unembed_bwd(m, w), exp["nobias"], "rt_patch_unembed_bwd")


@pytest.mark.parametrize("N", [192, 128, 64])
def test_wt_patch_embed(dev, N):
    """ops.wt_patch_embed (remainder rows / columns dropped): patch_embed_kernel<3>, <2>, and at N = 64 the K-streaming kernel
    with the gather and the patch_embed epilogue."""
    from transformerupscaler_amd import ops
    hw = G.HW_ODD[0]
    c = G.all_cases()[f"embed-wt{N}-{ids(hw)}"]()
    o = c.operands
    got = ops.wt_patch_embed(_map(o["map"], dev), _embed_w(o["w"], dev), o["b"].to(dev))
    _eq(got, c.expected(torch.float64)["tokens"], f"wt_patch_embed N={N}")
    _zero_rows(got, "wt", hw, "wt_patch_embed")


@pytest.mark.parametrize("hw", G.HW_ODD, ids=ids)
def test_patch_unembed_and_embed_bwd(dev, hw):
    """ops.patch_unembed from fp32 and from bf16 tokens (gemm_panel2_kernel<A_F32 / A_BF16, E_UNEMBED>: the cropped map, + bias + skip)
    and ops.patch_embed_bwd (the padded map, neither)."""
    from transformerupscaler_amd import ops
    cases = G.all_cases()
    c = cases[f"unembed-ft192-{ids(hw)}"]()
    o, exp = c.operands, c.expected(torch.float64)
    w, b, skip = _unembed_w(o["w"], dev), o["b"].to(dev), _map(o["skip"], dev)
    _eq(ops.patch_unembed(o["x"].to(dev), w, b, skip), exp["map"], f"patch_unembed {hw}")
    _eq(ops.patch_unembed(o["x"].to(BF16).to(dev), w, b, skip), exp["map"], f"patch_unembed, bf16 tokens {hw}")
    c = cases[f"unembed-ftb192-{ids(hw)}"]()
    got = ops.patch_embed_bwd(c.operands["x"].to(dev), _unembed_w(c.operands["w"], dev), G.B, *hw)
    _eq(got, c.expected(torch.float64)["map"], f"patch_embed_bwd {hw}")


@pytest.mark.parametrize("hw", G.HW_MULT8, ids=ids)
def test_patch_embed_bwd_merge(dev, hw):
    """ops.patch_embed_bwd_merge with add2 absent and present, relu_src of +, 0 and - values, and the column sums of add1 (integer
    sums: exact despite the float atomics)."""
    from transformerupscaler_amd import ops
    c = G.all_cases()[f"unembed-merge192-{ids(hw)}"]()
    o, exp = c.operands, c.expected(torch.float64)
    x, w = o["x"].to(dev), _unembed_w(o["w"], dev)
    add1, add2, src = _map(o["skip"], dev), _map(o["add2"], dev), _map(o["relu_src"], dev)
    for key, a2 in (("one", None), ("two", add2)):
        got, cs = ops.patch_embed_bwd_merge(x, w, add1, a2, src, want_add1_colsum=True)
        _eq(got, exp[key], f"patch_embed_bwd_merge {key} {hw}")
        _eq(cs, exp["colsum"], f"patch_embed_bwd_merge column sums {key} {hw}")
        _eq(ops.patch_embed_bwd_merge(x, w, add1, a2, src), exp[key], f"patch_embed_bwd_merge {key}, no column sums {hw}")


def test_rt_patch_unembed_and_embed_bwd(dev):
    """ops.rt_patch_unembed (+ bias + skip) and ops.rt_patch_embed_bwd (+ add): the K-streaming kernel at K = 128, plain token grid."""
    from transformerupscaler_amd import ops
    c = G.all_cases()[f"unembed-rt128-{ids(G.HW_RT)}"]()
    o, exp = c.operands, c.expected(torch.float64)
    x, w, skip = o["x"].to(dev), _unembed_w(o["w"], dev), _map(o["skip"], dev)
    _eq(ops.rt_patch_unembed(x, w, o["b"].to(dev), skip), exp["map"], "rt_patch_unembed")
    _eq(ops.rt_patch_embed_bwd(x, w, skip), exp["nobias"], "rt_patch_embed_bwd")


@pytest.mark.parametrize("K", [128, 192])
@pytest.mark.parametrize("hw", G.HW_MULT8, ids=ids)
def test_wt_patch_unembed(dev, hw, K):
    """ops.wt_patch_unembed: the K-streaming kernel with the unembed epilogue in window layout, two and three K steps."""
    from transformerupscaler_amd import ops
    c = G.all_cases()[f"unembed-wt{K}-{ids(hw)}"]()
    o = c.operands
    got = ops.wt_patch_unembed(o["x"].to(dev), _unembed_w(o["w"], dev), o["b"].to(dev), _map(o["skip"], dev))
    _eq(got, c.expected(torch.float64)["map"], f"wt_patch_unembed K={K} {hw}")
