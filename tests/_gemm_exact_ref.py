"""Exact-operand references for the token GEMMs of csrc/gemm_tokens.hip (tests/test_gemm_exact_cpu.py,
tests/test_hip_gemm_exact.py).  No tests here.

Same argument as tests/_exact_ref.py: every entry of that file is a GEMM with gather / scatter addressing and an epilogue that
adds integers.  With integers of amplitude 7 in A, the weights, the bias, the residual, the skip maps and pos, every product and
partial sum is an integer of magnitude at most K * 49 + 21 <= 4096 * 49 + 21 < 2**24: the fp32 result is exact in any summation
order, an addressing error changes some output by at least 1, and a bf16 output is the round-to-nearest-even of an exact value
(common.h's pack_bf16x2).  Unlike the conv cases, the bf16 outputs here are MEANT to exceed 256 (K >= 64 products of variance
~ 21**2): test_gemm_exact_cpu.py asserts that between 5 % and 95 % of them do, so the rounding really happens.

The GELU epilogues are not exact and stay in the tolerance tests of tests/test_hip_kernels.py."""
import torch
import torch.nn.functional as F

import _exact_ref as R
from oracle import fast_transformer_oracle as O          # window_partition / window_reverse: the reference's own layout

AMP = 7
ints = R.ints

# (M, N, K) of ops.gemm_tokens and the kernel each takes
LINEAR_SHAPES = [
    (133, 128, 192),        # panel kernel: one full 128-row tile + five rows (row clamp, m >= M skip), two weight tiles (both LDS buffers)
    (133, 128, 64),         # K-streaming kernel, one K step: no pipeline
    (133, 128, 128),        # K-streaming kernel, two K steps
]
BIG_SHAPES = [
    (4133, 192, 256),       # the 256-row big tile: 17 workgroups, the last with 37 rows
    (4095, 192, 256),       # one row below the dispatch edge M >= 4096: the K-streaming kernel
]
B = 2


def _sid(shape):
    return "x".join(str(v) for v in shape)


def to_windows(tok):
    """[B][ht][wt][C] token grid -> window layout [B * nWy * nWx * 64][C], the grid zero-padded to whole 8 x 8 windows."""
    ht, wt = tok.shape[1:3]
    tok = F.pad(tok.permute(0, 3, 1, 2), (0, -wt % 8, 0, -ht % 8)).permute(0, 2, 3, 1).contiguous()
    return O.window_partition(tok, 8).reshape(-1, tok.shape[-1])


def from_windows(x, ht, wt):
    """window layout [B * nWy * nWx * 64][C] -> [B][C][ht][wt]; rows of padded tokens are dropped."""
    hp, wp = (ht + 7) // 8 * 8, (wt + 7) // 8 * 8
    return O.window_reverse(x.view(B, -1, 64, x.shape[-1]), 8, hp, wp)[:, :ht, :wt, :].permute(0, 3, 1, 2)


def window_rows(ht, wt):
    return B * ((ht + 7) // 8) * ((wt + 7) // 8) * 64


def valid_rows(ht, wt):
    """bool [M]: the rows of the window layout that hold a token of the ht x wt grid."""
    return to_windows(torch.ones(B, ht, wt, 1)).view(-1) > 0


def linear_case(shape, want=("bf16", "nobias", "res")):
    """ops.gemm_tokens: 'bf16' with and without bias (bf16 and fp32 A give the same values), 'res' (fp32)."""
    M, N, K = shape
    s = 9000 + K
    o = {"a": ints((M, K), s, AMP), "w": ints((N, K), s + 1, AMP), "b": ints((N,), s + 2, AMP), "res": ints((M, N), s + 3, AMP)}

    def refs(dtype):
        y = o["a"].to(dtype) @ o["w"].to(dtype).t()
        out = {"bf16": y + o["b"].to(dtype), "nobias": y, "res": y + o["b"].to(dtype) + o["res"].to(dtype)}
        return {k: v for k, v in out.items() if k in want}
    return R.Case(f"linear-{_sid(shape)}", o, refs, bf16=tuple(k for k in ("bf16", "nobias") if k in want), rounding=True)


def embed_case(kind, hw, N=192):
    """The patch_embed family: tokens fp32 = patches(map) @ W^T (+ bias) (+ pos), K = 4096.  kind:
    'ft'  ops.patch_embed: reflect padding to multiples of 8, window layout (padded tokens are zero rows);
    'ftb' ops.patch_unembed_bwd: zeros beyond the map, no bias, window layout;
    'rt'  ops.rt_patch_embed (+ bias + pos) and ops.rt_patch_unembed_bwd (neither): plain token grid, N = 128;
    'wt'  ops.wt_patch_embed: the remainder rows / columns are dropped, window layout, N given."""
    H, W = hw
    s = 9100 + N + {"ft": 0, "ftb": 1, "rt": 2, "wt": 3}[kind]
    o = {"map": ints((B, 64, H, W), s, AMP), "w": ints((N, 64, 8, 8), s + 1, AMP), "b": ints((N,), s + 2, AMP)}
    if kind == "rt":
        o["pos"] = ints(((H // 8) * (W // 8), N), s + 3, AMP)

    def refs(dtype):
        m, w, b = o["map"].to(dtype), o["w"].to(dtype), o["b"].to(dtype)
        ph, pw = -H % 8, -W % 8
        if kind == "ft":
            tok = F.conv2d(F.pad(m, (0, pw, 0, ph), mode="reflect") if (ph or pw) else m, w, b, stride=8)
            return {"tokens": to_windows(tok.permute(0, 2, 3, 1))}
        if kind == "ftb":
            return {"tokens": to_windows(F.conv2d(F.pad(m, (0, pw, 0, ph)), w, None, stride=8).permute(0, 2, 3, 1))}
        if kind == "wt":
            return {"tokens": to_windows(F.conv2d(m, w, b, stride=8).permute(0, 2, 3, 1))}
        plain = F.conv2d(m, w, None, stride=8).permute(0, 2, 3, 1)
        return {"tokens": (plain + b + o["pos"].to(dtype).view(1, H // 8, W // 8, N)).reshape(-1, N), "nobias": plain.reshape(-1, N)}
    return R.Case(f"embed-{kind}{N}-{_sid(hw)}", o, refs)


def token_grid(kind, hw):
    H, W = hw
    return ((H + 7) // 8, (W + 7) // 8) if kind in ("ft", "ftb") else (H // 8, W // 8)


def unembed_case(kind, hw, K=192):
    """The patch_unembed family: bf16 NHWC map = scatter(x @ W^T) (+ bias) (+ skip), N = 4096.  kind:
    'ft'    ops.patch_unembed (fp32 and bf16 tokens give the same values): window layout, the map cropped to H x W, + bias + skip;
    'ftb'   ops.patch_embed_bwd: the padded map, no bias, no skip;
    'merge' ops.patch_embed_bwd_merge: (x W^T + add1 [+ add2]) * (relu_src > 0) and the column sums of add1; H, W multiples of 8;
    'rt'    ops.rt_patch_unembed (+ bias + skip) and ops.rt_patch_embed_bwd (+ add): plain token grid;
    'wt'    ops.wt_patch_unembed: window layout, H, W multiples of 8.
    The window-layout rows of padded tokens hold non-zero values too: the kernels must not let them reach the map."""
    H, W = hw
    ht, wt = (H + 7) // 8, (W + 7) // 8
    s = 9200 + K + {"ft": 0, "ftb": 1, "merge": 2, "rt": 3, "wt": 4}[kind]
    M = B * ht * wt if kind == "rt" else window_rows(ht, wt)
    o = {"x": ints((M, K), s, AMP), "w": ints((K, 64, 8, 8), s + 1, AMP), "b": ints((64,), s + 2, AMP), "skip": ints((B, 64, H, W), s + 3, AMP)}
    if kind == "merge":
        o["add2"] = ints((B, 64, H, W), s + 4, AMP)
        o["relu_src"] = ints((B, 64, H, W), s + 5, 1, 0.66)          # +1, 0 and -1, a third each

    def refs(dtype):
        x, w, b, skip = (o[k].to(dtype) for k in ("x", "w", "b", "skip"))
        t = x.view(B, ht, wt, K).permute(0, 3, 1, 2) if kind == "rt" else from_windows(x, ht, wt)
        y = F.conv_transpose2d(t, w, None, stride=8)                # [B][64][ht*8][wt*8]
        if kind == "ftb":
            return {"map": R.nhwc(y)}
        y = y[:, :, :H, :W]
        if kind == "merge":
            gate = o["relu_src"] > 0
            return {"one": R.nhwc((y + skip) * gate), "two": R.nhwc((y + skip + o["add2"].to(dtype)) * gate), "colsum": skip.sum((0, 2, 3))}
        out = {"map": R.nhwc(y + b.view(1, 64, 1, 1) + skip)}
        if kind == "rt":
            out["nobias"] = R.nhwc(y + skip)
        return out
    bf16 = {"merge": ("one", "two"), "rt": ("map", "nobias")}.get(kind, ("map",))
    return R.Case(f"unembed-{kind}{K}-{_sid(hw)}", o, refs, bf16=bf16, rounding=True)


HW_ODD = [(20, 28), (64, 72)]          # reflect / zero padding both ways and one window; 1 x 2 windows, the second one token wide
HW_MULT8 = [(24, 40), (64, 72)]        # the same where H, W must be multiples of 8
HW_RT = (16, 24)


def all_cases():
    """name (= Case.id) -> builder of every case tests/test_hip_gemm_exact.py runs."""
    t = {}
    for sh in LINEAR_SHAPES:
        t[f"linear-{_sid(sh)}"] = lambda sh=sh: linear_case(sh)
    for sh in BIG_SHAPES:
        t[f"linear-{_sid(sh)}"] = lambda sh=sh: linear_case(sh, want=("bf16", "res"))
    for hw in HW_ODD:
        t[f"embed-ft192-{_sid(hw)}"] = lambda hw=hw: embed_case("ft", hw)
        t[f"embed-ftb192-{_sid(hw)}"] = lambda hw=hw: embed_case("ftb", hw)
        t[f"unembed-ft192-{_sid(hw)}"] = lambda hw=hw: unembed_case("ft", hw)
        t[f"unembed-ftb192-{_sid(hw)}"] = lambda hw=hw: unembed_case("ftb", hw)
    for hw in HW_MULT8:
        t[f"unembed-merge192-{_sid(hw)}"] = lambda hw=hw: unembed_case("merge", hw)
        for K in (128, 192):
            t[f"unembed-wt{K}-{_sid(hw)}"] = lambda hw=hw, K=K: unembed_case("wt", hw, K)
    t[f"embed-rt128-{_sid(HW_RT)}"] = lambda: embed_case("rt", HW_RT, 128)
    t[f"unembed-rt128-{_sid(HW_RT)}"] = lambda: unembed_case("rt", HW_RT, 128)
    for N in (192, 128, 64):          # N = 64 is the only small route into gemm_tokens_kernel<A_PATCH, E_PATCH_EMBED>
        t[f"embed-wt{N}-{_sid(HW_ODD[0])}"] = lambda N=N: embed_case("wt", HW_ODD[0], N)
    return t
