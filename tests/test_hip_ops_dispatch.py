"""Which C entry a wrapper of ops.py launches: the reduction wrappers take the atomic entry with ops.deterministic off and its *_det
twin, with a slab and otherwise the same scalar arguments, with it on; LayerNorm and the window attention pick their entries from
the row width / head count of their operands.  (A wrapper that always took the deterministic entry would pass every numeric test
and only cost speed.)  Smallest shapes the kernels take: 128 token rows, maps of 1 x 16 x 32."""
import pytest
import torch

from transformerupscaler_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
M = 128          # two windows
B, H, W = 1, 16, 32


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


@pytest.fixture
def calls(monkeypatch):
    """[(entry name, arguments)] of every _lib.call from here on; the calls still go through."""
    rec, real = [], _lib.call

    def spy(name, *args):
        rec.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    return rec


def _rand(*shape, dtype=F32, seed=0):
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    return torch.randn(shape, generator=g, device=DEV).to(dtype)


def _scalars(name, args):
    return [a for a, t in zip(args, _lib.SIGNATURES[name]) if t is not _lib.P]


def _nulls(name, args):
    return [a is None or a == 0 for a, t in zip(args, _lib.SIGNATURES[name]) if t is _lib.P]


# ---- the twelve reduction wrappers: id -> (operands -> outputs, the atomic entries one call launches) ----
def _gemm(fn, N, dtype):
    p, q = _rand(M, N, dtype=dtype, seed=1), _rand(M, N, dtype=BF16, seed=2)
    return lambda: fn(p, q)


def _patch(reflect):
    p, fmap = _rand(64, 192, seed=3), _rand(B, H, W, 64, dtype=BF16, seed=4)          # 2 x 4 tokens: one window
    return lambda: ops.patch_wgrad(p, fmap, reflect)


def _colsum(N, dtype, masked):
    g = _rand(M, N, dtype=dtype, seed=5)
    mask = (torch.arange(M, device=DEV) % 3 != 0).to(torch.uint8) if masked else None
    return lambda: ops.colsum(g, rowmask=mask)


def _layernorm_bwd(D, drop):
    x, gy, gres = _rand(M, D, seed=6), _rand(M, D, dtype=BF16, seed=7), _rand(M, D, seed=8)
    gamma = _rand(D, seed=9)
    mean, rstd = x.mean(1).contiguous(), (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    return lambda: ops.layernorm_bwd(gy, x, mean, rstd, gamma, gres=gres, drop=(0.1, 77) if drop else None)


def _rt_patch():
    p, fmap = _rand(B * (H // 8) * (W // 8), 128, seed=10), _rand(B, H, W, 64, dtype=BF16, seed=11)
    return lambda: ops.rt_patch_wgrad(p, fmap)


def _wt_patch():
    p, fmap = _rand(64, 128, seed=12), _rand(B, H, W, 64, dtype=BF16, seed=13)
    return lambda: ops.wt_patch_wgrad(p, fmap)


def _c64(gr):
    x, gmap = _rand(B, H, W, 64, dtype=BF16, seed=14), _rand(B, H * gr, W * gr, 64, dtype=BF16, seed=15)
    return lambda: ops.conv_c64_wgrad(x, gmap, gr)


def _c64_s2d():
    x, gmap = _rand(B, 2 * H, 2 * W, 64, dtype=BF16, seed=16), _rand(B, H, W, 64, dtype=BF16, seed=17)
    return lambda: ops.conv_c64_wgrad_s2d(x, gmap, 2)


def _thin(want_bias):
    x, gpl = _rand(B, H, W, 64, dtype=BF16, seed=18), _rand(B, 3, H, W, seed=19)
    return lambda: ops.conv_thin_wgrad(x, gpl, want_bias)


def _planar(r):
    x, gpl = _rand(B, 3, H, W, seed=20), _rand(B, 3, H * r, W * r, seed=21)
    return lambda: ops.conv_planar_wgrad(x, gpl, r)


_NAME = {BF16: "bf16", F32: "fp32"}
REDUCTIONS = {
    **{f"gemm_wgrad {N} {_NAME[dt]}": (lambda N=N, dt=dt: _gemm(ops.gemm_wgrad, N, dt), ["tup_gemm_wgrad"])
       for N in (192, 128) for dt in (BF16, F32)},
    **{f"gemm_wgrad_bias {N} {_NAME[dt]}": (lambda N=N, dt=dt: _gemm(ops.gemm_wgrad_bias, N, dt), ["tup_gemm_wgrad_bias"])
       for N in (192, 128) for dt in (BF16, F32)},
    **{f"colsum {N} {_NAME[dt]}{' masked' if masked else ''}": (lambda N=N, dt=dt, masked=masked: _colsum(N, dt, masked), ["tup_colsum"])
       for N, masked in ((192, True), (128, False)) for dt in (BF16, F32)},
    "patch_wgrad wide": (lambda: _patch(True), ["tup_patch_wgrad_bf16"]),
    "patch_wgrad wide no reflect": (lambda: _patch(False), ["tup_patch_wgrad_bf16"]),
    "patch_wgrad narrow": (lambda: _patch(True), ["tup_patch_wgrad"]),
    "layernorm_bwd 192": (lambda: _layernorm_bwd(192, False), ["tup_layernorm_bwd"]),
    "layernorm_bwd 192 dropout": (lambda: _layernorm_bwd(192, True), ["tup_layernorm_bwd"]),
    "layernorm_bwd 128": (lambda: _layernorm_bwd(128, False), ["tup_layernorm128_bwd"]),
    "layernorm_bwd 128 dropout": (lambda: _layernorm_bwd(128, True), ["tup_layernorm128_bwd"]),
    "rt_patch_wgrad": (_rt_patch, ["tup_rt_patch_wgrad"]),
    "wt_patch_wgrad": (_wt_patch, ["tup_wt_patch_wgrad"]),
    "conv_c64_wgrad gr 1": (lambda: _c64(1), ["tup_conv3x3_c64_wgrad"]),
    "conv_c64_wgrad gr 2": (lambda: _c64(2), ["tup_conv3x3_c64_wgrad"] * 4),
    "conv_c64_wgrad_s2d xr 2": (_c64_s2d, ["tup_conv3x3_c64_wgrad_s2d"] * 4),
    "conv_thin_wgrad": (lambda: _thin(True), ["tup_conv3x3_thin_wgrad"]),
    "conv_thin_wgrad no bias": (lambda: _thin(False), ["tup_conv3x3_thin_wgrad"]),
    "conv_planar_wgrad r 1": (lambda: _planar(1), ["tup_conv3x3_planar_wgrad"]),
    "conv_planar_wgrad r 2": (lambda: _planar(2), ["tup_conv3x3_planar_wgrad"]),
}
# tup_gemm_wgrad has no twin of its own name: the bias twin with a null bias pointer
DET_OF = {"tup_gemm_wgrad": "tup_gemm_wgrad_bias_det"}


def _tensors(out):
    return [t for t in (out if isinstance(out, tuple) else (out,)) if t is not None]


@pytest.mark.parametrize("case", list(REDUCTIONS))
def test_reduction_wrapper_takes_the_atomic_entry_or_its_twin(case, calls, monkeypatch):
    make, atomic = REDUCTIONS[case]
    monkeypatch.setattr(ops, "PATCH_WGRAD_WIDE", "narrow" not in case)
    run = make()
    assert not calls          # building the operands launches nothing of the library's

    assert not ops.deterministic_enabled()
    off = _tensors(run())
    off_calls = list(calls)
    assert [n for n, _ in off_calls] == atomic

    del calls[:]
    with ops.deterministic_mode():
        on = _tensors(run())
        on_calls = list(calls)
        again = _tensors(run())
    assert [n for n, _ in on_calls] == [DET_OF.get(n, n + "_det") for n in atomic]
    for (an, aa), (dn, da) in zip(off_calls, on_calls):
        assert _lib.SIGNATURES[dn][-2] is _lib.P and da[-2], (dn, "slab pointer")
        assert _scalars(dn, da) == _scalars(an, aa), (dn, _scalars(dn, da), _scalars(an, aa))
        if an + "_det" == dn:          # the same pointers are null; the slab sits in front of the stream
            nulls = _nulls(an, aa)
            assert _nulls(dn, da) == nulls[:-1] + [False] + nulls[-1:], dn
    assert len(on) == len(off) == len(again)
    for a, b, c in zip(on, again, off):
        assert a.shape == c.shape and a.dtype == c.dtype
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- one wrapper per operation: the entry follows the operand ----
ENTRIES = {
    (192, 12): dict(ln="tup_layernorm_fwd", ln_bwd="tup_layernorm_bwd", expand="tup_relpos_bias_expand",
                    expand_n="tup_relpos_bias_expand_n", attn="tup_window_attn_fwd", attn_bwd="tup_window_attn_bwd",
                    reduce="tup_relpos_bias_reduce", heads=[]),
    (128, 8): dict(ln="tup_layernorm128_fwd", ln_bwd="tup_layernorm128_bwd", expand="tup_relpos_bias_expand_h",
                   expand_n="tup_relpos_bias_expand_n_h", attn="tup_window_attn_fwd_h", attn_bwd="tup_window_attn_bwd_h",
                   reduce="tup_relpos_bias_reduce_h", heads=[8]),
}


def _block_operands(D, heads):
    x, gamma, beta = _rand(64, D, seed=30), _rand(D, seed=31), _rand(D, seed=32)
    table = _rand(225, heads, seed=33)
    qkv = _rand(64, 48 * heads, dtype=BF16, seed=34)          # one window
    gout = _rand(64, 16 * heads, dtype=BF16, seed=35)
    return x, gamma, beta, table, qkv, gout


@pytest.mark.parametrize("D,heads", list(ENTRIES))
def test_width_and_head_count_pick_the_entry(D, heads, calls):
    e = ENTRIES[(D, heads)]
    x, gamma, beta, table, qkv, gout = _block_operands(D, heads)

    def launched():
        got = [(n, _scalars(n, a)) for n, a in calls]
        del calls[:]
        return got
    y, mean, rstd = ops.layernorm(x, gamma, beta, save_stats=True)
    assert launched() == [(e["ln"], [64])] and tuple(y.shape) == (64, D)
    dx, dg, db = ops.layernorm_bwd(y, x, mean, rstd, gamma)
    assert launched() == [(e["ln_bwd"], [64, 0.0, 0])] and tuple(dx.shape) == (64, D) and tuple(dg.shape) == tuple(db.shape) == (D,)
    frag, frag_n = ops.relpos_bias_expand(table), ops.relpos_bias_expand_n(table)
    assert launched() == [(e["expand"], e["heads"]), (e["expand_n"], e["heads"])]
    assert tuple(frag.shape) == tuple(frag_n.shape) == (heads, 4, 4, 64, 4)
    att, lse = ops.window_attn(qkv, frag, 0.1, 5, save_lse=True)
    assert launched() == [(e["attn"], [1] + e["heads"] + [0.1, 5])]
    assert tuple(att.shape) == (64, 16 * heads) and tuple(lse.shape) == (1, heads, 64)
    gqkv, dtable = ops.window_attn_bwd(qkv, gout, att, lse, frag_n, 0.1, 5)
    assert launched() == [(e["attn_bwd"], [1] + e["heads"] + [0.1, 5]), (e["reduce"], e["heads"])]
    assert tuple(gqkv.shape) == (64, 48 * heads) and tuple(dtable.shape) == (225, heads)
    for t in (y, dx, dg, db, frag, frag_n, att, lse, gqkv, dtable):
        assert torch.isfinite(t.float()).all()


def test_another_width_or_head_count_is_refused_before_any_launch(calls):
    x, gamma, beta, table, qkv, gout = _block_operands(64, 5)
    stats = torch.zeros(64, device=DEV)
    frag = torch.zeros((5, 4, 4, 64, 4), device=DEV)
    att, lse = torch.zeros((64, 80), dtype=BF16, device=DEV), torch.zeros((1, 5, 64), device=DEV)
    for refused in (lambda: ops.layernorm(x, gamma, beta),
                    lambda: ops.layernorm_bwd(x.to(BF16), x, stats, stats, gamma),
                    lambda: ops.relpos_bias_expand(table),
                    lambda: ops.relpos_bias_expand_n(table),
                    lambda: ops.window_attn(qkv, frag),
                    lambda: ops.window_attn_bwd(qkv, gout, att, lse, frag)):
        with pytest.raises(ValueError):
            refused()
        assert not calls
