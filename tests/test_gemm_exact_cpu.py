"""Exact-operand tests of the token GEMMs, the part that runs without a GPU: every reference tests/test_hip_gemm_exact.py compares
csrc/gemm_tokens.hip with is itself exact (integer-valued, below 2**24, operands that survive the cast to bf16), and every bf16
output really is rounded: between 5 % and 95 % of its reference magnitudes exceed 256, where bf16 no longer holds every integer
(tests/_gemm_exact_ref.py states the argument)."""
import pytest
import torch

import _exact_ref as R          # tests/ is on sys.path (rootdir-less test modules)
import _gemm_exact_ref as G

CASES = G.all_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_exact_and_bf16_outputs_round(name):
    case = CASES[name]()
    refs = case.refs(torch.float64)
    for key, t in case.operands.items():
        assert torch.equal(t.to(torch.bfloat16).float(), t) and float(t.abs().max()) <= G.AMP, f"{name}: operand {key}"
    for key, ref in refs.items():
        assert ref.dtype == torch.float64
        R.assert_exact_preconditions(ref, bf16_out=key in case.bf16, default_case=False)
        if key in case.bf16:
            share = R.share_above_256(ref)
            assert 0.05 <= share <= 0.95, f"{name}/{key}: {share:.3f} of the outputs exceed 256"
            assert not torch.equal(R.bf16_round(ref), ref), f"{name}/{key}: no value is changed by the rounding"
    assert case.bf16 <= set(refs)


def test_padded_tokens_are_zero_rows_in_the_embed_references():
    """Window-layout rows without a token are exact zeros (no bias); the cases have such rows, and rows with a token are not zero."""
    for name in ("embed-ft192-20x28", "embed-ftb192-64x72", "embed-wt128-20x28"):
        case = CASES[name]()
        kind = name.split("-")[1].rstrip("0123456789")
        hw = tuple(int(v) for v in name.split("-")[2].split("x"))
        valid = G.valid_rows(*G.token_grid(kind, hw))
        tok = case.refs(torch.float64)["tokens"]
        assert 0 < int(valid.sum()) < valid.numel() == tok.shape[0]
        assert bool((tok[~valid] == 0).all()) and bool((tok[valid].abs().sum(1) > 0).all())


def test_case_table_covers_every_path():
    names = set(CASES)
    assert {f"linear-{G._sid(sh)}" for sh in G.LINEAR_SHAPES + G.BIG_SHAPES} <= names
    assert [sh[0] >= 4096 for sh in G.BIG_SHAPES] == [True, False] and all(sh[1] == 192 and sh[2] > 192 for sh in G.BIG_SHAPES)
    assert {"embed-ft192-20x28", "embed-ft192-64x72", "embed-ftb192-20x28", "embed-ftb192-64x72", "embed-rt128-16x24",
            "embed-wt192-20x28", "embed-wt128-20x28", "embed-wt64-20x28"} <= names
    assert {"unembed-ft192-20x28", "unembed-ft192-64x72", "unembed-ftb192-20x28", "unembed-ftb192-64x72", "unembed-merge192-24x40",
            "unembed-merge192-64x72", "unembed-rt128-16x24", "unembed-wt128-24x40", "unembed-wt192-64x72"} <= names
    # (64, 72): 8 x 9 tokens = 1 x 2 windows, the second one token wide
    assert G.window_rows(8, 9) == G.B * 2 * 64 and int(G.valid_rows(8, 9).sum()) == G.B * 72
