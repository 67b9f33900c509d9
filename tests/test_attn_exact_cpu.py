"""Exact-operand tests of the attention kernels, the part that runs without a GPU: conditions on the INPUTS of
tests/test_hip_attn_exact.py, checked with the fp64 reference alone (tests/_attn_exact_ref.py states the argument).

For every case: the operands survive bf16, every logit is the row maximum or at least 128 below it, the number of maximal logits
is 1, 2, 4 or 64 (softmax values in {0, 1/64, 1/4, 1/2, 1}), the exp-free reference equals the plain fp64 softmax, every
expectation survives float32, and every dS of a gradient case has at most 8 significant bits.  Coverage: over the table walk
every one of the 225 x heads entries is the selected one exactly once and every (query, key) pair of the 4096 is the attended
one; over the key walk every key below N is a target once.  Sensitivity, per family: the expectation recomputed under a defect
(index table transposed, one index row off by one, one key dropped, the key tail unmasked, one key split dropped) differs from
the true one by at least 1 (gradients: by at least the smallest non-zero |expected|)."""
import pytest
import torch

import _attn_exact_ref as A          # tests/ is on sys.path (rootdir-less test modules)

BF16 = torch.bfloat16
SOFTMAX_VALUES = {1.0, 2.0, 4.0, 64.0}          # counts of maximal logits


def _check_case(c, counts, softmax_too=True):
    for name in ("q", "k", "v", "gout"):
        t = getattr(c, name)
        if t is not None:
            assert torch.equal(t.to(BF16).float(), t), f"{c.id}: {name} is not exact in bf16"
    assert float(c.v.abs().max()) <= 7 and float(c.q.abs().max()) <= A.QAMP and float(c.k.abs().max()) <= A.KAMP and (c.table is None or set(c.table.unique().tolist()) <= {0.0, A.NEG})
    e = c.expected()
    assert e["gap"] >= A.GAP, f"{c.id}: a logit lies {e['gap']} below its row maximum"
    got = set(e["cnt"].unique().tolist())
    assert got <= SOFTMAX_VALUES and got == set(counts), f"{c.id}: rows with {sorted(got)} maximal logits, expected {sorted(counts)}"
    assert set(e["mx"].unique().tolist()) <= {A.NEG, 0.0, 256.0}          # -256: a window row without the selected offset
    keys = ["out", "lse"] + (["gqkv"] if c.gout is not None else []) + (["dtable", "dtable_abs"] if "dtable" in e else [])
    for key in keys:
        t = e[key].double()
        assert bool(torch.isfinite(t).all())
        if key != "lse":                          # lse = mx + ln(count) is the one expectation that is not a dyadic rational
            assert torch.equal(t.float().double(), t), f"{c.id}: {key} does not survive float32"
    if c.gout is not None:
        assert e["dS_bits"] <= 8, f"{c.id}: a dS has {e['dS_bits']} significant bits"
        assert float(e["gqkv"].abs().max()) > 0 or c.n == 1
    if softmax_too:                               # the exp-free form against the plain fp64 softmax, and fp32 against fp64
        assert (c.raw(exact=False)["out"] - c.raw()["out"]).abs().max().item() <= 1e-30, c.id
        e32 = c.expected(torch.float32)
        for key in keys:
            if key != "lse":
                assert torch.equal(e32[key].double(), c.expected(torch.float64)[key]), f"{c.id}: {key} in fp32"
    return e


# ------------------------------------------------------------------------------------------------
# window cases
# ------------------------------------------------------------------------------------------------
def _expected_counts(name):
    if name.startswith("tie2"):
        return {1, 2, 64}
    if name.startswith("tie4"):
        return {1, 2, 4, 64}
    if name.startswith("qk"):
        return {int(name[2])}
    return {1}                                    # combined


@pytest.mark.parametrize("heads", [12, 8])
def test_window_forward_cases_are_exact(heads):
    for nwin in A.NWIN_FWD:
        for name, build in A.window_forward_cases(heads, nwin).items():
            counts = _expected_counts(name)
            c = build()
            e = _check_case(c, counts, softmax_too=nwin == 3)
            if name.startswith("qk") or name == "combined":           # every query attends exactly to its direction's targets
                P = c.raw()["P"]
                for w in range(nwin):
                    for h in range(heads):
                        for i in (0, 17, 63):
                            keys = set(P[w, h, i].nonzero().flatten().tolist())
                            want = set(c.note["targets"][w][h][int(c.note["dmap"][w, h, i])])
                            assert keys <= want and (keys == want or name == "combined") and keys, (c.id, w, h, i)
            assert e["out"].shape == (nwin * 64, 16 * heads)


@pytest.mark.parametrize("heads", [12, 8])
def test_window_backward_cases_are_exact(heads):
    for nwin in A.NWIN_BWD:
        for name, build in A.window_backward_cases(heads, nwin).items():
            c = build()
            e = _check_case(c, {2} if name == "combined" else _expected_counts(name), softmax_too=nwin == 1)
            assert float(e["dtable_abs"].max()) > 0, c.id
            if "tie" in name:                 # the selected offsets, and no other entry, get a gradient
                sel = torch.zeros((225, heads), dtype=torch.bool)
                for h, offs in enumerate(c.note["offsets"]):
                    sel[offs, h] = True
                assert not bool(e["dtable_abs"][~sel].any()), c.id


@pytest.mark.parametrize("heads", [12, 8])
def test_window_gradient_walk_reaches_every_offset(heads):
    """the ceil(225 / heads) tie tables: every offset is the first of a selected group in some head, and gets a gradient there"""
    for m in (2, 4):
        first = torch.zeros(225, dtype=torch.long)
        hit = torch.zeros(225, dtype=torch.bool)
        for t in range(A.tie_tables(heads)):
            c = A.window_table_case(1, heads, A.tie_offsets(heads, t, m), "walk", backward=True)
            for h, offs in enumerate(c.note["offsets"]):
                first[offs[0]] += 1
            hit |= (c.expected()["dtable_abs"] > 0).any(1)
        assert int(first.min()) >= 1 and bool(hit.all())


@pytest.mark.parametrize("heads", [12, 8])
def test_window_table_walk_covers_every_entry_and_every_pair(heads):
    selected = torch.zeros((225, heads), dtype=torch.long)
    pairs = torch.zeros((heads, 64, 64), dtype=torch.bool)
    for t in range(A.WALK):
        c = A.window_table_case(5, heads, A.walk_offsets(heads, t), f"win-h{heads}-walk{t}")
        e = _check_case(c, {1, 64} if any(o[0] != 112 for o in c.note["offsets"]) else {1}, softmax_too=t % 45 == 0)
        for nwin in (1, 3) if t % 45 == 0 else ():          # the smaller launches run the first windows of the same tensors (whatever t)
            small = A.window_table_case(nwin, heads, A.walk_offsets(heads, t), c.id)
            assert torch.equal(small.qkv(), c.qkv()[:nwin * 64]) and torch.equal(small.table, c.table)
        selected += (c.table == 0).long()
        r = c.raw()
        P, cnt = r["P"], e["cnt"]
        pairs |= ((P[0] > 0) & (cnt[0] == 1).unsqueeze(-1))
        one = cnt == 1                            # a one-hot row is a row of v, bit for bit
        j = P.argmax(-1)
        rows = torch.gather(c.v.double(), 2, j.unsqueeze(-1).expand(-1, -1, -1, 16))
        assert torch.equal(A.pack_heads(torch.where(one.unsqueeze(-1), rows, r["out"])), e["out"])
    assert bool((selected == 1).all()), "every table entry is the selected one exactly once"
    assert bool(pairs.all()), "every (query, key) pair is the attended one in some table, in every head"


def _moves(a, b, least=1.0):
    return (a.double() - b.double()).abs().max().item() >= least


def _least(t):
    t = t.abs()
    return t[t > 0].min().item()


@pytest.mark.parametrize("heads", [12, 8])
def test_window_families_see_the_defects(heads):
    rel_t = A.REL.t().contiguous()
    rel_1 = A.REL.clone()
    fams = {"walk": A.window_table_case(3, heads, A.walk_offsets(heads, 3), "walk"),
            "tie2": A.window_table_case(3, heads, A.tie_offsets(heads, 5, 2), "tie2"),
            "tie4": A.window_table_case(3, heads, A.tie_offsets(heads, 5, 4), "tie4"),
            "qk1": A.window_qk_case(3, heads, 1, 0, "qk1"), "qk2": A.window_qk_case(3, heads, 2, 0, "qk2"),
            "qk4": A.window_qk_case(3, heads, 4, 0, "qk4"), "combined": A.window_combined_case(3, heads, "combined")}
    for name, c in fams.items():
        true = c.raw()
        i0 = int((true["cnt"][0, 0] < 64).nonzero()[0])             # a query of (window 0, head 0) that selects
        j0 = int(true["P"][0, 0, i0].argmax())
        keep = torch.ones(64, dtype=torch.bool)
        keep[j0] = False
        assert _moves(c.raw(exact=False, keep=keep)["out"], true["out"]), f"{name}: one key dropped"
        if not name.startswith("qk"):
            rel_1 = A.REL.clone()
            rel_1[i0] = (rel_1[i0] + 1) % 225
            assert _moves(c.raw(exact=False, rel=rel_t)["out"], true["out"]), f"{name}: index table transposed"
            assert _moves(c.raw(exact=False, rel=rel_1)["out"], true["out"]), f"{name}: one index row off by one"
    grads = {"tie2": A.window_table_case(3, heads, A.tie_offsets(heads, 5, 2), "tie2", backward=True),
             "tie4": A.window_table_case(3, heads, A.tie_offsets(heads, 5, 4), "tie4", backward=True),
             "qk2": A.window_qk_case(3, heads, 2, 1, "qk2", backward=True),
             "combined": A.window_combined_case(3, heads, "combined", backward=True)}
    for name, c in grads.items():
        true = c.raw()
        tie = (true["cnt"][0, 0] > 1) & (true["cnt"][0, 0] < 64)
        i0 = int(tie.nonzero()[0])
        j0 = int(true["P"][0, 0, i0].argmax())
        keep = torch.ones(64, dtype=torch.bool)
        keep[j0] = False
        rel_1 = A.REL.clone()
        rel_1[i0] = (rel_1[i0] + 1) % 225
        defects = {"one key dropped": dict(keep=keep)}
        if not name.startswith("qk"):
            defects.update({"index table transposed": dict(rel=rel_t), "one index row off by one": dict(rel=rel_1)})
        for what, kw in defects.items():
            bad = c.raw(exact=False, **kw)
            assert any(_moves(bad[key], true[key], _least(true[key])) for key in ("dq", "dk", "dv") if float(true[key].abs().max()) > 0), \
                f"{name} gradients: {what}"


# ------------------------------------------------------------------------------------------------
# ResidualTransformer cases
# ------------------------------------------------------------------------------------------------
def _attended(c):
    """[B][8][N] -> the set of keys each query attends to must equal the targets of its direction"""
    P = c.raw(torch.float32 if c.n > 1000 else torch.float64, heads=slice(0, 1))["P"] if c.n > 1000 else c.raw()["P"]
    for b in range(P.shape[0]):
        for h in range(P.shape[1]):
            for i in sorted({0, c.n // 2, c.n - 1}):
                keys = set(P[b, h, i].nonzero().flatten().tolist())
                assert keys == set(c.note["targets"][b][h][int(c.note["dmap"][b, h, i])]), (c.id, b, h, i)


@pytest.mark.parametrize("B,N", A.RT_SHAPES)
def test_rt_forward_cases_are_exact(B, N):
    cases = A.rt_forward_cases(B, N)
    assert "place" in cases and (N > 257 or len([n for n in cases if n.startswith("walk")]) == (N + 127) // 128)
    seen = torch.zeros(N, dtype=torch.long)
    for name, build in cases.items():
        c = build()
        _check_case(c, {int(name[3])} if name.startswith("tie") else {1}, softmax_too=N <= 257)
        _attended(c)
        tg = c.note["targets"]
        if name.startswith("walk"):
            fresh = {(128 * int(name[4:]) + 16 * h + d) for h in range(8) for d in range(16)}
            for key in fresh:
                if key < N:
                    seen[key] += 1
                    assert [key] in [tg[0][h][d] for h in range(8) for d in range(16)]
        if name == "place":
            keys = {k for d in tg[0][0] for k in d}
            tail = 64 * ((N - 1) // 64)
            want = [k for k in (0, 15, 16, 63, 64, tail - 1, tail, N - 1) if 0 <= k < N]
            assert len(A.rt_placement_keys(N)) <= 16 and all(set(want) <= {k for d in tg[b][h] for k in d} for b in range(B) for h in range(8)) \
                or N < 16, (N, want)
            if N >= 193:
                assert all({A.rt_split(k) for d in tg[0][h] for k in d} == {0, 1, 2, 3} for h in range(8))
            if N > 256:                     # a target in tile 4 .. 7 = some wave's SECOND key tile; its first holds only losers of that direction
                for h in range(8):
                    late = [(d, k) for d in range(16) for k in tg[0][h][d] if 4 <= k // 64 < 8]
                    assert late
                    for d, k in late:
                        first = slice(64 * (k // 64 - 4), 64 * (k // 64 - 4) + 64)
                        assert float(c.k[0, h, first, d].max()) == 0.0
            if N == 3600:
                assert {0, 63, 64, 3583, 3584, 3599} <= keys and sum(len(d) for h in range(8) for d in tg[0][h]) == 128
        if name.startswith("tie"):
            m, tiles = int(name[3]), (N + 63) // 64
            assert any(N - 1 in d for d in tg[0][0])
            for h in range(8):
                assert any(tg[0][h]), "a head without a direction"
                for d in tg[0][h]:
                    if d and tiles >= m:
                        assert len({A.rt_split(k) for k in d}) == m, (c.id, h, d)
    if N <= 257:
        assert bool((seen == 1).all()), "every key is a target of the walk exactly once"


@pytest.mark.parametrize("B,N", A.RT_BWD_SHAPES)
def test_rt_backward_cases_are_exact(B, N):
    cases = A.rt_backward_cases(B, N)
    assert set(cases) == ({f"tie{m}" for m in A.rt_tie_orders(N)} or {"place"})
    for name, build in cases.items():
        c = build()
        e = _check_case(c, {int(name[3])} if name.startswith("tie") else {1}, softmax_too=N <= 257)
        if N > 1:
            q, k, v = e["gqkv"].view(B * N, 3, 8, 16).unbind(1)
            assert min(float(t.abs().max()) for t in (q, k, v)) > 0, f"{c.id}: dq, dk and dv must all be exercised"


@pytest.mark.parametrize("N", [17, 65, 257, 3600])
def test_rt_families_see_the_defects(N):
    tiles = (N + 63) // 64
    dt = torch.float32 if N > 1000 else torch.float64
    hs = dict(heads=slice(0, 1))                  # head 0 holds key N - 1 as a tie target
    fams = {"place": A.rt_placement_case(1, N), "tie2": A.rt_tie_case(1, N, 2)}
    if N <= 257:
        fams["walk"] = A.rt_walk_case(1, N, A.rt_walk_launches(N) - 1)
    if N >= 193:
        fams["tie4"] = A.rt_tie_case(1, N, 4)
    for name, c in fams.items():
        true = c.raw(dt, **hs)["out"]
        t0 = c.note["targets"][0][0][0][0]
        keep = torch.ones(N, dtype=torch.bool)
        keep[t0] = False
        assert _moves(c.raw(dt, exact=False, keep=keep, **hs)["out"], true), f"{name} N={N}: one key dropped"
        split = (torch.arange(N) // 64) % 4 != A.rt_split(t0)
        if tiles > 1:
            assert _moves(c.raw(dt, exact=False, keep=split, **hs)["out"], true), f"{name} N={N}: one key split dropped"
        if name.startswith("tie"):
            assert _moves(c.raw(dt, exact=False, tail_pad=64 * tiles - N, **hs)["out"], true), f"{name} N={N}: key tail unmasked"
    g = A.rt_tie_case(1, N, 2, backward=True)
    true = g.raw(dt, **hs)
    t0 = g.note["targets"][0][0][0][0]
    keep = torch.ones(N, dtype=torch.bool)
    keep[t0] = False
    defects = {"one key dropped": dict(keep=keep), "key tail unmasked": dict(tail_pad=64 * tiles - N)}
    if tiles > 1:
        defects["one key split dropped"] = dict(keep=(torch.arange(N) // 64) % 4 != A.rt_split(t0))
    for what, kw in defects.items():
        bad = g.raw(dt, exact=False, **kw, **hs)
        assert any(_moves(bad[key][:, :, :N], true[key], _least(true[key])) for key in ("dq", "dk", "dv")), f"tie2 gradients N={N}: {what}"


def test_fragment_layout_readers_invert_the_kernels_index_maps():
    """frag_fwd_to_dense / frag_n_to_dense restate the layouts written above relpos_expand_kernel and relpos_expand_n_kernel:
    build the fragments from those sentences with explicit loops and read them back."""
    dense = torch.arange(2 * 4096).view(2, 64, 64)
    fwd, n = torch.zeros(2, 4, 4, 64, 4, dtype=torch.long), torch.zeros(2, 4, 4, 64, 4, dtype=torch.long)
    for a in range(4):
        for b in range(4):
            for lane in range(64):
                for e in range(4):
                    fwd[:, a, b, lane, e] = dense[:, 16 * b + (lane & 15), 16 * a + 4 * (lane >> 4) + e]      # [kt = a][qt = b]
                    n[:, a, b, lane, e] = dense[:, 16 * a + 4 * (lane >> 4) + e, 16 * b + (lane & 15)]        # [qt = a][kt = b]
    assert torch.equal(A.frag_fwd_to_dense(fwd), dense) and torch.equal(A.frag_n_to_dense(n), dense)
    rel = A.REL
    assert int(rel[0, 63]) == 0 and int(rel[63, 0]) == 224 and int(rel[7, 56]) == 14 and int(rel[56, 7]) == 210 and int(rel[5, 5]) == 112
    assert sorted(torch.bincount(rel.flatten(), minlength=225).tolist())[0] == 1         # the four corners: one pair each


def test_block_selector_tables():
    offs = [[(A.BLOCK_OFFSETS[i] + 19 * h) % 225 for h in range(12)] for i in range(len(A.BLOCK_OFFSETS))]
    assert len(A.BLOCK_OFFSETS) == 20 and {0, 14, 210, 224, 112} <= set(A.BLOCK_OFFSETS)
    for i in range(20):
        t = A.block_table(i)
        assert int((t == 0).sum()) == 12 and all(t[offs[i][h], h] == 0 for h in range(12))
