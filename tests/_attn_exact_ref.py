"""Exact-operand cases and references for the attention kernels (tests/test_attn_exact_cpu.py, tests/test_hip_attn_exact.py).
No tests here.

The argument.  q, k, v and the output gradient are small integers (|v| <= 7; q is 0 or 16 e_d, k is 0, +-64 e_d or small
integers), exact in bf16.  The bias table holds 0 or -256.  Every logit 0.25 q.k + bias is then an integer multiple of 256 or,
with q = 0, the table entry itself, and the builders make every logit of a row EITHER the row's maximum OR at least 128 below it.
exp of -128 or less is 0 in fp32 (exp(-104) already is), as __expf, as exp2f of the log2-domain score, with denormals flushed or
not; so a kernel's exp is exactly 1 on the maximal logits and exactly 0 elsewhere.  The number m of maximal logits per row is a
power of two (1, 2, 4 or 64): the sum is m, 1 / sum and P = 2^-m' are exact in fp32 and in bf16.  PV is a sum of at most 64
products of a dyadic with an integer of amplitude at most 7: exact in fp32 in any order, and the bf16 output is the
round-to-nearest-even of an exact value.  The online softmax of rt_attention_kernel stays exact too: the running maximum only
takes the values -inf, 0 (or -256) and 256 (in the log2 domain, times one rounded constant: equal logits stay equal), so every
alpha = exp2(m_run - m) and every factor of the merge of the four key splits is exactly 0 or 1.  An addressing, masking,
split-merge or layout defect attends to another key and moves an output by a difference of two integer rows of v.

Backward.  A one-hot row has a zero softmax gradient, so the gradient cases tie 2 or 4 keys: with P_a = P_b = 1/2,
dS_a = (dP_a - dP_b) / 4.  v is within +-2 and the output gradient within +-1 there: |dP| <= 32 and every dS is k / 4 or k / 16
with |k| < 256, at most 8 significant bits, which a rounding to bf16 keeps.  Rows that attend uniformly to all 64 keys (a window
query without the selected offset) get a zero output gradient, hence dS = 0.  dq = 0.25 dS k, dk = 0.25 dS^T q, dv = P^T gout
and dtable = sum of dS over the pairs of an offset are dyadic and exact in fp64 (and in fp32).

The reference (attend) does not call exp at all when exact=True: P = [logit == row max] / count, with the smallest gap to the
maximum returned so that the CPU test can assert it is >= 128; with exact=False it is the plain fp64 softmax, used to show that
both agree and to recompute an expectation under a defect."""
import math

import torch

from _exact_ref import ints

NEG = -256.0
GAP = 128.0
QAMP, KAMP = 16.0, 64.0                  # 0.25 * 16 * 64 = 256


def _rel_index():
    t = torch.arange(64)
    y, x = t // 8, t % 8
    return (y[:, None] - y[None, :] + 7) * 15 + (x[:, None] - x[None, :] + 7)


REL = _rel_index()                       # [query][key] -> row of the [225][heads] table (query - key offsets, + 7 each)


def dense_bias(table, rel=REL):
    """table [225][H] -> [H][64 query][64 key]"""
    return table[rel.reshape(-1)].view(64, 64, -1).permute(2, 0, 1).contiguous()


def frag_fwd_to_dense(frag):
    """relpos_expand_kernel's layout, frag[h][kt][qt][lane][e] = bias(query 16 qt + (lane & 15), key 16 kt + 4 (lane >> 4) + e),
    read back as [h][query][key]."""
    H = frag.shape[0]
    f = frag.reshape(H, 4, 4, 4, 16, 4)                    # h, kt, qt, g, p, e
    return f.permute(0, 2, 4, 1, 3, 5).reshape(H, 64, 64)  # h, (qt, p), (kt, g, e)


def frag_n_to_dense(frag):
    """relpos_expand_n_kernel's layout, frag[h][qt][kt][lane][e] = bias(query 16 qt + 4 (lane >> 4) + e, key 16 kt + (lane & 15))."""
    H = frag.shape[0]
    f = frag.reshape(H, 4, 4, 4, 16, 4)                    # h, qt, kt, g, p, e
    return f.permute(0, 1, 3, 5, 2, 4).reshape(H, 64, 64)  # h, (qt, g, e), (kt, p)


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def attend(q, k, v, bias=None, gout=None, dtype=torch.float64, exact=True, keep=None):
    """q [..., n, 16], k, v [..., nk, 16], bias broadcastable to [..., n, nk], gout like the output, keep: bool [nk] (False =
    the key does not exist).  Returns a dict: out, lse, cnt, mx, gap, P and, with gout, dq, dk, dv, dS."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    L = 0.25 * (q @ k.transpose(-2, -1))
    if bias is not None:
        L = L + bias.to(dtype)
    if keep is not None:
        L = L.masked_fill(~keep, -math.inf)
    mx = L.max(-1, keepdim=True).values
    if exact:
        top = L == mx
        cnt = top.sum(-1, keepdim=True).to(dtype)
        P = top.to(dtype) / cnt
        below = torch.where(top, torch.full_like(L, math.inf), mx - L)
        r = dict(gap=below.min().item(), cnt=cnt.squeeze(-1), lse=(mx + cnt.log()).squeeze(-1))
    else:
        P = torch.softmax(L, -1)
        r = dict(lse=torch.logsumexp(L, -1))
    r.update(P=P, mx=mx.squeeze(-1), out=P @ v)
    if gout is not None:
        g = gout.to(dtype)
        dP = g @ v.transpose(-2, -1)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        r.update(dS=dS, dq=0.25 * (dS @ k), dk=0.25 * (dS.transpose(-2, -1) @ q), dv=P.transpose(-2, -1) @ g)
    return r


def pack_heads(t):
    """[G][H][n][16] -> [G n][16 H]"""
    G, H, n, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(G * n, 16 * H)


def pack_qkv(q, k, v):
    """three [G][H][n][16] -> [G n][48 H], (q | k | v) each head-major: the kernels' token rows"""
    G, H, n, _ = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(G * n, 48 * H)


class AttnCase:
    """q, k, v: fp32 integers [G][H][n][16] (G = windows, or images of n tokens); table: fp32 [225][H] or None (no bias); gout:
    fp32 integers [G][H][n][16] or None; targets: what the case makes each query attend to, for the coverage assertions."""

    def __init__(self, ident, q, k, v, table=None, gout=None, note=None):
        self.id, self.q, self.k, self.v, self.table, self.gout, self.note = ident, q, k, v, table, gout, note or {}
        self.G, self.H, self.n = q.shape[:3]

    def qkv(self):
        return pack_qkv(self.q, self.k, self.v)

    def gout_rows(self):
        return pack_heads(self.gout)

    def raw(self, dtype=torch.float64, exact=True, rel=REL, keep=None, heads=None, tail_pad=0):
        """attend() on the case's operands; rel: the index table a defect may replace; heads: a subset (the large cases go head by
        head); tail_pad: that many keys beyond n, holding the last key's row (what the kernels' min(row, n - 1) loads fetch)."""
        hs = slice(None) if heads is None else heads
        q, k, v = self.q[:, hs], self.k[:, hs], self.v[:, hs]
        if tail_pad:
            k = torch.cat([k, k[:, :, -1:].expand(-1, -1, tail_pad, -1)], 2)
            v = torch.cat([v, v[:, :, -1:].expand(-1, -1, tail_pad, -1)], 2)
        bias = None if self.table is None else dense_bias(self.table, rel)[hs]
        gout = None if self.gout is None else self.gout[:, hs]
        return attend(q, k, v, bias, gout, dtype, exact, keep)

    def expected(self, dtype=None, **kw):
        """What the kernels must produce, in their layouts: out [G n][16 H], lse [G][H][n], and with gout gqkv [G n][48 H] and
        dtable [225][H]; plus cnt, mx [G][H][n], the smallest gap, and sum |dS| per table entry.  fp64 unless the case is large
        (3600 tokens, 150 windows): every value is a dyadic rational that fp32 holds, test_attn_exact_cpu.py compares the two."""
        dtype = dtype or (torch.float32 if self.n > 1000 or self.G > 32 else torch.float64)      # large: fp32, equal to fp64 on exact values
        parts = [self.raw(dtype, heads=slice(h, h + 1), **kw) for h in range(self.H)] if self.n > 1000 else [self.raw(dtype, **kw)]
        cat = (lambda key: torch.cat([p[key] for p in parts], 1))
        e = dict(out=pack_heads(cat("out")), lse=cat("lse"), mx=cat("mx"))
        if "cnt" in parts[0]:
            e.update(cnt=cat("cnt"), gap=min(p["gap"] for p in parts))
        if self.gout is not None:
            e["gqkv"] = pack_qkv(cat("dq"), cat("dk"), cat("dv"))
            e["dS_bits"] = max(_sig_bits(p["dS"]) for p in parts)
            if self.table is not None:
                dS = cat("dS")
                e["dtable"] = _reduce_offsets(dS.sum(0))
                e["dtable_abs"] = _reduce_offsets(dS.abs().sum(0))
        return e


def _reduce_offsets(d):
    """[H][64][64] -> [225][H]: the sum over the (query, key) pairs of every offset"""
    H = d.shape[0]
    return torch.zeros((225, H), dtype=d.dtype).index_add_(0, REL.reshape(-1), d.reshape(H, 4096).t())


def _sig_bits(t):
    """the largest number of significant bits of any element (dyadic rationals; 0 for an all-zero tensor)"""
    t = t[t != 0]
    if t.numel() == 0:
        return 0
    m, _ = torch.frexp(t.double().abs())
    for bits in range(1, 54):
        s = m * 2.0 ** bits
        if bool((s == s.round()).all()):
            return bits
    return 54


# ------------------------------------------------------------------------------------------------
# window cases: [nwin][heads][64][16]
# ------------------------------------------------------------------------------------------------
WALK = 225                               # tables of the full walk: head h of table t selects offset (t + 19 h) % 225
NWIN_FWD = (1, 3, 5)
NWIN_BWD = (1, 5, 150)


def selector_table(heads, offsets):
    """[225][heads] of -256 with 0 on offsets[h] (a list of table rows per head)"""
    t = torch.full((225, heads), NEG)
    for h, offs in enumerate(offsets):
        for o in offs:
            t[o, h] = 0.0
    return t


def walk_offsets(heads, t):
    return [[(t + 19 * h) % 225] for h in range(heads)]


def tie_tables(heads):
    return (225 + heads - 1) // heads


def tie_offsets(heads, t, m):
    """2 (a horizontal pair) or 4 (a 2 x 2 block) neighbouring offsets per head; the first is (t heads + h) % 225, so that the
    ceil(225 / heads) tables of a family start at every offset once.  A query has 0, 1, 2 or 4 of them inside its window."""
    out = []
    for h in range(heads):
        dy, dx = divmod((t * heads + h) % 225, 15)
        dx2 = dx + 1 if dx < 14 else dx - 1
        dy2 = dy + 1 if dy < 14 else dy - 1
        offs = [dy * 15 + dx, dy * 15 + dx2]
        if m == 4:
            offs += [dy2 * 15 + dx, dy2 * 15 + dx2]
        out.append(offs)
    return out


def _window_ints(nwin, heads, seed, amp):
    """[nwin][heads][64][16]; up to 5 windows are the first windows of the 5-window tensor (a window never meets another), so the
    CPU conditions shown at 5 windows hold for the 1- and 3-window launches of the same case"""
    return ints((max(nwin, 5), heads, 64, 16), seed, amp)[:nwin].contiguous()


def _window_operands(nwin, heads, seed, amp_v):
    return _window_ints(nwin, heads, seed, 3), _window_ints(nwin, heads, seed + 1, amp_v)


def _mask_uniform_rows(case, gout):
    """zero the output gradient of the rows that attend to all 64 keys (their dS would need more than 8 bits)"""
    cnt = case.raw(torch.float32)["cnt"]
    return gout * (cnt < 64).unsqueeze(-1)


def window_table_case(nwin, heads, offsets, ident, backward=False, seed=100):
    """q = 0: query i attends exactly to the keys at the selected offsets, or to all 64 keys where its window has none."""
    k, v = _window_operands(nwin, heads, seed, 2 if backward else 7)
    c = AttnCase(ident, torch.zeros_like(k), k, v, selector_table(heads, offsets), note=dict(offsets=offsets))
    if backward:
        c.gout = _mask_uniform_rows(c, _window_ints(nwin, heads, seed + 2, 1))
    return c


def _place(nwin, heads, n, targets, seed, amp_v, lose=0.3, low=False):
    """The q.k selector: targets[g][h][d] = list of keys that win direction d (an empty list: no query uses the direction), and
    query i of head h points at a used direction: q_i = 16 e_d(i).  High form: a target holds +64 in its direction and every other
    entry of k is 0 or -64: logits 256, 0, -256.  Low form (the window gradients, whose dtable bound wants a row maximum of 0):
    a target holds 0 and every other key -64 in a used direction, logits 0 and -256; the unused directions of k hold integers
    within +-3, which no logit sees and dq does.  Returns q, k, v, d."""
    shape = (nwin, heads, n, 16)
    g_ = torch.Generator().manual_seed(seed)
    k = -KAMP * (torch.rand(shape, generator=g_) < lose).float()
    free = ints(shape, seed + 7, 3)
    q = torch.zeros(shape)
    dmap = torch.zeros((nwin, heads, n), dtype=torch.long)
    for w in range(nwin):
        for h in range(heads):
            used = [d for d in range(16) if targets[w][h][d]]
            assert used, "a head needs at least one target"
            if low:
                is_used = torch.zeros(16, dtype=torch.bool)
                is_used[used] = True
                k[w, h] = torch.where(is_used, torch.full((), -KAMP), free[w, h])
            pairs = [(key, d) for d in used for key in targets[w][h][d]]
            k[w, h, [p[0] for p in pairs], [p[1] for p in pairs]] = 0.0 if low else KAMP
            dd = torch.tensor([used[(i + 3 * h + w) % len(used)] for i in range(n)])
            dmap[w, h] = dd
            q[w, h, torch.arange(n), dd] = QAMP
    return q, k, ints(shape, seed + 1, amp_v), dmap


def window_qk_case(nwin, heads, m, shift, ident, backward=False, table=None, seed=200):
    """table 0 (or given): direction d of (window w, head h) has m target keys, spread over the 64 keys by `shift`.  The
    gradient form is _place's low one, on 8 directions."""
    targets = [[[[((4 * d + j) * 5 + shift + 5 * h + 3 * w) % 64 for j in range(m)] if d < (8 if backward else 16) else []
                 for d in range(16)] for h in range(heads)] for w in range(nwin)]       # x 5: a bijection of 0 .. 63
    for w in range(nwin):                                  # keys of different directions must differ inside a head
        for h in range(heads):
            flat = [key for d in range(16) for key in targets[w][h][d]]
            assert len(set(flat)) == len(flat), (ident, w, h)
    q, k, v, dmap = _place(nwin, heads, 64, targets, seed + shift, 2 if backward else 7, low=backward)
    c = AttnCase(ident, q, k, v, torch.zeros((225, heads)) if table is None else table, note=dict(targets=targets, dmap=dmap))
    if backward:
        c.gout = ints(k.shape, seed + 2, 1)
    return c


def parity_table(heads):
    """-256 on the offsets whose column (even heads) or row (odd heads) distance d has (d + phase) % 4 >= 2, phase = h // 2: two
    keys two columns (rows) apart never share a value, and the table is not symmetric under query <-> key"""
    t = torch.zeros((225, heads))
    for h in range(heads):
        for o in range(225):
            dy, dx = o // 15 - 7, o % 15 - 7
            if ((dx if h % 2 == 0 else dy) + h // 2) % 4 >= 2:
                t[o, h] = NEG
    return t


def window_combined_case(nwin, heads, ident, backward=False, seed=300):
    """table 0 / -256 as above, plus q.k with two targets per direction two columns (even heads) or two rows (odd heads) apart:
    exactly one of the two has bias 0 for any query, so the bias and q.k must be added at the same (query, key).  A one-hot row
    has no gradient: the backward form uses 8 directions with those two keys in the upper half of the window and their twins four
    rows below, which share their table value: every row ties exactly two keys."""
    targets = []
    for w in range(nwin):
        per_h = []
        for h in range(heads):
            per_d = []
            for d in range(16):
                a = 4 * d + (h + w) % 2                      # columns 0, 1, 4, 5 of a row
                b = a + 2 if h % 2 == 0 else (a ^ 16) + 2    # two columns on, or (also) two rows away: distinct over d
                per_d.append(([a, b, a + 32, b + 32] if d < 8 else []) if backward else [a, b])
            per_h.append(per_d)
        targets.append(per_h)
    q, k, v, dmap = _place(nwin, heads, 64, targets, seed, 2 if backward else 7, low=backward)
    c = AttnCase(ident, q, k, v, parity_table(heads), note=dict(targets=targets, dmap=dmap))
    if backward:
        c.gout = ints(k.shape, seed + 2, 1)
    return c


def window_forward_cases(heads, nwin):
    """name -> builder of every forward case but the 225-table walk (window_table_case(nwin, heads, walk_offsets(heads, t), ..))"""
    t = {}
    for m in (2, 4):
        for i in range(tie_tables(heads)):
            t[f"tie{m}-{i}"] = lambda m=m, i=i: window_table_case(nwin, heads, tie_offsets(heads, i, m), f"win-h{heads}-w{nwin}-tie{m}-{i}")
    for m in (1, 2, 4):
        for shift in (0, 1, 2, 3):
            t[f"qk{m}-{shift}"] = lambda m=m, shift=shift: window_qk_case(nwin, heads, m, shift, f"win-h{heads}-w{nwin}-qk{m}-{shift}")
    t["combined"] = lambda: window_combined_case(nwin, heads, f"win-h{heads}-w{nwin}-combined")
    return t


def window_backward_cases(heads, nwin):
    """The tie families with gradients.  150 windows take one table of each family (the persistent loop, not the map)."""
    t = {}
    last = tie_tables(heads) - 1
    for m in (2, 4):
        for i in (range(last + 1) if nwin <= 5 else (0,) if m == 2 else (last,)):
            t[f"tie{m}-{i}"] = lambda m=m, i=i: window_table_case(nwin, heads, tie_offsets(heads, i, m), f"winbwd-h{heads}-w{nwin}-tie{m}-{i}",
                                                                  backward=True)
        if nwin <= 5 or m == 2:
            t[f"qk{m}"] = lambda m=m: window_qk_case(nwin, heads, m, 1, f"winbwd-h{heads}-w{nwin}-qk{m}", backward=True)
    t["combined"] = lambda: window_combined_case(nwin, heads, f"winbwd-h{heads}-w{nwin}-combined", backward=True)
    return t


# ------------------------------------------------------------------------------------------------
# ResidualTransformer cases: [B][8][N][16]
# ------------------------------------------------------------------------------------------------
RT_N = (1, 15, 17, 63, 64, 65, 129, 193, 257, 3600)
RT_B2 = (17, 65, 257)
RT_BWD_N = (1, 17, 65, 257, 3600)
RT_SHAPES = [(1, n) for n in RT_N] + [(2, n) for n in RT_B2]
RT_BWD_SHAPES = [(1, n) for n in RT_BWD_N]


def rt_split(key):
    """the wave of rt_attention_kernel that takes this key: key tile (key // 64) % 4"""
    return (key // 64) % 4


def rt_placement_keys(N):
    """keys 0, 15, 16, 63, 64, the last full tile's last key, the first and last key of the tail tile, one key in the first tile
    of each of the four waves, and one in each wave's SECOND tile (tiles 4 .. 7: the running maximum jumps from a loser's 0)"""
    tail = 64 * ((N - 1) // 64)
    c = [0, 15, 16, 63, 64, tail, N - 1, tail - 1] + [64 * w + 21 for w in range(4)] + [64 * (4 + w) + 9 for w in range(4)]
    out = []
    for key in c:
        if 0 <= key < N and key not in out:
            out.append(key)
    return out


def _rt_case(ident, B, N, targets, seed, backward):
    q, k, v, dmap = _place(B, 8, N, targets, seed, 2 if backward else 7)
    c = AttnCase(ident, q, k, v, None, note=dict(targets=targets, dmap=dmap))
    if backward:
        c.gout = ints(k.shape, seed + 2, 1)
    return c


def rt_placement_case(B, N, backward=False):
    keys = rt_placement_keys(N)
    nd = min(16, len(keys))
    targets = [[[[keys[(5 * h + d + b) % len(keys)]] if d < nd else [] for d in range(16)] for h in range(8)] for b in range(B)]
    return _rt_case(f"rt-place-{B}x{N}", B, N, targets, 400 + N, backward)


def rt_walk_launches(N):
    return (N + 127) // 128


def rt_walk_case(B, N, launch):
    """key (128 launch + 16 h + d) % N is the target of (head h, direction d): every key below N once over the launches"""
    nd = min(16, N)
    targets = [[[[(128 * launch + 16 * h + d + b) % N] if d < nd else [] for d in range(16)] for h in range(8)] for b in range(B)]
    return _rt_case(f"rt-walk{launch}-{B}x{N}", B, N, targets, 500 + N + launch, False)


def rt_tie_case(B, N, m, backward=False):
    """m targets per direction, each in another key tile (tiles apart by less than 4 are different key splits) where N has that
    many tiles; (head 0, direction 0) takes key N - 1.  A direction whose tile is full goes unused."""
    tiles = (N + 63) // 64
    targets = []
    for b in range(B):
        per_h = []
        for h in range(8):
            taken, per_d = set(), []
            for d in range(16):
                keys = []
                for s in range(m):
                    tile = (tiles - 1 - s if (h + d) % 2 == 0 else s) % tiles
                    lo, hi = 64 * tile, min(64 * tile + 64, N)
                    key = N - 1 if (h == 0 and d == 0 and tile == tiles - 1) else lo + (16 * h + 3 * d + 5 * s + b) % (hi - lo)
                    for _ in range(hi - lo):            # the next free key of the tile; key N - 1 of head 0 stays with direction 0
                        if key not in taken and (key != N - 1 or (h == 0 and d == 0) or h != 0):
                            break
                        key = lo + (key + 1 - lo) % (hi - lo)
                    else:
                        key = None
                    if key is None or key in taken:
                        keys = None
                        break
                    keys.append(key)
                    taken.add(key)
                if keys is None:
                    per_d.append([])
                    continue
                per_d.append(keys)
            per_h.append(per_d)
        targets.append(per_h)
    return _rt_case(f"rt-tie{m}-{B}x{N}", B, N, targets, 600 + N + m, backward)


def rt_tie_orders(N):
    """the tie sizes N has room for: two targets need two keys, four in four key splits need four tiles"""
    return [m for m in (2, 4) if (m == 2 and N >= 2) or (m == 4 and N >= 193)]


def rt_forward_cases(B, N):
    t = {"place": lambda: rt_placement_case(B, N)}
    if N <= 257:
        for l in range(rt_walk_launches(N)):
            t[f"walk{l}"] = lambda l=l: rt_walk_case(B, N, l)
    for m in rt_tie_orders(N):
        t[f"tie{m}"] = lambda m=m: rt_tie_case(B, N, m)
    return t


def rt_backward_cases(B, N):
    t = {f"tie{m}": (lambda m=m: rt_tie_case(B, N, m, backward=True)) for m in rt_tie_orders(N)}
    if not t:
        t["place"] = lambda: rt_placement_case(B, N, backward=True)       # N = 1: one key, P = 1, dq = dk = 0, dv = gout
    return t


# ------------------------------------------------------------------------------------------------
# block kernels: selector tables in place of the random one
# ------------------------------------------------------------------------------------------------
BLOCK_OFFSETS = [0, 14, 210, 224, 112, 7, 105, 119, 217, 1, 15, 16, 97, 111, 113, 127, 56, 168, 60, 200]      # corners, (0, 0) = 112


def block_table(i):
    """[225][12]: head h selects offset (BLOCK_OFFSETS[i] + 19 h) % 225"""
    return selector_table(12, [[(BLOCK_OFFSETS[i] + 19 * h) % 225] for h in range(12)])
