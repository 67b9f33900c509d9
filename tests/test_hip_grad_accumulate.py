"""`tup_grad_accumulate` (csrc/grad_accumulate.hip) against torch on the MI355X, through `accumulate.SegmentLauncher` -- the staging
and chunk-table code every caller uses.  All comparisons are `torch.equal`: mode 0 is a copy (alpha = 1) or one rounded product,
mode 1 one rounded product and one rounded add (no fused multiply-add), mode 2 zeros; there is nothing to tolerate.  Every segment
lies inside a NaN-guarded arena with sentinel floats between the segments, which must come back untouched."""
import pytest
import torch

from transformerupscaler_amd.accumulate import SegmentLauncher

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 63, 4096, 4097, 64 * 64 * 3 * 3]          # ..., a conv3x3 64 -> 64 weight
GUARD = 64


def _arena(sizes, gen, dst_shift=0):
    """One buffer: GUARD sentinel floats, then per segment its floats (starting `dst_shift` floats off a 64-float boundary) and
    GUARD more sentinels.  Returns (arena, [(offset, n)], expected-untouched mask)."""
    offs, cur = [], GUARD
    for n in sizes:
        cur = (cur + 63) // 64 * 64 + dst_shift
        offs.append((cur, n))
        cur += n + GUARD
    arena = torch.randn((cur,), generator=gen, device=DEV)
    guard = torch.ones((cur,), dtype=torch.bool, device=DEV)
    for o, n in offs:
        guard[o:o + n] = False
    return arena, offs, guard


def _src(n, gen, shift):
    """A source of n floats that starts `shift` floats off its allocation (shift % 4 != 0: not 16-byte aligned)."""
    base = torch.randn((n + 8,), generator=gen, device=DEV)
    return base[shift:shift + n]


@pytest.mark.parametrize("alpha", [1.0, 0.37])
@pytest.mark.parametrize("dst_shift,src_shift", [(0, 0), (0, 1), (0, 3), (1, 0), (2, 2), (0, 4)])
def test_modes_against_torch(alpha, dst_shift, src_shift):
    gen = torch.Generator(device=DEV).manual_seed(100 + 7 * dst_shift + src_shift)
    sizes = SIZES + [4095, 8192 + 5]
    arena, offs, guard = _arena(sizes, gen, dst_shift)
    before = arena.clone()
    srcs = [_src(n, gen, src_shift) for n in sizes]
    if src_shift % 4:
        assert any(s.data_ptr() % 16 for s in srcs)
    modes = [(i * 5 + dst_shift) % 3 for i in range(len(sizes))]          # the three modes mixed inside one launch
    assert set(modes) == {0, 1, 2}
    launcher = SegmentLauncher(torch.device(DEV, torch.cuda.current_device()))
    a32 = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    want = before.clone()
    for (o, n), s, m in zip(offs, srcs, modes):
        if m == 0:
            want[o:o + n] = a32 * s                     # one rounded product (alpha = 1: the value itself)
        elif m == 1:
            prod = a32 * s
            want[o:o + n] = before[o:o + n] + prod      # product rounded, then the add: two fp32 operations
        else:
            want[o:o + n] = 0
    launcher.launch([(arena.data_ptr() + 4 * o, 0 if m == 2 else s.data_ptr(), n, alpha, m) for (o, n), s, m in zip(offs, srcs, modes)])
    torch.cuda.synchronize()
    assert torch.equal(arena[guard], before[guard]), "floats outside the segments were written"
    for (o, n), m in zip(offs, modes):
        assert torch.equal(arena[o:o + n], want[o:o + n]), (n, m, alpha, dst_shift, src_shift)


def test_alpha_one_is_torchs_own_accumulation():
    """grad = g0; grad += g1; grad += g2 by torch, and the same three gradients through modes 0, 1, 1."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    shapes = [(64, 64, 3, 3), (192,), (576, 192), (1,), (225, 6), (3, 64, 3, 3)]
    sizes = [torch.Size(s).numel() for s in shapes]
    arena, offs, guard = _arena(sizes, gen)
    arena.fill_(float("nan"))                           # never zero-filled: the first touch overwrites
    launcher = SegmentLauncher(torch.device(DEV, torch.cuda.current_device()))
    want = [None] * len(shapes)
    for rnd in range(3):
        gs = [torch.randn(s, generator=gen, device=DEV) for s in shapes]
        for i, g in enumerate(gs):
            if want[i] is None:
                want[i] = g.clone()
            else:
                want[i] += g
        launcher.launch([(arena.data_ptr() + 4 * o, g.data_ptr(), n, 1.0, 0 if rnd == 0 else 1) for (o, n), g in zip(offs, gs)])
    torch.cuda.synchronize()
    for (o, n), w, s in zip(offs, want, shapes):
        assert torch.equal(arena[o:o + n].view(s), w)
    assert torch.isnan(arena[guard]).all()


def test_launcher_reuses_its_tables_and_survives_many_launches():
    """The chunk table is cached per set of sizes; the two pinned staging slots are recycled safely when the host runs ahead."""
    gen = torch.Generator(device=DEV).manual_seed(6)
    launcher = SegmentLauncher(torch.device(DEV, torch.cuda.current_device()))
    dst = torch.zeros((3, 5000), device=DEV)
    g = torch.randn((3, 5000), generator=gen, device=DEV)
    want = torch.zeros_like(dst)
    for _ in range(40):
        launcher.launch([(dst[i].data_ptr(), g[i].data_ptr(), 5000, 1.0, 1) for i in range(3)])
        want += g
    torch.cuda.synchronize()
    assert len(launcher._chunks) == 1 and next(iter(launcher._chunks.values())).shape == (6, 2)
    assert torch.equal(dst, want)
    launcher.launch([])                                 # nothing to do: no launch, no error
    launcher.launch([(dst.data_ptr(), 0, 0, 1.0, 2)])   # empty segments are dropped
