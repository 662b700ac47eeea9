"""What the walk table of tests/wino_walks.py covers, proven without a GPU: the restated geometry and grid against the shipped
library's plan queries, and the walk forms every (family, mode) of the table reaches.

* every case is planned on the family it declares, on the grid the restatement gives, and the restated walk runs every item
  of the launch exactly once;
* per (family, mode): blocks that walk three items and blocks that walk fewer than others, XCD lists of different lengths,
  consecutive items of a block in different cout blocks, a ragged last image group, items of the family's minimum chunk count;
* the strided data gradient: a block keeps its dx phase over its whole walk in EVERY launch of the shipped library -- the walk
  stride is 32 whenever a block has a second item and the phase is the item number mod 4 -- so "the next item has another
  output phase" is a form the host never launches; what changes there is the cout block (by two of three);
* the one-item-per-block sub-launches the GPU test compares with: at most one item per block, whole image groups, the whole
  launch covered, and on F(4x4,3x3) the item width of the whole launch (a restatement of Wino44::n32);
* the five launches of tests/test_wino_gpu.py that run "several items per CU" walk exactly one item per block.
"""
import ctypes
import os

import pytest

import wino_walks as WW
from contrad_amd import _lib, ops


@pytest.fixture(scope='module')
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _desc(case, N=None):
    P, mode, N0, H, W, C, K, k, s, p = case[:10]
    ldx, ldy, ldw = WW.lds(case)
    return ops.make_desc(N0 if N is None else N, H, W, C, K, k, k, s, p, ldx, ldy, ldw)


GROUPS = sorted({c[:2] for c in WW.WALK_CASES})


def _of(group):
    return [c for c in WW.WALK_CASES if c[:2] == group]


def test_the_table_has_every_family_and_mode():
    assert GROUPS == [(7, 0), (7, 1), (8, 0), (8, 1), (9, 0), (9, 1), (10, 0), (11, 0), (11, 1)]
    assert len(WW.WALK_CASES) == 29 and len({WW.case_id(c) for c in WW.WALK_CASES}) == 29


@pytest.mark.parametrize('case', WW.WALK_CASES, ids=WW.case_id)
def test_the_library_plans_the_case_as_restated(L, case):
    P, mode = case[:2]
    d = _desc(case)
    g = WW.geometry(case)
    assert L.raw('contrad_conv2d_path')(ctypes.byref(d), mode) == P
    assert WW.family(case) == P                                   # (the restated width rule agrees with the planner)
    grid = WW.grid(g.NP, g.NSUB)
    assert L.raw('contrad_conv2d_grid_blocks')(ctypes.byref(d), mode, 1) == grid == 256
    blocks = WW.walk(g.NP, g.NSUB, grid)
    items = [it for (_, _, its) in blocks for it in its]
    assert len(items) == g.NP * g.NSUB > 256
    assert sorted(items) == [(tb, s) for tb in range(g.NP) for s in range(g.NSUB)]      # every item exactly once
    assert g.chunks == WW.MIN_CHUNKS[(P, mode)]
    assert max(len(its) for (_, _, its) in blocks) >= 2
    assert all(4 + ch == ld for ch, ld in zip((case[5], case[6], case[6]), WW.lds(case)))


@pytest.mark.parametrize('group', GROUPS, ids=lambda g: 'p%d-m%d' % g)
def test_the_walk_forms_of_a_family(group):
    three = fewer = lists = cout_changes = ragged = same_cout = False
    for case in _of(group):
        g = WW.geometry(case)
        blocks = WW.walk(g.NP, g.NSUB, WW.grid(g.NP, g.NSUB))
        lens = {len(its) for (_, _, its) in blocks}
        three |= max(lens) >= 3
        fewer |= len(lens) >= 2
        lists |= len(set(WW.xcd_lists(g.NP, g.NSUB))) >= 2
        ragged |= case[2] % g.NIMG != 0
        for (_, _, its) in blocks:
            for (_, s0), (_, s1) in zip(its, its[1:]):
                (kb0, ph0), (kb1, ph1) = WW.sub_item(case, s0), WW.sub_item(case, s1)
                cout_changes |= kb0 != kb1
                same_cout |= kb0 == kb1
                assert ph0 == ph1          # (see the module docstring: the dx phase of a block never changes)
    assert three and fewer and lists and cout_changes and ragged, (group, three, fewer, lists, cout_changes, ragged)
    if group in ((7, 0), (9, 0)):          # (the two ragged walks with a constant cout block)
        assert same_cout


def test_the_ragged_constant_cout_walks_are_what_they_say():
    a, b = WW.WALK_CASES[-2:]
    for case, items, lens in ((a, 384, {1, 2}), (b, 766, {2, 3})):
        g = WW.geometry(case)
        assert g.NP * g.NSUB == items and g.NSUB == 2
        blocks = WW.walk(g.NP, g.NSUB, 256)
        assert {len(its) for (_, _, its) in blocks} == lens
        assert all(len({s for (_, s) in its}) == 1 for (_, _, its) in blocks)


def test_no_launch_of_the_strided_data_gradient_changes_a_blocks_phase():
    """Every (tile blocks, cout blocks) the host can launch: a block with a second item has the full grid's stride of 32, and
    the dx phase is the item number mod 4."""
    for NTB in range(1, 400):
        for NKB in (1, 2, 3, 4, 5, 8):
            grid = WW.grid(NTB, 4 * NKB)
            if WW.cdiv(NTB, 8) * 4 * NKB > 32:
                assert grid == 256
            for (_, _, its) in WW.walk(NTB, 4 * NKB, grid)[:64]:
                assert len({s & 3 for (_, s) in its}) <= 1


@pytest.mark.parametrize('case', WW.WALK_CASES, ids=WW.case_id)
def test_the_sub_launches_walk_one_item_per_block(case):
    P, N = case[0], case[2]
    g = WW.geometry(case)
    cuts = WW.sub_launches(case)
    assert cuts[0][0] == 0 and cuts[-1][1] == N and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    assert len(cuts) <= 8
    for a, b in cuts:
        assert a % g.NIMG == 0 and (b % g.NIMG == 0 or b == N)
        s = WW.geometry(case, b - a)
        assert (s.NIMG, s.ppi, s.NSUB, s.chunks) == (g.NIMG, g.ppi, g.NSUB, g.chunks)
        assert WW.family(case, b - a) == P
        assert WW.cdiv(s.NP, 8) * s.NSUB <= 32
        assert all(len(its) <= 1 for (_, _, its) in WW.walk(s.NP, s.NSUB, WW.grid(s.NP, s.NSUB)))
    if P == 9:            # (Wino44::n32 keeps 64-wide items at >= 230 of them, and below 115)
        K = case[6] if case[1] == 0 else case[5]
        for a, b in cuts:
            items64 = WW.geometry(case, b - a).NP * (K // 64)
            assert items64 >= 230 or items64 < 115, (a, b, items64)


def test_the_width_rule_restated(L):
    """Wino44::n32 on the 64-wide item counts around its window (16 x 16 maps, 128 couts: two cout blocks, NP = N / 2), and
    against the planner wherever it takes F(4x4,3x3): path 11 exactly where the restatement says 32-wide."""
    seen = set()
    for case in (WW.WALK_CASES[-2], WW.WALK_CASES[6], WW.WALK_CASES[8]):
        for N in range(1, 2 * case[2]):
            P = L.raw('contrad_conv2d_path')(ctypes.byref(_desc(case, N)), 0)
            if P in (9, 11):
                assert WW.family(case, N) == P, (WW.case_id(case), N, P)
                seen.add(P)
    assert seen == {9, 11}
    assert [WW.n32(128, 16, n) for n in (57, 58, 64, 114, 115, 128, 182, 183, 192)] == \
        [False, True, True, True, False, False, True, False, False]
    assert WW.n32(96, 16, 500) and WW.n32(64, 4, 500) and not WW.n32(192, 8, 187) and not WW.n32(192, 8, 27)


def test_the_permutation_moves_every_whole_group():
    for case in WW.WALK_CASES:
        g = WW.geometry(case)
        order = WW.group_permutation(case)
        N, full = case[2], case[2] // g.NIMG
        assert sorted(order) == list(range(N))
        assert order[full * g.NIMG:] == list(range(full * g.NIMG, N))
        assert order[:g.NIMG] == list(range((full - 1) * g.NIMG, full * g.NIMG))
        moved = sum(order[i] != i for i in range(N))
        assert moved >= (full - 1) * g.NIMG        # (every whole group but the middle one of an odd count moves)


@pytest.mark.parametrize('case', WW.SINGLE_ITEM_CASES, ids=WW.case_id)
def test_the_small_launches_of_the_forced_entry_tests_walk_one_item_per_block(L, case):
    """tests/test_wino_gpu.py: 40 (70) images give these launches more items than a tile block has, never two per block."""
    P, mode = case[:2]
    d = _desc(case)
    ok = L.raw('contrad_conv2d_wino44_ok' if P in (9, 11) else 'contrad_conv2d_wino_ok')(ctypes.byref(d), mode)
    assert ok == 1 and WW.family(case) == P
    g = WW.geometry(case)
    grid = WW.grid(g.NP, g.NSUB)
    blocks = WW.walk(g.NP, g.NSUB, grid)
    assert 1 < g.NP * g.NSUB <= 40 and grid <= 8 * 12
    assert max(len(its) for (_, _, its) in blocks) == 1
    assert sum(len(its) for (_, _, its) in blocks) == g.NP * g.NSUB
