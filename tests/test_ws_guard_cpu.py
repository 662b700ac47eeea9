"""The workspace harness (tests/ws_guard.py) on CPU tensors, no kernel launched: a guard that cannot fail is no guard.  And the
coverage table of tests/test_workspace_contract_gpu.py: every ``contrad_*_workspace_bytes`` prototype that contrad_amd/_lib.py
parses from include/contrad_hip.h names the contract cases that exercise it, so a new query without a case fails here (the
pattern of tests/kernel_ledger.py for kernel instances)."""
import pytest
import torch

from contrad_amd import _lib, ops
from ws_guard import BACK_BYTES, FRONT_BYTES, POISONS, GuardError, WorkspaceGuard

import test_workspace_contract_gpu as W

CPU = torch.device('cpu')


def some_wrapper(nbytes):
    """Stands for an ``ops`` wrapper: looks ``_workspace`` up by name at call time."""
    return ops._workspace(nbytes, CPU)


def _helper(nbytes):
    return ops._workspace(nbytes, CPU)


def wrapper_over_a_helper(nbytes):
    return _helper(nbytes)


def _i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


@pytest.mark.parametrize('poison', sorted(POISONS))
@pytest.mark.parametrize('nbytes', [0, 1, 3, 4, 100, 4096, 70001])
def test_view_has_the_promised_size_alignment_and_poison(poison, nbytes):
    word = POISONS[poison]
    with WorkspaceGuard(word) as g:
        ws = some_wrapper(nbytes)
        again = some_wrapper(nbytes)
        g.check()
    n4 = (max(nbytes, 1) + 3) // 4 * 4                                  # as ops._workspace rounds
    assert ws.dtype == torch.float32 and ws.dim() == 1 and ws.numel() * 4 == n4
    assert ws.data_ptr() % 16 == 0 and ws.data_ptr() % 32 == 16          # 16 bytes is all the header promises
    assert FRONT_BYTES % 32 == 16
    assert again.data_ptr() != ws.data_ptr()                            # fresh storage per request, nothing cached
    r = g.log[0]
    assert [q.index for q in g.log] == [0, 1] and r.nbytes == nbytes and r.caller == 'some_wrapper'
    assert r.view.data_ptr() == ws.data_ptr()
    assert r.front.data_ptr() + FRONT_BYTES == ws.data_ptr()            # the guards touch the view on both sides
    assert r.back.data_ptr() == ws.data_ptr() + n4 and r.back.numel() * 4 == BACK_BYTES
    for part in (r.front, ws.view(torch.int32), r.back):
        assert bool((part == _i32(word)).all())
    if poison != 'zero':
        assert bool(torch.isnan(ws).all())
    if poison == 'ones' and ws.numel() % 2 == 0:
        assert bool(torch.isnan(ws.view(torch.float64)).all())          # a NaN as a double too, and -1 / the maximum as integers
        assert bool((ws.view(torch.int32) == -1).all())


def test_a_write_just_before_the_view_is_caught_and_named():
    with WorkspaceGuard(POISONS['qnan']) as g:
        some_wrapper(64)
        ws = wrapper_over_a_helper(100)
        some_wrapper(8)
        ws.fill_(1.0)                                                   # the workspace itself is the op's to write
        g.check()
        g.log[1].front[-1] = 0                                          # the four bytes in front of ws[0]
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    assert 'request #1' in msg and '100 bytes' in msg and 'wrapper_over_a_helper' in msg and 'front guard' in msg
    assert 'byte offset -4 ' in msg and 'request #0' not in msg and 'request #2' not in msg


@pytest.mark.parametrize('poison', sorted(POISONS))
def test_a_write_just_after_the_view_is_caught_and_named(poison):
    with WorkspaceGuard(POISONS[poison]) as g:
        some_wrapper(64)
        ws = some_wrapper(101)                                          # 104 bytes after rounding: the guard begins there
        g.check()
        g.log[1].back[0] = 7
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    assert 'request #1' in msg and '101 bytes' in msg and 'some_wrapper' in msg and 'back guard' in msg
    assert 'byte offset 104 ' in msg and '0x00000007' in msg and 'request #0' not in msg
    assert ws.numel() == 26


def test_the_last_word_of_the_back_guard_counts_too():
    with WorkspaceGuard(POISONS['ones']) as g:
        some_wrapper(16)
        g.log[0].back[-1] = 0
        with pytest.raises(GuardError, match='back guard'):
            g.check()


def test_workspace_function_is_restored_after_a_normal_exit():
    before = ops._workspace
    with WorkspaceGuard(POISONS['zero']) as g:
        assert ops._workspace is not before and ops._workspace == g._request
        with WorkspaceGuard(POISONS['ones']) as inner:                  # nests: the inner one logs, then hands back
            some_wrapper(4)
        assert len(inner.log) == 1 and not g.log and ops._workspace == g._request
    assert ops._workspace is before


def test_workspace_function_is_restored_after_an_exception():
    before = ops._workspace
    with pytest.raises(ZeroDivisionError):
        with WorkspaceGuard(POISONS['qnan']):
            some_wrapper(4)
            1 // 0
    assert ops._workspace is before


def test_requests_can_be_filtered_by_wrapper():
    with WorkspaceGuard(POISONS['qnan']) as g:
        some_wrapper(4); wrapper_over_a_helper(8); some_wrapper(12)
    assert [r.nbytes for r in g.requests('some_wrapper')] == [4, 12]
    assert [r.nbytes for r in g.requests('wrapper_over_a_helper')] == [8] and len(g.requests()) == 3


# ======================================================================================================================
# coverage: workspace query -> the contract cases (ids of W.CASE_TABLES) that run a launch sized by it
# ======================================================================================================================
def _all(*families):
    return [i for f in families for i in W.CASE_TABLES[f]]


COVERAGE = {
    'contrad_conv2d_fwd_workspace_bytes': [
        'conv/p2-m0-split-2x1x1x512-64-k1s1p0', 'conv/p2-m0-split-4x8x8x64-96-k3s1p1', 'conv/p2-m0-split-3x17x17x64-64-k3s1p1',
        'conv/p7-m0-5x32x32x16-512-k3s1p1', 'conv/p7-m0-75x8x8x16-512-k3s1p1', 'conv/p8-m0-48x32x32x8-512-k4s2p1',
        'conv/p9-m0-16x32x32x32-512-k3s1p1', 'conv/p9-m0-229x8x8x32-512-k3s1p1', 'conv/p10-m0-192x33x33x16-256-k3s2p0',
        'conv/p11-m0-1536x4x4x32-160-k3s1p1'],
    'contrad_conv2d_dgrad_workspace_bytes': [
        'conv/p2-m1-split-2x1x1x48-512-k1s1p0', 'conv/p2-m1-split-3x17x17x64-64-k3s1p1', 'conv/p7-m1-5x32x32x512-32-k3s1p1',
        'conv/p7-m1-75x8x8x512-16-k3s1p1', 'conv/p8-m1-48x16x16x512-32-k4s2p1', 'conv/p9-m1-16x32x32x512-32-k3s1p1',
        'conv/p11-m1-1536x4x4x160-32-k3s1p1'],
    'contrad_conv2d_wgrad_workspace_bytes': [
        'conv/p0-m2-1x1x1x3-1-k1s1p0', 'conv/p0-m2-split-5x9x9x3-8-k3s1p1', 'conv/p1-m2-1x1x1x8-8-k1s1p0',
        'conv/p1-m2-split-1x9x9x8-8-k1s1p0', 'conv/p2-m2-1x4x4x8-8-k1s1p0', 'conv/p2-m2-split-5x4x4x8-8-k1s1p0',
        'conv/p3-m2-16x2x2x128-8-k3s1p1', 'conv/p3-m2-split-48x2x2x128-8-k3s1p1', 'conv/p4-m2-split-16x64x64x32-32-k3s1p1',
        'conv/p7-m2-split-1x64x64x256-512-k3s1p1', 'conv/p8-m2-split-16x16x16x512-512-k4s2p1'],
    'contrad_conv2d_wino_workspace_bytes': [
        'conv forced/p7-m0-5x32x32x16-512-k3s1p1', 'conv forced/p7-m1-5x32x32x512-32-k3s1p1',
        'conv forced/p7-m2-split-1x64x64x256-512-k3s1p1', 'conv forced/p8-m0-48x32x32x8-512-k4s2p1',
        'conv forced/p8-m1-48x16x16x512-32-k4s2p1', 'conv forced/p8-m2-split-16x16x16x512-512-k4s2p1',
        'conv forced/p10-m0-192x33x33x16-256-k3s2p0', 'conv forced/p7-m0-75x8x8x16-512-k3s1p1',
        'conv forced/p7-m1-75x8x8x512-16-k3s1p1'],
    'contrad_conv2d_wino44_workspace_bytes': [
        'conv forced/p9-m0-16x32x32x32-512-k3s1p1', 'conv forced/p9-m1-16x32x32x512-32-k3s1p1',
        'conv forced/p9-m0-229x8x8x32-512-k3s1p1', 'conv forced/p11-m0-1536x4x4x32-160-k3s1p1',
        'conv forced/p11-m1-1536x4x4x160-32-k3s1p1'],
    'contrad_contrast_workspace_bytes': _all('ntxent'),
    'contrad_rgb_conv_wgrad_workspace_bytes': _all('rgb wgrad'),
    'contrad_colstats_workspace_bytes': _all('colstats', 'bn stats'),
    'contrad_simclr_workspace_bytes': _all('simclr fwd'),
    'contrad_simclr_augment_bwd_workspace_bytes': _all('simclr bwd'),
    'contrad_diffaug_workspace_bytes': _all('diffaug'),
    'contrad_sumsq_workspace_bytes': _all('sumsq'),
    'contrad_nhwc_dot_workspace_bytes': _all('nhwc_dot'),
    'contrad_linhead_workspace_bytes': _all('linhead'),
    'contrad_gp_penalty_workspace_bytes': _all('gp_penalty'),
    'contrad_knn_select_workspace_bytes': _all('knn_select'),
    'contrad_kid_sums_workspace_bytes': _all('sums'),
    'contrad_swd_gather_workspace_bytes': _all('swd gather'),
    'contrad_swd_absdiff_workspace_bytes': _all('swd absdiff'),
}


def header_queries():
    return {name for name in _lib.parse_header() if name.endswith('_workspace_bytes')}


def test_every_workspace_query_of_the_header_has_contract_cases():
    queries = header_queries()
    assert len(queries) >= 19
    missing, stale = sorted(queries - set(COVERAGE)), sorted(set(COVERAGE) - queries)
    assert not missing, 'workspace queries without a contract case in tests/test_workspace_contract_gpu.py: %s' % missing
    assert not stale, 'COVERAGE names queries the header no longer declares: %s' % stale
    assert all(COVERAGE[q] for q in queries)


def test_every_named_case_exists_in_the_gpu_module():
    known = [i for ids in W.CASE_TABLES.values() for i in ids]
    assert len(known) == len(set(known)), 'case ids must be unique'
    for q, ids in COVERAGE.items():
        for i in ids:
            assert i in known, (q, i)
    covered = {i for ids in COVERAGE.values() for i in ids}
    # and the other way round for the families that exist for one query only: no case is left unclaimed
    for fam in W.CASE_TABLES:
        if fam not in ('conv', 'conv forced'):
            assert set(W.CASE_TABLES[fam]) <= covered, fam


def test_every_ops_wrapper_that_asks_for_scratch_sizes_it_by_a_header_query():
    """Each ``_workspace(`` call site in contrad_amd/ops.py sits in a function that names a ``*_workspace_bytes`` query of the
    header (directly or through the private helper that calls it): a wrapper that sized its scratch some other way would be
    outside this contract."""
    import inspect
    import re
    queries = header_queries()
    sites = 0
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if fn.__module__ != ops.__name__ or name == '_workspace':
            continue
        src = inspect.getsource(fn)
        if not re.search(r'(?<![\w.])_workspace\(', src):
            continue
        sites += 1
        named = set(re.findall(r"'(contrad_\w+_workspace_bytes)'", src))
        assert named and named <= queries, (name, named)
    assert sites >= 19
