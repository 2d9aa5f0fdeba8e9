"""frag_set membership of the link-matrix row partition as one bit per fragment (csrc/hhx_matrix.hip: SrcDirectedPacked, the bitmap a
workgroup keeps in LDS beside its tile; csrc/hhx_partition.h: LDS_TABLE), through Ingest.push_device -> finalize -> link_matrix(in_set),
against oracle.dict_to_matrix bit for bit: n_linked, frag_index, indptr, indices, data.

  word seams      33, 64, 65 and 700 fragments (700: both radix levels) x seven sets: every fragment in; every f % 32 == 0 out; every
                  f % 32 == 31 out; only the last fragment out; only the last fragment and one of its partners in; no member at all
                  (the partition ends with n_valid == 0); a seeded random half
  several tiles   700 fragments, 60k pairs: 20k flank keys among 52k keys, fifteen scatter tiles of 7168 directed entries, under
                  HHX_PART_GRID = 1 and 2 (seven tiles a workgroup at least): the table lies behind the staging arrays and has to
                  outlive the staging of every tile of the workgroup
  fallback / cap  the same stream with HHX_D2M_LDS_FRAGS=0 (bitmap words gathered from global memory); at 700 fragments a cap of 700
                  (LDS) against a cap of 699 (global): equal to the oracle and to each other
  same handle     two link_matrix calls on one finalized ingest with two different sets: nothing of the first call is kept

Only the knob is new: the build with byte gathers that this replaced ignores HHX_D2M_LDS_FRAGS and passes every case too.
The streams come from a seed; the oracle's tables are computed once per stream."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_link_build_paths import _Stream, _check_matrix, _ingest, _random_pairs

SIZES = {33: 6_000, 64: 10_001, 65: 12_003, 700: 40_000}            # fragments -> pairs
SETS = ('all_in', 'mod32_0_out', 'mod32_31_out', 'last_out', 'last_and_partner', 'none', 'random_half')
SCATTER_TILE = 7_168                                                # directed entries of a first-level scatter tile (8-byte entries, 512 threads)


@functools.lru_cache(maxsize=None)
def _stream(n):
    return _Stream(n, _random_pairs(np.random.default_rng(100 + n), n, SIZES[n]), 20 + n)


@functools.lru_cache(maxsize=None)
def _long_stream():
    """700 fragments, 60k pairs: more than 15k flank keys among 50k keys, i.e. fourteen scatter tiles of directed entries"""
    return _Stream(700, _random_pairs(np.random.default_rng(99), 700, 60_000), 19)


def _partner_of_last(s):
    """a fragment that shares a flank key with fragment n - 1"""
    fi, fj = s.ref['flank_i'], s.ref['flank_j']
    other = np.concatenate([fj[fi == s.n - 1], fi[fj == s.n - 1]])
    assert len(other), 'fragment %d has no flank key' % (s.n - 1)
    return int(other.min())


def _set(s, which):
    n = s.n
    f = np.arange(n)
    if which == 'all_in':
        return np.ones(n, np.uint8)
    if which == 'mod32_0_out':
        return (f % 32 != 0).astype(np.uint8)
    if which == 'mod32_31_out':
        return (f % 32 != 31).astype(np.uint8)
    if which == 'last_out':
        return (f != n - 1).astype(np.uint8)
    if which == 'last_and_partner':
        m = np.zeros(n, np.uint8)
        m[[n - 1, _partner_of_last(s)]] = 1
        return m
    if which == 'none':
        return np.zeros(n, np.uint8)
    if which == 'random_half':
        return (np.random.default_rng(7 * n).random(n) < 0.5).astype(np.uint8)
    raise KeyError(which)


def _matrix(ing, in_set):
    """what link_matrix returns for this set, as host arrays"""
    m, fidx, n_linked = ing.link_matrix(np.ascontiguousarray(in_set, np.uint8), -1, add_self_loops=True)
    try:
        return (n_linked, fidx.copy()) + tuple(a.copy() for a in m.to_arrays())
    finally:
        m.free()


def _same(a, b, what):
    assert a[0] == b[0], what + ': n_linked'
    for x, y, name in zip(a[1:], b[1:], ('frag_index', 'indptr', 'indices', 'data')):
        assert np.array_equal(x, y), '%s: %s' % (what, name)


@pytest.mark.parametrize('which', SETS)
@pytest.mark.parametrize('n', sorted(SIZES))
def test_word_seams(n, which):
    assert 'HHX_D2M_LDS_FRAGS' not in os.environ and 'HHX_D2M_WIDE' not in os.environ and 'HHX_D2M_GENERIC' not in os.environ
    s = _stream(n)
    in_set = _set(s, which)
    assert (n > 512) == (n == 700)
    ing = _ingest(s)
    try:
        n_rest, n_linked = _check_matrix(ing, s.ref, n, in_set, '%d fragments, %s' % (n, which))
        if which == 'none':
            assert (n_rest, n_linked) == (0, 0)
        elif which == 'last_and_partner':
            assert (n_rest, n_linked) == (0, 2)
        else:
            assert n_linked > 0
    finally:
        ing.destroy()


@pytest.mark.parametrize('grid', [1, 2])
def test_table_outlives_every_tile_of_a_workgroup(grid, monkeypatch):
    s = _long_stream()
    assert len(s.ref['flank_i']) >= 15_000
    assert 2 * len(s.ref['full_i']) >= 4 * grid * SCATTER_TILE, 'a workgroup has fewer than four scatter tiles'
    monkeypatch.setenv('HHX_PART_GRID', str(grid))
    ing = _ingest(s)
    try:
        for which in ('random_half', 'mod32_31_out'):
            _check_matrix(ing, s.ref, s.n, _set(s, which), '700 fragments, %s, HHX_PART_GRID=%d' % (which, grid))
    finally:
        ing.destroy()


@pytest.mark.parametrize('grid', [0, 1])
def test_fallback_gathers_the_words_from_global_memory(grid, monkeypatch):
    s = _long_stream()
    if grid:
        monkeypatch.setenv('HHX_PART_GRID', str(grid))
    ing = _ingest(s)
    try:
        for which in ('random_half', 'last_out', 'none'):
            in_set = _set(s, which)
            monkeypatch.delenv('HHX_D2M_LDS_FRAGS', raising=False)
            in_lds = _matrix(ing, in_set)
            monkeypatch.setenv('HHX_D2M_LDS_FRAGS', '0')
            what = '700 fragments, %s, HHX_D2M_LDS_FRAGS=0, HHX_PART_GRID=%s' % (which, grid or 'default')
            _check_matrix(ing, s.ref, s.n, in_set, what)
            _same(_matrix(ing, in_set), in_lds, what + ' against the LDS table')
    finally:
        ing.destroy()


def test_cap_at_the_fragment_count(monkeypatch):
    s = _stream(700)
    in_set = _set(s, 'random_half')
    ing = _ingest(s)
    try:
        got = {}
        for cap in (700, 699):
            monkeypatch.setenv('HHX_D2M_LDS_FRAGS', str(cap))
            _check_matrix(ing, s.ref, s.n, in_set, '700 fragments, HHX_D2M_LDS_FRAGS=%d' % cap)
            got[cap] = _matrix(ing, in_set)
        _same(got[700], got[699], 'a cap of 700 (LDS) against 699 (global)')
    finally:
        ing.destroy()


@pytest.mark.parametrize('n', [65, 700])
def test_two_sets_on_one_handle(n):
    s = _stream(n)
    ing = _ingest(s)
    try:
        first, second = _set(s, 'mod32_0_out'), _set(s, 'random_half')
        assert not np.array_equal(first, second)
        for which in ('mod32_0_out', 'random_half', 'none', 'all_in', 'mod32_0_out'):
            _check_matrix(ing, s.ref, n, _set(s, which), '%d fragments, %s after another set on the same handle' % (n, which))
    finally:
        ing.destroy()
