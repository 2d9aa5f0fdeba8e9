"""The write-out of the row emit kernel (csrc/hhx_matrix.hip: k_row_emit) against the oracle, bit for bit: n_linked, frag_index and
the CSR triple of Ingest.link_matrix, at the seams of the staged write-out.

A row's entries are staged in LDS at their rank, HHX_EMIT_STAGE positions a pass at most (unset: what LDS allows, 0: every entry
stored directly), and copied out in runs; HHX_EMIT_GRID caps the workgroups.  The cases:

  pass seams        rows of exactly S, of more than S and of more than 2 S entries, S taken from the row lengths of the reference
                    (the self loop counted in), with and without self loops
  the self loop     in a row where it is the smallest column and in one where it is the largest, on a pass boundary
  beyond registers  the hub row of 4600+ entries (the first EMIT_R * EMIT_T = 4096 are held in registers, the rest read again in every pass), packed
                    and wide entries
  one workgroup     HHX_EMIT_GRID=1 and 2: every row by one workgroup, rows outside frag_set and link-less members in between
  no room to stage  orders that leave no or little LDS beside the bitmap (650k: direct stores; 600k: short passes)
  knobs             two link_matrix calls on one handle under different knob values give the same arrays

Streams, tables and the comparison are those of tests/test_gpu_link_build_paths.py; a library without the knobs passes unchanged
(they only move seams)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_gpu_link_build_paths import _Stream, _stream, _ingest, _check_matrix, _random_pairs, _third_out


def _ref_rows(s, in_set, self_loops):
    """(indptr, indices, n_linked) of the reference matrix of stream s over in_set"""
    ref = s.ref
    in_set = np.ascontiguousarray(in_set, np.uint8)
    ok = in_set[ref['flank_i']].astype(bool) & in_set[ref['flank_j']].astype(bool)
    linked = np.zeros(s.n, bool)
    linked[ref['flank_i'][ok]] = True
    linked[ref['flank_j'][ok]] = True
    n_rest = int(in_set.sum() - linked.sum())
    rp, rj, _rx, _ridx, rl = orc.dict_to_matrix(ref['flank_i'], ref['flank_j'], ref['flank_cnt'].astype(np.float64), s.n, in_set, n_rest,
                                                add_self_loops=self_loops)
    return rp, rj, rl


def _set_knobs(monkeypatch, **knobs):
    for k in ('HHX_EMIT_STAGE', 'HHX_EMIT_GRID', 'HHX_D2M_WIDE'):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


@pytest.mark.parametrize('self_loops', [True, False])
def test_pass_seams(monkeypatch, self_loops):
    s = _stream('two_levels')
    in_set = np.ones(s.n, np.uint8)
    rp, _rj, rl = _ref_rows(s, in_set, self_loops)
    lens = np.diff(rp)[:rl]                                            # the emitted rows, the self loop counted in
    L = int(lens[lens >= 8].min())
    assert L >= 8 and (lens == L).any()
    stages = [L, L - 1, L + 1, (L + 1) // 2, 1, 0]
    for S in stages[:-1]:                                              # every size meets rows of two passes and of three or more,
        assert (lens > S).any() and (lens > 2 * S).any(), (S, int(lens.max()))
        assert (lens % S == 0).any() or S == L - 1, S                   # ... and a row that fills its last pass (S = L: in one pass)
    ing = _ingest(s)
    try:
        for S in stages:
            _set_knobs(monkeypatch, HHX_EMIT_STAGE=S)
            _check_matrix(ing, s.ref, s.n, in_set, 'two_levels, %d positions a pass, self loops %s' % (S, self_loops), self_loops=self_loops)
    finally:
        ing.destroy()


@pytest.mark.parametrize('which', ['all', 'third_out'])
def test_self_loop_first_and_last_of_its_row(monkeypatch, which):
    s = _stream('two_levels')
    in_set = np.ones(s.n, np.uint8) if which == 'all' else _third_out(s.n)
    rp, rj, rl = _ref_rows(s, in_set, True)
    rows = np.arange(rl)
    first = rows[rj[rp[:rl]] == rows]                                  # the row's own index is its smallest column
    last = rows[rj[rp[1:rl + 1] - 1] == rows]                          # ... its largest
    assert len(first) and len(last) and not set(first) & set(last)
    lo, hi = int(first[0]), int(last[-1])
    len_lo, len_hi = int(rp[lo + 1] - rp[lo]), int(rp[hi + 1] - rp[hi])
    assert len_lo > 2 and len_hi > 2
    # rank 0 opens a pass at any size; rank len_hi - 1 closes the only pass (len_hi), is alone in the second (len_hi - 1), closes the
    # second of two ((len_hi + 1) // 2 for an even length, else opens the third of (len_hi - 1) // 2); size 1 puts every entry on a boundary
    ing = _ingest(s)
    try:
        for S in (len_hi, len_hi - 1, (len_hi + 1) // 2, (len_hi - 1) // 2, len_lo, len_lo - 1, 1):
            _set_knobs(monkeypatch, HHX_EMIT_STAGE=S)
            _check_matrix(ing, s.ref, s.n, in_set, 'two_levels, %s, %d positions a pass' % (which, S))
    finally:
        ing.destroy()


def test_rows_beyond_the_registers(monkeypatch):
    s = _stream('hub')
    in_set = np.ones(s.n, np.uint8)
    rp, _rj, rl = _ref_rows(s, in_set, True)
    assert int(np.diff(rp)[:rl].max()) > 4600
    ing = _ingest(s)
    try:
        for knobs in ({}, {'HHX_EMIT_STAGE': 1000}, {'HHX_EMIT_STAGE': 0}, {'HHX_D2M_WIDE': 1}):
            _set_knobs(monkeypatch, **knobs)
            for self_loops in (True, False):
                _check_matrix(ing, s.ref, s.n, in_set, 'hub, %s, self loops %s' % (knobs or 'default staging', self_loops), self_loops=self_loops)
    finally:
        ing.destroy()


@pytest.mark.parametrize('grid', [1, 2])
def test_one_workgroup_walks_every_row(monkeypatch, grid):
    s = _stream('two_levels')
    in_set = _third_out(s.n)
    in_set[-1] = 0                                                     # the last fragment is not a member
    _rp, _rj, rl = _ref_rows(s, in_set, True)
    ing = _ingest(s)
    try:
        for stage in (None, 7, 0):
            _set_knobs(monkeypatch, HHX_EMIT_GRID=grid, HHX_EMIT_STAGE=stage)
            for self_loops in (True, False):
                n_rest, n_linked = _check_matrix(ing, s.ref, s.n, in_set, 'two_levels, a third out, %d workgroups, stage %s' % (grid, stage),
                                                 self_loops=self_loops)
                assert n_rest > 0 and n_linked == rl and 0 < rl < int(in_set.sum())
    finally:
        ing.destroy()


def test_one_workgroup_and_no_surviving_key(monkeypatch):
    s = _stream('even_odd')
    evens = (np.arange(s.n) % 2 == 0).astype(np.uint8)
    ing = _ingest(s)
    try:
        for grid in (1, 2):
            _set_knobs(monkeypatch, HHX_EMIT_GRID=grid)
            n_rest, n_linked = _check_matrix(ing, s.ref, s.n, evens, 'even-odd keys, the even fragments, %d workgroups' % grid)
            assert (n_rest, n_linked) == (350, 0)
    finally:
        ing.destroy()


@functools.lru_cache(maxsize=None)
def _wide_order_stream(n):
    """n fragments, 3000 of them (spread over the whole range) in 30k pairs, one of those linked to 2600 others inside the flanks"""
    rng = np.random.default_rng(17)
    active = np.sort(rng.choice(n, 3000, replace=False)).astype(np.int32)
    a, p1, b, p2 = _random_pairs(rng, 3000, 30_001)
    others = rng.permutation(np.arange(1, 3000))[:2600].astype(np.int32)
    hub = np.zeros(2600, np.int32) + 1500
    others[others == 1500] = 0
    first = rng.random(2600) < 0.5
    ha, hb = np.where(first, hub, others).astype(np.int32), np.where(first, others, hub).astype(np.int32)
    order = rng.permutation(30_001 + 2600)
    cat = lambda u, v: np.concatenate([u, v])[order]
    return _Stream(n, (active[cat(a, ha)], cat(p1, np.full(2600, 10, np.int32)), active[cat(b, hb)], cat(p2, np.full(2600, 9_990, np.int32))), 7)


@pytest.mark.parametrize('n,stages', [(650_000, (None,)), (600_000, (None, 600))], ids=['650k_direct', '600k_short_passes'])
def test_orders_that_leave_little_lds(monkeypatch, n, stages):
    # the bitmap and prefix take 8 bytes per 32 columns of the 160 KiB: 650k columns leave 1.3 KB (no pass worth its barriers: direct
    # stores), 600k leave 13 KB (1.7k positions a pass); the capacity is 655,232 columns
    s = _wide_order_stream(n)
    in_set = np.ones(n, np.uint8)
    rp, _rj, rl = _ref_rows(s, in_set, True)
    longest = int(np.diff(rp)[:rl].max())
    assert longest > 2600 and rl <= 3000 and len(rp) - 1 == n
    ing = _ingest(s)
    try:
        for S in stages:
            _set_knobs(monkeypatch, HHX_EMIT_STAGE=S)
            _check_matrix(ing, s.ref, n, in_set, '%d fragments, stage %s' % (n, S))
    finally:
        ing.destroy()


def test_two_calls_on_one_handle_under_different_knobs(monkeypatch):
    s = _stream('hub')
    in_set = _third_out(s.n)
    ing = _ingest(s)
    got = []
    try:
        for knobs in ({}, {'HHX_EMIT_STAGE': 333, 'HHX_EMIT_GRID': 3}, {'HHX_EMIT_STAGE': 0}, {}):
            _set_knobs(monkeypatch, **knobs)
            m, fidx, n_linked = ing.link_matrix(in_set, -1)
            try:
                got.append((n_linked, fidx.copy()) + tuple(np.array(x) for x in m.to_arrays()))
            finally:
                m.free()
        for other in got[1:]:
            assert other[0] == got[0][0]
            for u, v in zip(other[1:], got[0][1:]):
                assert np.array_equal(u, v)
        _set_knobs(monkeypatch)
        _check_matrix(ing, s.ref, s.n, in_set, 'hub, a third out')
    finally:
        ing.destroy()
