"""The first-position cut of the link-matrix build (csrc/hhx_matrix.hip: SrcDirectedPacked::mark_load, k_first_unsettled,
k_first_repair; HHX_D2M_FIRST_CUT) against the oracle, bit for bit, at every seam of the cut.

A directed entry whose position 2 * ordinal + side lies at or past the cut takes no read of the first-position table; a fragment
all of whose entries lie there is found afterwards and repaired from the whole table.  For every cut the matrix, frag_index and
n_linked must be the oracle's, and the two profile counters must be what the stream says they are, so that no case passes without
the path it is about having run:

  d2m_first_reads      directed entries (both ends in frag_set) of a key whose ordinal is below the cut
  d2m_first_unsettled  fragments with entries none of which is below the cut

The ordinal of a key is the stream index of its first flank-qualified pair, intra-contig pairs counted; it is computed here on the
host and checked against the oracle's insertion order.  The knob counts ORDINALS from the ingest's base, so the cut is an even
position: the two directed entries of one key (positions 2 * ord and 2 * ord + 1) always fall on the same side of it.  The tie of a
key that is the first entry of both its fragments is therefore pinned at cut == ord (both fragments repaired) and ord + 1 (both read)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_link_build_paths import CTG_LEN, FLANK, _Stream, _check_matrix, _ingest, _random_pairs

NO_CUT = 1 << 40


def _key_ordinals(s):
    """(flank_i, flank_j, ordinal) of every flank key, in insertion order — which must be the oracle's"""
    a, p1, b, p2 = [x.astype(np.int64) for x in s.pairs]
    rank = s.table.ctg_rank.astype(np.int64)
    swap = rank[a] > rank[b]
    i, j = np.where(swap, b, a), np.where(swap, a, b)
    yi, yj = np.where(swap, p2, p1) + 1, np.where(swap, p1, p2) + 1
    in_flank = lambda y: (y <= FLANK) | (y > CTG_LEN - FLANK)
    t = np.flatnonzero((a != b) & in_flank(yi) & in_flank(yj))
    _, first = np.unique(i[t] * s.n + j[t], return_index=True)
    ordinal = np.sort(t[first])
    fi, fj = i[ordinal].astype(np.int32), j[ordinal].astype(np.int32)
    assert np.array_equal(fi, s.ref['flank_i']) and np.array_equal(fj, s.ref['flank_j']), 'host ordinals disagree with the oracle\'s order'
    return fi, fj, ordinal


def _expect(s, in_set, cut):
    """(entries below the cut, unsettled fragments, directed entries, linked fragments) for a cut of `cut` ordinals from the base"""
    fi, fj, ordinal = _key_ordinals(s)
    in_set = np.asarray(in_set, bool)
    ok = in_set[fi] & in_set[fj]
    below = ok & (ordinal < cut)                                 # (the ordinals here count from 0, as the knob does from the base)
    first = np.full(s.n, np.iinfo(np.int64).max)
    np.minimum.at(first, fi[ok], ordinal[ok])
    np.minimum.at(first, fj[ok], ordinal[ok])
    linked = first != np.iinfo(np.int64).max
    return 2 * int(below.sum()), int((linked & (first >= cut)).sum()), 2 * int(ok.sum()), int(linked.sum())


def _counters():
    from haphic_amd import _lib
    return _lib.profile_counter('d2m_first_reads'), _lib.profile_counter('d2m_first_unsettled')


@pytest.fixture
def profiled():
    from haphic_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    yield
    _lib.profile_enable(False)
    _lib.profile_reset()


def _run(ing, s, in_set, cut, what, monkeypatch, **kw):
    """one link_matrix call under HHX_D2M_FIRST_CUT = cut (None: unset) against the oracle; returns (reads, unsettled) of that call"""
    from haphic_amd import _lib
    if cut is None:
        monkeypatch.delenv('HHX_D2M_FIRST_CUT', raising=False)
    else:
        monkeypatch.setenv('HHX_D2M_FIRST_CUT', str(cut))
    _lib.profile_reset()
    _check_matrix(ing, s.ref, s.n, in_set, what, **kw)
    return _counters()


def _third_out(n):
    return (np.arange(n) % 3 != 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _stream(name):
    if name == 'two_levels':            # 700 fragments (both radix levels), 60 of them in no pair
        return _Stream(700, _random_pairs(np.random.default_rng(21), 640, 20_001), 1)
    if name == 'one_level':
        return _Stream(40, _random_pairs(np.random.default_rng(22), 35, 4_003), 2)
    if name == 'late':                  # 680 fragments in the first 20k pairs, 20 more only in the 600 pairs behind them
        rng = np.random.default_rng(23)
        early = _random_pairs(rng, 680, 20_000)
        a, p1, b, p2 = _random_pairs(rng, 20, 600)
        return _Stream(700, tuple(np.concatenate([u, v]) for u, v in zip(early, (a + 680, p1, b + 680, p2))), 3)
    if name == 'early_do_not_count':
        # fragment 100: in the first 3000 pairs its partners are all odd fragments (kept out of frag_set), later even ones too;
        # fragment 102: in the first 3000 pairs its coordinates lie outside the flanks (no flank ordinal), later inside
        rng = np.random.default_rng(24)
        n_pairs = 12_000
        a = (2 * rng.integers(0, 350, n_pairs)).astype(np.int32)         # even-even background, fragments 100 and 102 kept out of it
        b = (2 * rng.integers(0, 350, n_pairs)).astype(np.int32)
        a[(a == 100) | (a == 102)] = 104
        b[(b == 100) | (b == 102)] = 106
        p1, p2 = rng.integers(0, FLANK, n_pairs).astype(np.int32), rng.integers(0, FLANK, n_pairs).astype(np.int32)
        for lo, hi, odd_only in ((0, 3_000, True), (3_000, 12_000, False)):
            t = lo + rng.choice(hi - lo, 60 if lo == 0 else 200, replace=False)
            a[t] = 100
            b[t] = (2 * rng.integers(0, 350, len(t)) + 1).astype(np.int32) if odd_only else (2 * rng.integers(0, 40, len(t))).astype(np.int32)
        t = rng.choice(3_000, 60, replace=False)
        a[t], b[t], p1[t] = 102, (2 * rng.integers(0, 40, 60)).astype(np.int32), CTG_LEN // 2       # outside the flanks
        t = 3_000 + rng.choice(9_000, 200, replace=False)
        a[t], b[t] = 102, (2 * rng.integers(0, 40, 200)).astype(np.int32)
        return _Stream(700, (a, p1, b, p2), 4)
    if name == 'tie':                   # pair 5000 joins fragments 690 and 691, which occur nowhere before it
        a, p1, b, p2 = _random_pairs(np.random.default_rng(25), 690, 9_000)
        a[5_000], b[5_000], p1[5_000], p2[5_000] = 690, 691, 5, 7
        a[7_000:7_050], b[7_000:7_050] = 690, np.arange(50, dtype=np.int32)
        b[8_000:8_050], a[8_000:8_050] = 691, np.arange(50, dtype=np.int32)
        return _Stream(700, (a, p1, b, p2), 5)
    if name == 'many_tiles':            # 60k pairs: > 15 tiles of 7168 directed entries in the level-1 count pass
        return _Stream(700, _random_pairs(np.random.default_rng(26), 700, 60_000), 6)
    raise KeyError(name)


@pytest.mark.parametrize('name', ['two_levels', 'one_level'])
def test_cut_seams(name, profiled, monkeypatch):
    s = _stream(name)
    in_set = np.ones(s.n, np.uint8)
    _fi, _fj, ordinal = _key_ordinals(s)
    first, median, last = int(ordinal[0]), int(ordinal[len(ordinal) // 2]), int(ordinal[-1])
    ing = _ingest(s)
    try:
        seen = set()
        for cut in (0, 1, first, first + 1, median, last, last + 1, NO_CUT):
            reads, unsettled, entries, linked = _expect(s, in_set, cut)
            got = _run(ing, s, in_set, cut, '%s, cut %d' % (name, cut), monkeypatch)
            assert got == (reads, unsettled), '%s, cut %d: (reads, unsettled)' % (name, cut)
            seen.add((reads == 0, reads == entries, unsettled == 0, unsettled == linked))
            if cut == 0:
                assert (reads, unsettled) == (0, linked) and linked > 0            # every linked fragment repaired
            if cut == first + 1:
                assert reads == 2 and unsettled == linked - 2                      # one key read, its two fragments settled
            if cut == last:
                assert reads == entries - 2
            if cut in (last + 1, NO_CUT):
                assert (reads, unsettled) == (entries, 0)                          # nothing repaired
        assert len(seen) >= 3
        # a third of the fragments out of frag_set: entries dropped by membership are not counted, their fragments not unsettled
        in_set = _third_out(s.n)
        reads, unsettled, entries, linked = _expect(s, in_set, median)
        assert 0 < reads < entries and 0 < linked
        assert _run(ing, s, in_set, median, name + ', a third out', monkeypatch) == (reads, unsettled)
    finally:
        ing.destroy()


def test_late_fragments(profiled, monkeypatch):
    s = _stream('late')
    in_set = np.ones(s.n, np.uint8)
    fi, fj, ordinal = _key_ordinals(s)
    late_linked = int(np.union1d(fi[fi >= 680], fj[fj >= 680]).size)
    assert 10 <= late_linked <= 20 and ordinal[fi >= 680].min() >= 20_000
    ing = _ingest(s)
    try:
        reads, unsettled, entries, _linked = _expect(s, in_set, 20_000)
        assert unsettled == late_linked and 0 < reads < entries
        assert _run(ing, s, in_set, 20_000, 'late fragments', monkeypatch) == (reads, late_linked)
    finally:
        ing.destroy()


def test_early_entries_that_do_not_count(profiled, monkeypatch):
    s = _stream('early_do_not_count')
    in_set = (np.arange(s.n) % 2 == 0).astype(np.uint8)                  # the even fragments
    fi, fj, ordinal = _key_ordinals(s)
    with_100 = (fi == 100) | (fj == 100)
    partner = np.where(fi == 100, fj, fi)[with_100]
    early = ordinal[with_100] < 3_000
    assert early.any() and (partner[early] % 2 == 1).all() and (partner[~early] % 2 == 0).any()
    with_102 = (fi == 102) | (fj == 102)
    assert with_102.any() and ordinal[with_102].min() >= 3_000                  # its early pairs never entered the flank table
    assert ((s.pairs[0][:3_000] == 102) | (s.pairs[2][:3_000] == 102)).any()
    ing = _ingest(s)
    try:
        reads, unsettled, entries, linked = _expect(s, in_set, 3_000)
        assert unsettled == 2 and 0 < reads < entries and linked > 100          # exactly the two, everything else settled early
        assert _run(ing, s, in_set, 3_000, 'early entries that do not count', monkeypatch) == (reads, 2)
    finally:
        ing.destroy()


def test_key_that_is_first_for_both_its_fragments(profiled, monkeypatch):
    s = _stream('tie')
    in_set = np.ones(s.n, np.uint8)
    fi, fj, ordinal = _key_ordinals(s)
    k = int(np.flatnonzero(ordinal == 5_000)[0])
    assert {int(fi[k]), int(fj[k])} == {690, 691}
    assert ordinal[(fi == 690) | (fj == 690)].min() == 5_000 == ordinal[(fi == 691) | (fj == 691)].min()
    ing = _ingest(s)
    try:
        at = _expect(s, in_set, 5_000)
        past = _expect(s, in_set, 5_001)
        assert at[1] == past[1] + 2 and past[0] == at[0] + 2                    # both sides of the key change sides together
        assert _run(ing, s, in_set, 5_000, 'tie, cut at the key', monkeypatch) == at[:2]
        assert _run(ing, s, in_set, 5_001, 'tie, cut behind the key', monkeypatch) == past[:2]
    finally:
        ing.destroy()


@pytest.mark.parametrize('cuts', [(7_003,), (1, 9_998)], ids=['two_pushes', 'three_pushes'])
def test_pushes_of_one_stream(cuts, profiled, monkeypatch):
    s = _stream('two_levels')
    in_set = _third_out(s.n)
    _fi, _fj, ordinal = _key_ordinals(s)
    ing = _ingest(s, cuts)
    try:
        for cut in (0, int(ordinal[len(ordinal) // 2]), cuts[-1], None):
            c = cut if cut is not None else (len(s.pairs[0]) + 15) // 16
            reads, unsettled, entries, _linked = _expect(s, in_set, c)
            assert _run(ing, s, in_set, cut, '%d pushes, cut %s' % (len(cuts) + 1, cut), monkeypatch) == (reads, unsettled)
            if cut is None:
                assert 0 < reads < entries // 8
    finally:
        ing.destroy()


def test_ordinal_base_keeps_the_fast_path(profiled, monkeypatch):
    import torch
    from haphic_amd import _lib
    s = _stream('two_levels')
    base = 1_000_003
    in_set = np.ones(s.n, np.uint8)
    dev = [torch.from_numpy(x).to('cuda') for x in s.pairs]
    ing = _lib.Ingest(s.table, FLANK, bins=False, skip_intra=True)
    try:
        ing.set_ordinal_base(base)
        ing.push_device(len(s.pairs[0]), *[x.data_ptr() for x in dev])
        torch.cuda.synchronize()
        ing.finalize()
        default = (len(s.pairs[0]) + 15) // 16                                  # a sixteenth of the ordinals seen, counted from the base
        reads, unsettled, entries, _linked = _expect(s, in_set, default)
        assert 0 < reads < entries // 8, 'the default cut must leave most entries without a table read'
        assert _run(ing, s, in_set, None, 'ordinal base, default cut', monkeypatch) == (reads, unsettled)
        # ... and the knob counts from the base too
        reads, unsettled, _entries, _linked = _expect(s, in_set, 5_000)
        assert unsettled > 0
        assert _run(ing, s, in_set, 5_000, 'ordinal base, cut 5000', monkeypatch) == (reads, unsettled)
    finally:
        ing.destroy()


@pytest.mark.parametrize('grid', [1, 2])
def test_one_workgroup_through_many_tiles(grid, profiled, monkeypatch):
    s = _stream('many_tiles')
    in_set = np.ones(s.n, np.uint8)
    monkeypatch.setenv('HHX_PART_GRID', str(grid))
    ing = _ingest(s)
    try:
        assert 2 * ing.n_full > 14 * 7168, 'fewer than fifteen count tiles'
        for cut in (2_000, 30_000):
            reads, unsettled, entries, _linked = _expect(s, in_set, cut)
            assert 0 < reads < entries                                          # skipped and read records side by side in every tile
            assert _run(ing, s, in_set, cut, 'HHX_PART_GRID=%d, cut %d' % (grid, cut), monkeypatch) == (reads, unsettled)
    finally:
        ing.destroy()


def test_two_sets_on_one_handle(profiled, monkeypatch):
    s = _stream('two_levels')
    evens = (np.arange(s.n) % 2 == 0).astype(np.uint8)
    ing = _ingest(s)
    try:
        for in_set, cut in ((evens, 300), (_third_out(s.n), 9_000), (evens, NO_CUT), (np.ones(s.n, np.uint8), 0)):
            reads, unsettled, _entries, _linked = _expect(s, in_set, cut)
            assert _run(ing, s, in_set, cut, 'set of %d members, cut %d' % (int(in_set.sum()), cut), monkeypatch) == (reads, unsettled)
        assert _expect(s, evens, 300)[1] > 0 and _expect(s, _third_out(s.n), 9_000)[1] == 0
    finally:
        ing.destroy()


def test_membership_words_from_global_memory(profiled, monkeypatch):
    s = _stream('two_levels')
    in_set = _third_out(s.n)
    monkeypatch.setenv('HHX_D2M_LDS_FRAGS', '0')
    ing = _ingest(s)
    try:
        for cut in (0, 2_000, NO_CUT):
            reads, unsettled, _entries, _linked = _expect(s, in_set, cut)
            assert _run(ing, s, in_set, cut, 'HHX_D2M_LDS_FRAGS=0, cut %d' % cut, monkeypatch) == (reads, unsettled)
    finally:
        ing.destroy()
