"""The phases of one bucket of the group-by aggregation (csrc/hhx_ingest.hip: k_aggregate — clear, insert, scan, reservation, write-out)
against the oracle, bit for bit, tables and link matrix, at the bucket shapes where they take another path.

  Same-key records: one key for all 3,000 records of a bucket, two keys, and buckets of two or three keys whose threads hold four
  register records each (a thread then holds the same key twice: the records of ONE thread race for one empty slot).
  Small tables: buckets of exactly 1, 2, 31, 32, 33, 255, 256, 511, 512, 1,023 and 1,024 records with all-distinct keys — tables of
  64 up to 2,048 slots, one, two and four slots a thread, threads beyond the table idle; the 31 keys of the 64-slot table are chosen
  at the end of the table, so that their probe chains wrap it; five of the sixteen buckets are empty, between the full ones.
  Single-pass boundaries: 2,048 and 2,049 records, 1,024 and 1,025 distinct keys, a bucket of more than 4,096 records and one of
  70,001 records on a single key (a count above 65,535, sixteen sub-passes, the loop over the records beyond the registers).
  Mixed records: keys seen only outside the flanks, only inside and both, in one bucket.  (The map of these streams is the combined
  one, `bins=False`: a record inside the flanks counts for the full table as well, so "flank only" is a key ALL of whose records
  lie inside; records with the flank bit alone belong to the fragment stream of a split assembly, which is a table of its own.)
  Workgroup counts: one and two workgroups over all sixteen buckets (HHX_AGG_WGS), and the default.
  Merges: the same streams in three pushes (k_aggregate<1>), and two ingests on one process back to back.

Every case first asserts, with the numpy restatement of the bucket hash, the bucket shape that routes it.  The streams are built on the
host from a seed; the oracle's tables are computed once per stream and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_aggregate_paths import (AG_CAP, AG_REGS, HALF, _bucket_of, _check, _keys, _shape, _stream as _paths_stream,
                                            _total_bits)
from tests.test_gpu_link_build_paths import (CTG_LEN, FLANK, _Stream, _check_matrix, _check_tables, _ingest, _mix64, _random_pairs,
                                             _table, _third_out)

SMALL = (1, 2, 31, 32, 33, 255, 256, 511, 512, 1023, 1024)
SMALL_BUCKETS = (0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15)      # of sixteen: 2, 5, 8, 11 and 14 stay empty
N_FRAG = 5000


def _tsize(records):
    """slots of the table of one pass over `records` records (csrc/hhx_ingest.hip: tsize)"""
    per = records + 1
    if 2 * per > AG_CAP:
        return AG_CAP
    t = 64
    while t < 2 * per:
        t <<= 1
    return t


def _sub_bits(records):
    bits = 0
    while (records >> bits) > 1024 and bits < 4:
        bits += 1
    return bits


def _wrapped(keys, tsize):
    """keys that end up in front of their home slot when inserted with linear probing (the occupied set does not depend on the order)"""
    occ = np.zeros(tsize, bool)
    wrapped = 0
    for h in (_mix64(keys) & np.uint64(tsize - 1)).astype(np.int64).tolist():
        s = h
        while occ[s]:
            s = (s + 1) % tsize
        occ[s] = True
        wrapped += s < h
    return wrapped


def _exact(spec, n_items, seed, at_table_end=()):
    """A stream of n_items pairs whose group-by buckets are exactly `spec`: (bucket, records, distinct keys) each, every other bucket empty.
    The pairs beyond the records of `spec` are intra-contig ones, which the map drops.  A bucket named in `at_table_end` takes the keys
    whose home slots are the last ones of its table."""
    rng = np.random.default_rng(seed)
    table = _table(N_FRAG, seed)
    bits = _total_bits(n_items)
    pa, _p1, pb, _p2 = _random_pairs(rng, N_FRAG, 120_000)
    ok = pa != pb
    pa, pb = pa[ok], pb[ok]
    pk = _keys(table, pa, pb)
    _u, first = np.unique(pk, return_index=True)                # one pair per distinct key
    pa, pb, pk = pa[first], pb[first], pk[first]
    bucket = _bucket_of(pk, bits)
    parts = []
    for bkt, records, distinct in spec:
        own = np.flatnonzero(bucket == bkt)
        if bkt in at_table_end:
            ts = _tsize(records)
            own = own[np.argsort(-(_mix64(pk[own]) & np.uint64(ts - 1)).astype(np.int64), kind='stable')]
        own = own[:distinct]
        assert len(own) == distinct, 'bucket %d has %d candidate keys' % (bkt, len(own))
        parts.append(np.concatenate([own, own[rng.integers(0, distinct, records - distinct)]]))
    rows = np.concatenate(parts)
    n_pad = n_items - len(rows)
    assert n_pad >= 0
    a = np.concatenate([pa[rows], rng.integers(0, N_FRAG, n_pad).astype(np.int32)])
    b = np.concatenate([pb[rows], a[len(rows):]])
    flip = rng.random(n_items) < 0.5
    a, b = np.where(flip, b, a).astype(np.int32), np.where(flip, a, b).astype(np.int32)
    order = rng.permutation(n_items)
    a, b = a[order], b[order]
    return _Stream(N_FRAG, (a, rng.integers(0, CTG_LEN, n_items).astype(np.int32), b, rng.integers(0, CTG_LEN, n_items).astype(np.int32)), seed)


@functools.lru_cache(maxsize=None)
def _stream(name):
    if name == 'one_key':               # 3,000 pairs of fragments 3 and 4
        rng = np.random.default_rng(41)
        n = 3_000
        flip = rng.random(n) < 0.5
        a, b = np.where(flip, 3, 4).astype(np.int32), np.where(flip, 4, 3).astype(np.int32)
        return _Stream(40, (a, rng.integers(0, CTG_LEN, n).astype(np.int32), b, rng.integers(0, CTG_LEN, n).astype(np.int32)), 41)
    if name == 'two_keys':              # 3,000 pairs over two keys of one bucket
        rng = np.random.default_rng(42)
        n = 3_000
        t = _table(40, 42)
        ci, cj = np.triu_indices(40, 1)
        cb = _bucket_of(_keys(t, ci.astype(np.int32), cj.astype(np.int32)), _total_bits(n))
        pick = np.flatnonzero(cb == cb[0])[:2][rng.integers(0, 2, n)]
        flip = rng.random(n) < 0.5
        a, b = np.where(flip, cj[pick], ci[pick]).astype(np.int32), np.where(flip, ci[pick], cj[pick]).astype(np.int32)
        return _Stream(40, (a, rng.integers(0, CTG_LEN, n).astype(np.int32), b, rng.integers(0, CTG_LEN, n).astype(np.int32)), 42)
    if name == 'twelve_fragments':      # 60k pairs over 12 fragments: 66 keys in 32 buckets
        return _Stream(12, _random_pairs(np.random.default_rng(43), 12, 60_000), 43)
    if name == 'small_tables':          # sixteen buckets: eleven of exactly SMALL records, all keys distinct, five empty
        return _exact([(b, n, n) for b, n in zip(SMALL_BUCKETS, SMALL)], 20_000, 44, at_table_end=(SMALL_BUCKETS[2],))
    if name == 'boundaries':            # 64 buckets: 2,048 and 2,049 records, more than 4,096, and 70,001 records of one key
        return _exact([(3, 2048, 300), (10, 2049, 300), (20, 4500, 200), (40, 70_001, 1)], 90_000, 45)
    if name == 'mixed':                 # one bucket; keys 0..12 inside the flanks only, 13..25 outside only, 26..39 both
        rng = np.random.default_rng(46)
        n = 1_500
        ci, cj = np.triu_indices(12, 1)
        which = rng.integers(0, 40, n)
        inside = np.where(which < 13, True, np.where(which < 26, False, rng.random(n) < 0.5))
        lo = rng.random(n) < 0.5
        p_in = np.where(lo, rng.integers(0, FLANK - 1, n), rng.integers(CTG_LEN - FLANK, CTG_LEN, n))     # 1-based coordinate <= FLANK or > length - FLANK
        p_out = rng.integers(FLANK, CTG_LEN - FLANK - 1, n)
        p1 = np.where(inside, p_in, p_out).astype(np.int32)
        p2 = np.where(inside, np.where(lo, 5, CTG_LEN - 5), p_out[::-1]).astype(np.int32)
        flip = rng.random(n) < 0.5
        a, b = np.where(flip, cj[which], ci[which]).astype(np.int32), np.where(flip, ci[which], cj[which]).astype(np.int32)
        return _Stream(40, (a, p1, b, p2), 46)
    raise KeyError(name)


def _shape_of(s):
    return _shape(_keys(s.table, s.pairs[0], s.pairs[2]), len(s.pairs[0]))


# ---- same-key records
def test_one_key_for_a_whole_bucket():
    s = _stream('one_key')
    sizes, distinct = _shape_of(s)
    assert sorted(sizes.tolist()) == [0, 3000] and distinct.max() == 1
    assert _sub_bits(3000) == 2                          # four sub-passes, three of them without a record; 952 records beyond the registers
    _check(s, 'one key')
    assert s.ref['full_cnt'].tolist() == [3000]


def test_two_keys_in_one_bucket():
    s = _stream('two_keys')
    sizes, distinct = _shape_of(s)
    assert sorted(sizes.tolist()) == [0, 3000] and sorted(distinct.tolist()) == [0, 2]
    _check(s, 'two keys')


def test_threads_holding_one_key_twice(monkeypatch):
    s = _stream('twelve_fragments')
    sizes, distinct = _shape_of(s)
    assert len(sizes) == 32
    # more than 1,536 records in registers: every thread holds three of them, the first ones four; two keys: every thread holds a key twice
    crowded = (sizes > 3 * 512) & (sizes <= AG_REGS) & (distinct <= 2)
    assert crowded.sum() >= 8, 'buckets %s keys %s' % (sizes, distinct)
    monkeypatch.setenv('HHX_AGG_WGS', '4')
    _check(s, 'twelve fragments')
    few = _paths_stream('few_keys')                      # ~24 keys a bucket: about a quarter of the threads hold one twice
    f_sizes, f_distinct = _shape(_keys(few.table, few.pairs[0], few.pairs[2]), len(few.pairs[0]))
    assert ((f_sizes > 1536) & (f_distinct <= 40)).sum() >= 8
    _check(few, 'few keys')


# ---- small tables, workgroup counts
@pytest.mark.parametrize('wgs', [None, '1', '2'], ids=['default', 'one_workgroup', 'two_workgroups'])
def test_small_tables_and_empty_buckets(wgs, monkeypatch):
    s = _stream('small_tables')
    sizes, distinct = _shape_of(s)
    assert len(sizes) == 16
    assert sizes[list(SMALL_BUCKETS)].tolist() == list(SMALL) and sizes.sum() == sum(SMALL)     # the other five are empty
    assert (distinct == sizes).all()                     # every record its own key
    assert [_tsize(n) for n in SMALL] == [64, 64, 64, 128, 128, 512, 1024, 1024, 2048, 2048, 2048]
    assert sorted({max(1, _tsize(n) // 512) for n in SMALL}) == [1, 2, 4]                       # slots a thread
    keys = _keys(s.table, s.pairs[0], s.pairs[2])
    k31 = np.unique(keys[_bucket_of(keys, 4) == SMALL_BUCKETS[2]])
    assert len(k31) == 31 and _wrapped(k31, 64) >= 1     # a probe chain runs over the end of the 64-slot table
    if wgs is not None:
        monkeypatch.setenv('HHX_AGG_WGS', wgs)
    else:
        monkeypatch.delenv('HHX_AGG_WGS', raising=False)
    _check(s, 'small tables, workgroups %s' % wgs)


# ---- single-pass boundaries
@pytest.mark.parametrize('wgs', [None, '1'], ids=['default', 'one_workgroup'])
def test_record_count_boundaries_and_a_heavy_key(wgs, monkeypatch):
    s = _stream('boundaries')
    sizes, distinct = _shape_of(s)
    assert len(sizes) == 64
    assert (sizes[3], sizes[10], sizes[20], sizes[40]) == (2048, 2049, 4500, 70_001) and sizes.sum() == 2048 + 2049 + 4500 + 70_001
    assert sizes[3] == AG_REGS and sizes[10] == AG_REGS + 1                                   # the last bucket held in registers, the first that is not
    assert (distinct[3], distinct[10], distinct[20], distinct[40]) == (300, 300, 200, 1)
    assert (_sub_bits(2048), _sub_bits(2049), _sub_bits(4500), _sub_bits(70_001)) == (1, 1, 3, 4)
    if wgs is not None:
        monkeypatch.setenv('HHX_AGG_WGS', wgs)
    else:
        monkeypatch.delenv('HHX_AGG_WGS', raising=False)
    _check(s, 'boundaries, workgroups %s' % wgs)
    assert s.ref['full_cnt'].max() == 70_001             # a count above 65,535


def test_distinct_key_boundary(monkeypatch):
    s = _paths_stream('boundary')
    sizes, distinct = _shape(_keys(s.table, s.pairs[0], s.pairs[2]), len(s.pairs[0]))
    assert distinct[0] == HALF and distinct[1] == HALF + 1 and (sizes[:2] <= AG_REGS).all() and (sizes[:2] > HALF).all()
    monkeypatch.setenv('HHX_AGG_WGS', '1')
    _check(s, '1024 and 1025 distinct keys, one workgroup')
    monkeypatch.setenv('HHX_AGG_WGS', '2')
    _check(s, '1024 and 1025 distinct keys, two workgroups')


# ---- mixed records
def test_keys_inside_outside_and_across_the_flanks():
    s = _stream('mixed')
    sizes, _distinct = _shape_of(s)
    assert len(sizes) == 1                               # one bucket
    full = set(zip(s.ref['full_i'].tolist(), s.ref['full_j'].tolist()))
    flank = dict(zip(zip(s.ref['flank_i'].tolist(), s.ref['flank_j'].tolist()), s.ref['flank_cnt'].tolist()))
    cnt = dict(zip(zip(s.ref['full_i'].tolist(), s.ref['full_j'].tolist()), s.ref['full_cnt'].tolist()))
    only_full = [k for k in full if k not in flank]
    all_flank = [k for k in flank if flank[k] == cnt[k]]
    both = [k for k in flank if flank[k] < cnt[k]]
    assert len(only_full) >= 8 and len(all_flank) >= 8 and len(both) >= 8, (len(only_full), len(all_flank), len(both))
    _check(s, 'mixed records')


# ---- merges
@pytest.mark.parametrize('name,cuts', [('small_tables', (6_000, 13_000)), ('boundaries', (30_000, 60_000)), ('one_key', (1_000, 2_000))])
def test_three_pushes(name, cuts, monkeypatch):
    s = _stream(name)
    edges = (0,) + cuts + (len(s.pairs[0]),)
    rows = np.concatenate([np.unique(_keys(s.table, s.pairs[0][lo:hi], s.pairs[2][lo:hi])) for lo, hi in zip(edges[:-1], edges[1:])])
    uniq = len(np.unique(rows))
    assert len(rows) > uniq or name == 'small_tables'    # the runs share keys: the merge adds counts and takes minima
    if name == 'small_tables':
        assert len(rows) == uniq == sum(SMALL)           # ... or none: every row passes through the merge unchanged
    sizes, _distinct = _shape(rows, len(rows))
    assert sizes.sum() == len(rows) and len(sizes) == 1 << _total_bits(len(rows))
    monkeypatch.delenv('HHX_AGG_WGS', raising=False)
    _check(s, name + ' in three pushes', cuts)


def test_two_ingests_back_to_back():
    a, b = _stream('small_tables'), _stream('mixed')
    assert len(_shape_of(a)[0]) == 16 and len(_shape_of(b)[0]) == 1
    first = _ingest(a)
    second = _ingest(b)                                  # a second handle while the first is alive
    try:
        _check_tables(second, b.ref, 'second ingest')
        _check_tables(first, a.ref, 'first ingest')
        _check_matrix(first, a.ref, a.n, _third_out(a.n), 'first ingest, a third out')
        _check_matrix(second, b.ref, b.n, np.ones(b.n, np.uint8), 'second ingest')
    finally:
        first.destroy()
        second.destroy()
    _check(a, 'small tables again')                      # ... and the same stream once more on the same process
