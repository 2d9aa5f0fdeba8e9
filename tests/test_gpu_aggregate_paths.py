"""The routes of the group-by aggregation (csrc/hhx_ingest.hip: k_aggregate) and the map's grid-stride loop (k_map_records) against the
oracle, bit for bit, tables and link matrix.

  A bucket of 1025..2048 records (all of them in registers) is first taken in ONE pass over the 2048-slot table; more than 1024
  distinct keys abandon the attempt for the sub-passes, and a workgroup carries the outcome to its next bucket.  The streams:
  few keys (single pass taken), every record its own key (abandoned, then skipped), buckets of both kinds in turn (both transitions
  of the carried choice), 1024 and 1025 distinct keys (the boundary), more than 2048 records (no attempt), and the first two pushed
  in three batches (the merge of the runs: MODE 1).  The map: 4k + r pairs on a grid of two workgroups (four grid strides, the
  last one partial) and a stream at a 4-byte offset (the scalar kernel).

Every test first asserts, with a numpy restatement of the bucket hash and of the distinct keys per bucket, the bucket shape that
routes it: a change of constants must not move a test to another path silently.  HHX_AGG_WGS caps the aggregation's workgroups, so
that one workgroup takes several of the few dozen buckets of these streams (by default 1024 workgroups share them, one bucket
each, and nothing is carried); HHX_MAP_GRID caps the map's grid."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_link_build_paths import (CTG_LEN, FLANK, _Stream, _bucket_sizes, _check_matrix, _check_tables, _ingest, _mix64,
                                             _random_pairs, _stream as _build_stream, _table, _third_out)

AG_CAP, AG_REGS = 2048, 4 * 512             # slots of the LDS table; records a workgroup holds in registers (AG_R * AG_T)
HALF = AG_CAP // 2                          # distinct keys one table pass may hold; also the records of one sub-pass


def _total_bits(n_items):
    """csrc/hhx_ingest.hip: ingest_total_bits, first attempt"""
    bits = 0
    while (n_items >> bits) > 2048 and bits < 24:
        bits += 1
    return bits


def _keys(table, id1, id2):
    """keys of the records that survive the map (the key orientation of map_pair: the fragment of lower rank first)"""
    keep = id1 != id2
    a, b = id1[keep].astype(np.int64), id2[keep].astype(np.int64)
    swap = table.ctg_rank[a] > table.ctg_rank[b]
    i, j = np.where(swap, b, a), np.where(swap, a, b)
    return (i.astype(np.uint64) << np.uint64(29)) | j.astype(np.uint64)


def _bucket_of(key, bits):
    return (_mix64(key) >> np.uint64(64 - bits)).astype(np.int64) if bits else np.zeros(len(key), np.int64)


def _shape(keys, n_items):
    """(records, distinct keys) per group-by bucket of a launch over n_items items of which `keys` survive"""
    bits = _total_bits(n_items)
    b = _bucket_of(keys, bits)
    uniq = np.unique(keys)
    return np.bincount(b, minlength=1 << bits), np.bincount(_bucket_of(uniq, bits), minlength=1 << bits)


def _attempted(sizes):
    """buckets that k_aggregate may take in a single pass where the parent took two sub-passes"""
    return (sizes > HALF) & (sizes <= min(AG_CAP, AG_REGS))


def _buckets_per_wg(n_buckets, wgs):
    n_wg = min(n_buckets, wgs)
    return (n_buckets + n_wg - 1) // n_wg


@functools.lru_cache(maxsize=None)
def _stream(name):
    if name == 'few_keys':              # 60k pairs over 40 fragments: at most 780 keys
        return _Stream(40, _random_pairs(np.random.default_rng(21), 40, 60_000), 11)
    if name == 'own_keys':              # 60k pairs over 5000 fragments: 12.5 M possible keys
        return _Stream(5000, _random_pairs(np.random.default_rng(22), 5000, 60_000), 12)
    if name == 'alternating':           # own_keys with the records of every odd bucket moved onto eight keys of that very bucket
        base = _stream('own_keys')
        a, p1, b, p2 = [x.copy() for x in base.pairs]
        table = base.table
        bits = _total_bits(len(a))
        # candidate keys among the first 64 fragments, by bucket
        ci, cj = np.triu_indices(64, 1)
        ck = _keys(table, ci.astype(np.int32), cj.astype(np.int32))
        cb = _bucket_of(ck, bits)
        keep = np.flatnonzero(a != b)
        rb = _bucket_of(_keys(table, a, b), bits)
        rng = np.random.default_rng(23)
        for bucket in range(1, 1 << bits, 2):
            cand = np.flatnonzero(cb == bucket)[:8]
            assert len(cand) == 8
            rows = keep[rb == bucket]
            pick = cand[rng.integers(0, 8, len(rows))]
            flip = rng.random(len(rows)) < 0.5
            a[rows] = np.where(flip, cj[pick], ci[pick]).astype(np.int32)
            b[rows] = np.where(flip, ci[pick], cj[pick]).astype(np.int32)
        return _Stream(5000, (a, p1, b, p2), 12)        # the same seed: the same table
    if name == 'boundary':              # four buckets: 1024 distinct keys, 1025, and two small ones
        rng = np.random.default_rng(24)
        t = _table(5000, 13)
        pa, _p1, pb, _p2 = _random_pairs(rng, 5000, 40_000)
        ok = pa != pb
        pa, pb = pa[ok], pb[ok]
        pk = _keys(t, pa, pb)
        _u, first = np.unique(pk, return_index=True)            # one pair per distinct key
        pa, pb, pk = pa[first], pb[first], pk[first]
        bucket = _bucket_of(pk, 2)
        parts = []
        for bkt, distinct, records in ((0, HALF, 1900), (1, HALF + 1, 1900), (2, 300, 400), (3, 300, 400)):
            own = np.flatnonzero(bucket == bkt)[:distinct]
            assert len(own) == distinct
            parts.append(np.concatenate([own, own[rng.integers(0, distinct, records - distinct)]]))
        rows = rng.permutation(np.concatenate(parts))
        a, b = pa[rows].copy(), pb[rows].copy()
        flip = rng.random(len(rows)) < 0.5
        a[flip], b[flip] = pb[rows][flip], pa[rows][flip]
        n = len(rows)
        return _Stream(5000, (a, rng.integers(0, CTG_LEN, n).astype(np.int32), b, rng.integers(0, CTG_LEN, n).astype(np.int32)), 13)
    if name.startswith('map_tail_'):    # 8000 + r pairs over 700 fragments
        r = int(name[-1])
        return _Stream(700, _random_pairs(np.random.default_rng(30 + r), 640, 8_000 + r), 14)
    raise KeyError(name)


def _check(s, what, cuts=()):
    ing = _ingest(s, cuts)
    try:
        _check_tables(ing, s.ref, what)
        _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), what)
        _check_matrix(ing, s.ref, s.n, _third_out(s.n), what + ', a third out')
    finally:
        ing.destroy()


def test_single_pass_taken(monkeypatch):
    s = _stream('few_keys')
    sizes, distinct = _shape(_keys(s.table, s.pairs[0], s.pairs[2]), len(s.pairs[0]))
    assert len(sizes) == 32 and len(np.unique(_keys(s.table, s.pairs[0], s.pairs[2]))) <= 780
    assert _attempted(sizes).sum() >= 8, 'too few buckets of 1025..2048 records: %s' % sizes
    assert (distinct <= HALF).all()                     # no attempt is abandoned, and the sub-passes of a larger bucket hand `single` on
    monkeypatch.setenv('HHX_AGG_WGS', '4')
    assert _buckets_per_wg(len(sizes), 4) == 8
    _check(s, 'few keys')


def test_attempt_abandoned_then_skipped(monkeypatch):
    s = _stream('own_keys')
    sizes, distinct = _shape(_keys(s.table, s.pairs[0], s.pairs[2]), len(s.pairs[0]))
    assert len(sizes) == 32
    assert (distinct[sizes > 0] > HALF).all() and (sizes <= AG_CAP).all() and _attempted(sizes).all()
    monkeypatch.setenv('HHX_AGG_WGS', '4')              # the first bucket of a workgroup abandons its attempt, the other seven make none
    assert _buckets_per_wg(len(sizes), 4) == 8
    _check(s, 'own keys')


def test_alternating_buckets(monkeypatch):
    s = _stream('alternating')
    sizes, distinct = _shape(_keys(s.table, s.pairs[0], s.pairs[2]), len(s.pairs[0]))
    assert len(sizes) == 32 and _attempted(sizes).all()
    many = distinct > HALF
    assert many[0::2].all() and not many[1::2].any()    # 32 consecutive buckets alternate: abandoned, sub-passes that re-arm, taken, ...
    assert (distinct[1::2] <= 8).all()
    monkeypatch.setenv('HHX_AGG_WGS', '2')
    assert _buckets_per_wg(len(sizes), 2) == 16
    _check(s, 'alternating buckets')


def test_boundary_of_the_single_pass(monkeypatch):
    s = _stream('boundary')
    sizes, distinct = _shape(_keys(s.table, s.pairs[0], s.pairs[2]), len(s.pairs[0]))
    assert len(sizes) == 4
    assert distinct[0] == HALF and distinct[1] == HALF + 1
    assert _attempted(sizes[:2]).all() and (sizes[2:] <= HALF).all()
    monkeypatch.setenv('HHX_AGG_WGS', '1')              # one workgroup: taken at 1024, abandoned at 1025, then two one-pass buckets
    _check(s, '1024 and 1025 distinct keys')


def test_bucket_beyond_the_register_set():
    s = _build_stream('heavy_keys')
    sizes = _bucket_sizes(s.table, s.pairs[0], s.pairs[2])
    assert (sizes > max(AG_CAP, AG_REGS)).any() and _attempted(sizes).any()
    _check(s, 'heavy keys')                             # 10k records of one key in a bucket: the record count alone keeps it on the sub-passes


@pytest.mark.parametrize('name', ['few_keys', 'own_keys'])
def test_merge_of_three_runs(name, monkeypatch):
    s = _stream(name)
    cuts = (20_000, 40_000)
    edges = (0,) + cuts + (len(s.pairs[0]),)
    rows = np.concatenate([np.unique(_keys(s.table, s.pairs[0][lo:hi], s.pairs[2][lo:hi])) for lo, hi in zip(edges[:-1], edges[1:])])
    sizes, distinct = _shape(rows, len(rows))           # the merge aggregates the rows of the three runs (k_aggregate<1>)
    assert _attempted(sizes).any()
    if name == 'few_keys':
        assert (distinct <= HALF).all()
    else:
        assert (distinct[_attempted(sizes)] > HALF).all() and _attempted(sizes).sum() >= 8
    for lo, hi in zip(edges[:-1], edges[1:]):           # ... and every push on its own reaches the attempt too
        assert _attempted(_shape(_keys(s.table, s.pairs[0][lo:hi], s.pairs[2][lo:hi]), hi - lo)[0]).any()
    monkeypatch.setenv('HHX_AGG_WGS', '4')
    _check(s, name + ' in three pushes', cuts)


@pytest.mark.parametrize('r', [0, 1, 2, 3])
def test_map_grid_strides_and_tail(r, monkeypatch):
    s = _stream('map_tail_%d' % r)
    n = len(s.pairs[0])
    assert n == 8_000 + r
    monkeypatch.setenv('HHX_MAP_GRID', '2')             # 2000 groups of four pairs on 512 lanes: four strides, the last one of 464 lanes
    assert (n // 4) > 3 * 2 * 256 and (n // 4) % (2 * 256) != 0
    _check(s, '%d pairs on two workgroups' % n)


def test_map_from_an_unaligned_pointer():
    import torch
    from haphic_amd import _lib
    s = _stream('map_tail_1')
    n = len(s.pairs[0])
    dev = [torch.from_numpy(np.concatenate([np.zeros(1, np.int32), x])).to('cuda') for x in s.pairs]
    ptrs = [x[1:].data_ptr() for x in dev]
    assert all(p % 16 == 4 for p in ptrs)               # not 16-byte aligned: the one-pair-per-lane kernel takes every pair
    ing = _lib.Ingest(s.table, FLANK, bins=False, skip_intra=True)
    try:
        ing.push_device(n, *ptrs)
        torch.cuda.synchronize()
        ing.finalize()
        _check_tables(ing, s.ref, 'unaligned push')
        _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), 'unaligned push')
    finally:
        ing.destroy()
