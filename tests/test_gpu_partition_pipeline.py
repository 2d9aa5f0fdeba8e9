"""The tile loop of the radix partition's scatter pass (csrc/hhx_partition.h: k_part_scatter keeps the next tile of a workgroup in
flight while it stages and writes the current one) through Ingest.push_device -> finalize -> link_matrix, against the oracle, bit for
bit: tables, n_linked, frag_index and the CSR triple, checked the way tests/test_gpu_link_build_paths.py checks them.

HHX_PART_GRID (read at every launch) caps the grid of the count and scatter passes at 1, 2 and 3 workgroups, so the few tens of
thousands of records of a stream are 5-10 scatter tiles of 8192 (12-byte records; 7168 and 14336 for the 8-byte matrix entries of the
first and second level) and every workgroup walks several tiles through the prefetch; every case runs at each cap.

  * exactly 1 tile, 1 tile + 1, 2 tiles - 1 and grid x tile +- 1 surviving records (no pair is dropped, so the counts hold for both
    levels): the prefetch of a tile that does not exist, the clamped load of a tile's tail, a last tile of one record;
  * whole tiles of intra-contig pairs (dropped by the map) between surviving ones, and nothing surviving after the first tile;
  * two keys only: all records in two buckets, every other bucket empty;
  * a third of the fragments outside frag_set (the membership gathers of the packed matrix entries drop entries after a prefetch),
    700 fragments (two levels of the row partition, whose second-level tiles straddle first-level buckets of ~1.7k entries: the
    tile_group mismatch path) and 300 (one level);
  * the 16-byte matrix entries: forced (HHX_D2M_WIDE, read per call) on every stream, and taken by themselves for one link count
    >= 2^24, built as tests/test_gpu_kernels.py::test_link_matrix_packed_and_wide_entries builds it;
  * three pushes of the same stream (the merge partitions table rows).

The group-by takes ONE radix level at these sizes with the default 2048 records a bucket.  HHX_ING_BUCKET is read once per process,
so the same cases run a second time in a fresh child process under HHX_ING_BUCKET=2: 2^13..2^15 buckets, two levels, first-level
buckets of a few hundred records — far smaller than a tile, so almost every second-level tile straddles several of them."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.test_gpu_link_build_paths import CTG_LEN, FLANK, _Stream, _check_matrix, _check_tables, _ingest, _random_pairs, _third_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8192                      # 12-byte records per scatter tile of the group-by's partition (csrc/hhx_partition.h: PartTile, part_scatter_threads)
GRIDS = (1, 2, 3)
EXACT = sorted({TILE, TILE + 1, 2 * TILE - 1} | {g * TILE + d for g in GRIDS for d in (-1, 1)})
CHILD_BUCKET = 2                 # HHX_ING_BUCKET of the child process


def _levels(n_items, per_bucket):
    """(total bits, radix levels) of the group-by's partition of one push (csrc/hhx_ingest.hip: ingest_total_bits; levels of <= 9 bits)"""
    bits = 0
    while (n_items >> bits) > per_bucket and bits < 24:
        bits += 1
    return bits, max(1, -(-bits // 9))


def _inter_pairs(rng, n_ids, count):
    """`count` pairs over the fragments [0, n_ids), none of them intra-contig: every record survives the map"""
    a = rng.integers(0, n_ids, count)
    b = (a + 1 + rng.integers(0, n_ids - 1, count)) % n_ids
    return a.astype(np.int32), rng.integers(0, CTG_LEN, count).astype(np.int32), b.astype(np.int32), rng.integers(0, CTG_LEN, count).astype(np.int32)


def _with_dropped_tiles(rng, n_ids, tiles, dropped):
    a, p1, b, p2 = _inter_pairs(rng, n_ids, tiles * TILE)
    for t in dropped:
        b[t * TILE:(t + 1) * TILE] = a[t * TILE:(t + 1) * TILE]
    return a, p1, b, p2


@functools.lru_cache(maxsize=None)
def _stream(name):
    if name.startswith('exact_'):       # 300 fragments (one level of the row partition); 280 occur
        count = int(name[6:])
        return _Stream(300, _inter_pairs(np.random.default_rng(count), 280, count), 21)
    if name == 'dropped_tiles':         # nine tiles; 1, 2, 4, 6 and 7 hold intra-contig pairs only
        return _Stream(700, _with_dropped_tiles(np.random.default_rng(31), 640, 9, (1, 2, 4, 6, 7)), 22)
    if name == 'first_tile_only':       # nine tiles; nothing survives the map after the first
        return _Stream(700, _with_dropped_tiles(np.random.default_rng(32), 640, 9, range(1, 9)), 23)
    if name == 'two_keys':              # 50k pairs of two fragment pairs: two buckets hold everything
        rng = np.random.default_rng(33)
        which = rng.integers(0, 2, 50_001)
        a = np.array([3, 100], np.int32)[which]
        b = np.array([4, 50], np.int32)[which]
        return _Stream(300, (a, rng.integers(0, CTG_LEN, 50_001).astype(np.int32), b, rng.integers(0, CTG_LEN, 50_001).astype(np.int32)), 24)
    if name == 'general':               # 700 fragments (two levels of the row partition), ~3 % intra-contig pairs scattered through the tiles
        return _Stream(700, _random_pairs(np.random.default_rng(34), 640, 60_003), 25)
    raise KeyError(name)


CASES = [('exact_%d' % c, ()) for c in EXACT] + [('dropped_tiles', ()), ('first_tile_only', ()), ('two_keys', ()), ('general', ()),
                                                  ('general', (20_001, 40_002))]


def _shape_ok(name, cuts, per_bucket, want_levels):
    """the stream is what the case says it is, and the group-by takes the number of radix levels this process is meant to test"""
    s = _stream(name)
    n = len(s.pairs[0])
    alive = s.pairs[0] != s.pairs[2]
    if name.startswith('exact_'):
        assert alive.all() and n == int(name[6:])
    if name == 'dropped_tiles':
        assert [bool(alive[t * TILE:(t + 1) * TILE].any()) for t in range(9)] == [t in (0, 3, 5, 8) for t in range(9)]
    if name == 'first_tile_only':
        assert alive[:TILE].all() and not alive[TILE:].any()
    edges = [0] + list(cuts) + [n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        bits, levels = _levels(hi - lo, per_bucket)
        assert levels == want_levels, '%s: %d records are %d levels' % (name, hi - lo, levels)
        if want_levels == 2:            # first-level buckets far smaller than a tile: second-level tiles straddle them
            assert (hi - lo) >> (bits // 2) < TILE // 4


def _drive(name, cuts, grid):
    """one case at one grid cap: every table and the matrix (whole frag_set, a third out, 8- and 16-byte entries) against the oracle"""
    s = _stream(name)
    what = '%s, %d push(es), HHX_PART_GRID=%d' % (name, len(cuts) + 1, grid)
    os.environ['HHX_PART_GRID'] = str(grid)
    try:
        ing = _ingest(s, cuts)
        try:
            _check_tables(ing, s.ref, what)
            _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), what + ', every fragment in frag_set')
            _check_matrix(ing, s.ref, s.n, _third_out(s.n), what + ', a third out')
            os.environ['HHX_D2M_WIDE'] = '1'
            _check_matrix(ing, s.ref, s.n, _third_out(s.n), what + ', a third out, 16-byte entries')
        finally:
            os.environ.pop('HHX_D2M_WIDE', None)
            ing.destroy()
    finally:
        os.environ.pop('HHX_PART_GRID', None)


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('name,cuts', CASES, ids=['%s-%d' % (n, len(c) + 1) for n, c in CASES])
def test_one_level_group_by(name, cuts, grid):
    assert 'HHX_ING_BUCKET' not in os.environ and 'HHX_ING_LBITS' not in os.environ
    _shape_ok(name, cuts, 2048, 1)
    _drive(name, cuts, grid)


def test_two_level_group_by_in_a_child_process():
    """every case at every grid cap once more, under HHX_ING_BUCKET=2 (read once per process): two radix levels, straddling tiles"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), HHX_ING_BUCKET=str(CHILD_BUCKET))
    env.pop('HHX_ING_LBITS', None)
    p = subprocess.run(['timeout', '-k', '10', '150', sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, 'child failed with status %d:\n%s\n%s' % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    done = json.loads(p.stdout.strip().splitlines()[-1])
    assert done == {'cases': len(CASES) * len(GRIDS), 'failed': []}


@pytest.mark.parametrize('grid', GRIDS)
def test_count_beyond_the_packed_entries(grid, monkeypatch):
    """one fragment pair with 2^24 + 5 links among 20k others: the packed entries give way to the 16-byte ones by themselves"""
    import torch
    from haphic_amd import _lib
    s = _heavy()
    monkeypatch.setenv('HHX_PART_GRID', str(grid))
    dev = [torch.from_numpy(x).to('cuda') for x in s.pairs]
    ing = _lib.Ingest(s.table, FLANK, bins=False, skip_intra=True)
    try:
        ing.push_device(len(s.pairs[0]), *[x.data_ptr() for x in dev])
        torch.cuda.synchronize()
        ing.finalize()
        what = 'a count of 2^24 + 5, HHX_PART_GRID=%d' % grid
        _check_tables(ing, s.ref, what)
        assert s.ref['flank_cnt'].max() == HEAVY
        _check_matrix(ing, s.ref, s.n, _third_out(s.n), what)
    finally:
        ing.destroy()


HEAVY = (1 << 24) + 5


@functools.lru_cache(maxsize=None)
def _heavy():
    rng = np.random.default_rng(35)
    a, p1, b, p2 = _random_pairs(rng, 640, 20_001)
    cat = lambda u, v: np.concatenate([u, np.full(HEAVY, v, np.int32)])
    assert _third_out(700)[3] and _third_out(700)[5]
    return _Stream(700, (cat(a, 3), cat(p1, 10), cat(b, 5), cat(p2, 10)), 26)       # position 10: inside the flanks


def _child():
    failed = []
    for name, cuts in CASES:
        _shape_ok(name, cuts, CHILD_BUCKET, 2)
        for grid in GRIDS:
            try:
                _drive(name, cuts, grid)
            except AssertionError as e:
                failed.append('%s/%d/%d: %s' % (name, len(cuts) + 1, grid, str(e)[:200]))
    print(json.dumps({'cases': len(CASES) * len(GRIDS), 'failed': failed}))
    return 1 if failed else 0


if __name__ == '__main__':
    assert os.environ.get('HHX_ING_BUCKET') == str(CHILD_BUCKET)
    sys.exit(_child())
