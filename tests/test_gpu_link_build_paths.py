"""Every path of the link-matrix build (Ingest.push_device -> finalize -> link_matrix) against the oracle, bit for bit, at the
smallest shapes that reach it: the full and flank tables (keys, counts, insertion order), n_linked, frag_index and the CSR triple.

  700 fragments (> 2^9: both radix levels of the row partition) and 40 (one level); 4k + 1 and 4k + 3 pairs (the map kernel's
  bulk / tail split); a push of 0 pairs; a stream of intra-contig pairs only (no record survives the map); keys none of which
  has both ends in frag_set (the row partition ends with n_valid == 0); a third of the fragments outside frag_set and members
  without a link (trailing indices, k_rest_rows), with and without self loops, n_rest given and derived; 200k pairs with a few
  heavy keys, so that group-by buckets hold 1025..2048 records (k_aggregate's two sub-passes) and far more (sixteen); a hub row
  of more than EMIT_T * EMIT_R = 4096 entries among 5000 fragments (the emit kernel's tail loop, the sort-ranked index
  assignment); one, two and three pushes of the same stream (the merge of pushed runs).
  A count >= 2^24 (the packed path's fall-back to 16-byte entries) takes 17 M pairs of one key: it stays with
  tests/test_gpu_kernels.py::test_link_matrix_packed_and_wide_entries.

The streams are built on the host from a seed, the oracle's tables are computed once per stream and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc

TABLES = ('full_i', 'full_j', 'full_cnt', 'ht_cnt', 'flank_i', 'flank_j', 'flank_cnt', 'frag_links')
CTG_LEN, FLANK = 10_000, 3_000          # a coordinate is in a flank with probability 0.6: about a third of the keys never enter flank_link_dict


def _table(n, seed):
    rank = np.random.default_rng(seed).permutation(n).astype(np.int32)        # names in no particular order: both key orientations occur
    length = np.full(n, CTG_LEN, np.int64)
    return orc.FragTable(rank, length, np.arange(n, dtype=np.int32), np.zeros(n, np.uint8), 0, rank, length, np.ones(n, np.uint8))


def _random_pairs(rng, n_ids, count):
    """`count` pairs over the fragments [0, n_ids), about 3 % of them intra-contig (dropped by skip_intra)"""
    a = rng.integers(0, n_ids, count).astype(np.int32)
    b = rng.integers(0, n_ids, count).astype(np.int32)
    same = rng.random(count) < 0.03
    b[same] = a[same]
    return a, rng.integers(0, CTG_LEN, count).astype(np.int32), b, rng.integers(0, CTG_LEN, count).astype(np.int32)


def _mix64(x):
    """the group-by's bucket hash (csrc/hhx_ingest.hip: mix64) on uint64 arrays"""
    x = x.astype(np.uint64)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def _bucket_sizes(table, id1, id2):
    """records per group-by bucket of ONE push of this stream (csrc/hhx_ingest.hip: ingest_total_bits, bucket_of, the key orientation of the map)"""
    total_bits = 0
    while (len(id1) >> total_bits) > 2048 and total_bits < 24:
        total_bits += 1
    keep = id1 != id2
    a, b = id1[keep].astype(np.int64), id2[keep].astype(np.int64)
    swap = table.ctg_rank[a] > table.ctg_rank[b]
    i, j = np.where(swap, b, a), np.where(swap, a, b)
    key = (i.astype(np.uint64) << np.uint64(29)) | j.astype(np.uint64)
    assert total_bits > 0
    return np.bincount((_mix64(key) >> np.uint64(64 - total_bits)).astype(np.int64), minlength=1 << total_bits)


class _Stream:
    def __init__(self, n, pairs, seed):
        self.n = n
        self.table = _table(n, seed)
        self.pairs = [np.ascontiguousarray(x) for x in pairs]
        self._ref = None

    @property
    def ref(self):
        """the oracle's tables, computed once"""
        if self._ref is None:
            h = self.pairs
            keep = h[0] != h[2]                                   # pairs_generator_inter_ctgs :1582
            self._ref = orc.ingest(self.table, h[0][keep], h[1][keep].astype(np.int64), h[2][keep], h[3][keep].astype(np.int64), FLANK)
        return self._ref


@functools.lru_cache(maxsize=None)
def _stream(name):
    if name == 'two_levels':            # 700 fragments, 4k + 1 pairs; the last 60 fragments never occur in a pair
        return _Stream(700, _random_pairs(np.random.default_rng(11), 640, 20_001), 1)
    if name == 'one_level':             # 40 fragments, 4k + 3 pairs; the last 5 never occur
        return _Stream(40, _random_pairs(np.random.default_rng(12), 35, 4_003), 2)
    if name == 'intra_only':
        a, p1, _b, p2 = _random_pairs(np.random.default_rng(13), 700, 5_001)
        return _Stream(700, (a, p1, a.copy(), p2), 3)
    if name == 'even_odd':              # every pair joins an even and an odd fragment
        rng = np.random.default_rng(14)
        a = (2 * rng.integers(0, 350, 6_003)).astype(np.int32)
        b = (2 * rng.integers(0, 350, 6_003) + 1).astype(np.int32)
        flip = rng.random(6_003) < 0.5
        a, b = np.where(flip, b, a).astype(np.int32), np.where(flip, a, b).astype(np.int32)
        return _Stream(700, (a, rng.integers(0, CTG_LEN, 6_003).astype(np.int32), b, rng.integers(0, CTG_LEN, 6_003).astype(np.int32)), 4)
    if name == 'heavy_keys':            # 200k pairs: four fragment pairs carry 10k pairs each, the rest is spread over 700 fragments
        rng = np.random.default_rng(15)
        a, p1, b, p2 = _random_pairs(rng, 700, 200_000)
        heavy = rng.choice(200_000, 40_000, replace=False)
        which = rng.integers(0, 4, 40_000)
        a[heavy] = np.array([3, 100, 250, 699], np.int32)[which]
        b[heavy] = np.array([4, 50, 251, 0], np.int32)[which]
        return _Stream(700, (a, p1, b, p2), 5)
    if name == 'hub':                   # 5000 fragments; fragment 6 is linked to 4600 others, inside the flanks
        rng = np.random.default_rng(16)
        a, p1, b, p2 = _random_pairs(rng, 5000, 12_001)
        others = rng.permutation(np.setdiff1d(np.arange(5000), [6]))[:4600].astype(np.int32)
        hub = np.full(4600, 6, np.int32)
        first = rng.random(4600) < 0.5
        ha, hb = np.where(first, hub, others).astype(np.int32), np.where(first, others, hub).astype(np.int32)
        order = rng.permutation(12_001 + 4600)
        cat = lambda u, v: np.concatenate([u, v])[order]
        return _Stream(5000, (cat(a, ha), cat(p1, np.full(4600, 10, np.int32)), cat(b, hb), cat(p2, np.full(4600, 9_990, np.int32))), 6)
    raise KeyError(name)


def _ingest(s, cuts=()):
    """the stream pushed from device memory in len(cuts) + 1 batches; finalized"""
    import torch
    from haphic_amd import _lib
    dev = [torch.from_numpy(x).to('cuda') for x in s.pairs]
    ing = _lib.Ingest(s.table, FLANK, bins=False, skip_intra=True)
    edges = [0] + list(cuts) + [len(s.pairs[0])]
    for lo, hi in zip(edges[:-1], edges[1:]):
        ing.push_device(hi - lo, *[x[lo:hi].data_ptr() for x in dev])
    torch.cuda.synchronize()
    ing.finalize()
    return ing


def _check_tables(ing, ref, what):
    got = ing.fetch()
    for k in TABLES:
        assert np.array_equal(got[k], ref[k]), '%s: table %s' % (what, k)


def _check_matrix(ing, ref, n, in_set, what, self_loops=True, give_n_rest=False):
    in_set = np.ascontiguousarray(in_set, np.uint8)
    ok = in_set[ref['flank_i']].astype(bool) & in_set[ref['flank_j']].astype(bool)
    linked = np.zeros(n, bool)
    linked[ref['flank_i'][ok]] = True
    linked[ref['flank_j'][ok]] = True
    n_rest = int(in_set.sum() - linked.sum())
    rp, rj, rx, ridx, rl = orc.dict_to_matrix(ref['flank_i'], ref['flank_j'], ref['flank_cnt'].astype(np.float64), n, in_set, n_rest,
                                             add_self_loops=self_loops)
    m, fidx, n_linked = ing.link_matrix(in_set, n_rest if give_n_rest else -1, add_self_loops=self_loops)
    try:
        assert n_linked == rl == int(linked.sum()), '%s: n_linked' % what
        assert np.array_equal(fidx, ridx), '%s: frag_index' % what
        assert m.shape3[0] == rl + n_rest, '%s: matrix order' % what
        gp, gj, gx = m.to_arrays()
        assert np.array_equal(gp, rp), '%s: indptr' % what
        assert np.array_equal(gj, rj), '%s: indices' % what
        assert np.array_equal(gx, rx), '%s: data' % what
    finally:
        m.free()
    return n_rest, rl


def _third_out(n):
    return (np.arange(n) % 3 != 1).astype(np.uint8)


@pytest.mark.parametrize('name,pairs_mod4', [('two_levels', 1), ('one_level', 3)])
def test_both_partition_depths_and_the_map_tail(name, pairs_mod4):
    s = _stream(name)
    assert len(s.pairs[0]) % 4 == pairs_mod4
    assert (s.n > 512) == (name == 'two_levels')
    ing = _ingest(s)
    try:
        _check_tables(ing, s.ref, name)
        assert 0 < len(s.ref['flank_i']) < len(s.ref['full_i'])                # keys that never entered flank_link_dict are in the run
        _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), name + ', every fragment in frag_set')
    finally:
        ing.destroy()


@pytest.mark.parametrize('name', ['two_levels', 'one_level'])
@pytest.mark.parametrize('self_loops', [True, False])
def test_frag_set_with_a_third_out_and_link_less_members(name, self_loops):
    s = _stream(name)
    in_set = _third_out(s.n)
    ing = _ingest(s)
    try:
        for give in (False, True):
            n_rest, n_linked = _check_matrix(ing, s.ref, s.n, in_set, '%s, a third out, self loops %s, n_rest %s' % (
                name, self_loops, 'given' if give else 'derived'), self_loops=self_loops, give_n_rest=give)
            assert n_rest > 0 and n_linked > 0                                 # members without a link follow the linked ones
    finally:
        ing.destroy()


def test_push_of_no_pairs():
    import torch
    from haphic_amd import _lib
    s = _stream('one_level')
    dev = [torch.from_numpy(x).to('cuda') for x in s.pairs]
    empty = orc.ingest(s.table, *[np.zeros(0, t) for t in (np.int32, np.int64, np.int32, np.int64)], FLANK)
    ing = _lib.Ingest(s.table, FLANK, bins=False, skip_intra=True)
    try:
        ing.push_device(0, *[x.data_ptr() for x in dev])
        assert ing.finalize() == (0, 0)
        _check_tables(ing, empty, 'nothing pushed')
        n_rest, n_linked = _check_matrix(ing, empty, s.n, _third_out(s.n), 'nothing pushed')
        assert (n_rest, n_linked) == (int(_third_out(s.n).sum()), 0)
    finally:
        ing.destroy()
    # ... and an empty push between two real ones changes nothing
    ing = _lib.Ingest(s.table, FLANK, bins=False, skip_intra=True)
    try:
        cut = 1_001
        ing.push_device(cut, *[x.data_ptr() for x in dev])
        ing.push_device(0, *[x.data_ptr() for x in dev])
        ing.push_device(len(s.pairs[0]) - cut, *[x[cut:].data_ptr() for x in dev])
        torch.cuda.synchronize()
        ing.finalize()
        _check_tables(ing, s.ref, 'an empty push between two')
        _check_matrix(ing, s.ref, s.n, _third_out(s.n), 'an empty push between two')
    finally:
        ing.destroy()


def test_stream_without_a_surviving_record():
    s = _stream('intra_only')
    assert len(s.ref['full_i']) == 0
    ing = _ingest(s)
    try:
        assert ing.finalize() == (0, 0)
        _check_tables(ing, s.ref, 'intra-contig pairs only')
        for self_loops in (True, False):
            n_rest, n_linked = _check_matrix(ing, s.ref, s.n, _third_out(s.n), 'intra-contig pairs only', self_loops=self_loops)
            assert n_linked == 0 and n_rest > 0
    finally:
        ing.destroy()


def test_no_key_with_both_ends_in_frag_set():
    s = _stream('even_odd')
    assert len(s.ref['flank_i']) > 1000 and ((s.ref['flank_i'] + s.ref['flank_j']) % 2 == 1).all()
    evens = (np.arange(s.n) % 2 == 0).astype(np.uint8)
    ing = _ingest(s)
    try:
        _check_tables(ing, s.ref, 'even-odd keys')
        for self_loops in (True, False):
            n_rest, n_linked = _check_matrix(ing, s.ref, s.n, evens, 'even-odd keys, the even fragments in frag_set', self_loops=self_loops)
            assert (n_rest, n_linked) == (350, 0)                              # the row partition kept no entry
        _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), 'even-odd keys, every fragment in frag_set')
    finally:
        ing.destroy()


def test_group_by_buckets_of_two_and_more_sub_passes():
    s = _stream('heavy_keys')
    sizes = _bucket_sizes(s.table, s.pairs[0], s.pairs[2])
    assert ((sizes > 1024) & (sizes <= 2048)).any(), 'no bucket of 1025..2048 records: k_aggregate\'s two sub-passes are not reached'
    assert (sizes > 8192).any(), 'no bucket of a heavy key'
    ing = _ingest(s)
    try:
        _check_tables(ing, s.ref, 'heavy keys')
        assert s.ref['full_cnt'].max() >= 9_000
        _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), 'heavy keys')
        _check_matrix(ing, s.ref, s.n, _third_out(s.n), 'heavy keys, a third out')
    finally:
        ing.destroy()


def test_row_longer_than_the_emit_registers():
    s = _stream('hub')
    ing = _ingest(s)
    try:
        _check_tables(ing, s.ref, 'hub')
        hub_keys = int(((s.ref['flank_i'] == 6) | (s.ref['flank_j'] == 6)).sum())
        assert hub_keys > 4096, 'the hub row holds %d entries' % hub_keys
        for self_loops in (True, False):
            _check_matrix(ing, s.ref, s.n, np.ones(s.n, np.uint8), 'hub, self loops %s' % self_loops, self_loops=self_loops)
        in_set = _third_out(s.n)
        assert in_set[6]
        _check_matrix(ing, s.ref, s.n, in_set, 'hub, a third out')
    finally:
        ing.destroy()


@pytest.mark.parametrize('name', ['two_levels', 'hub'])
@pytest.mark.parametrize('cuts', [(), (7_003,), (1, 9_998)], ids=['one_push', 'two_pushes', 'three_pushes'])
def test_pushes_of_the_same_stream(name, cuts):
    s = _stream(name)
    ing = _ingest(s, cuts)
    try:
        _check_tables(ing, s.ref, '%s in %d pushes' % (name, len(cuts) + 1))
        _check_matrix(ing, s.ref, s.n, _third_out(s.n), '%s in %d pushes' % (name, len(cuts) + 1))
    finally:
        ing.destroy()
