"""GPU: the front of `haphic reassign` in the library.
  * hhx_fasta_re_counts (the RE sites counted on the sequences a Fasta handle holds in HBM) against Python's str.count on the same strings and
    against hhx_count_re_sites, the entry that takes the bytes from the host, on the same inputs: the edge genome of
    tests/reassign_front_cases.py (block seams, contig seams, the greedy rule, both letter cases, two site lengths at once, overlapping
    segments) and a 2 MB genome;
  * hhx_fasta_fetch at offset 0, across a block seam, of length 0, to the last byte; a range outside the sequences is refused;
  * Reassign.from_pickle against Reassign on the host arrays of the same file: cells, pair sums and one round equal bit for bit, with the grid
    of the key pass at 1 and 2 workgroups (many steps per lane) and at its default on ~200 000 keys; n_keys = 0; contigs beyond the table's
    names; every refusal with its flag and reason and without a handle."""
from collections import defaultdict

import numpy as np
import pytest

from haphic_amd import _lib, cluster
from tests import build_cases as bc
from tests import link_pickle_cases as lp
from tests import reassign_front_cases as fc

pytestmark = pytest.mark.gpu


def _sites(RE):
    return cluster._sites_of(RE)


def _count(seq, sites):
    return sum(seq.count(s) for s in sites)


@pytest.fixture(scope='module')
def edge():
    text, names, seqs = fc.edge_genome()
    return text, names, seqs


@pytest.mark.parametrize('keep', [False, True], ids=['upper', 'keep_case'])
def test_re_counts_on_the_resident_sequences(edge, keep):
    text, names, seqs = edge
    fa = _lib.Fasta(text, keep_letter_case=keep)
    try:
        assert fa.names() == names and fa.seq_len.tolist() == [len(s) for s in seqs]
        strings = [s if keep else s.upper() for s in seqs]
        genome = b''.join(strings)
        assert genome.endswith(b'GATC') and fa.n_seq_bytes == len(genome) > 20000
        host = fa.sequences()
        # whole contigs, then segments that overlap: a prefix and a suffix of one contig, a window over a block seam, one over two contigs, one
        # that ends in the middle of a site, the whole genome, empty segments at both ends
        k = names.index('three_blocks')
        o, n = int(fa.seq_off[k]), int(fa.seq_len[k])
        extra = [(o, 5000), (o + 3000, n - 3000), (o + 4000, 4), (o + 4001, 3), (4090, 12), (int(fa.seq_off[names.index('left_gatc')]), 204), (0, len(genome)),
                 (0, 0), (len(genome), 0), (len(genome) - 4, 4), (len(genome) - 3, 3)]
        off = np.array(fa.seq_off.tolist() + [a for a, _b in extra], np.int64)
        ln = np.array(fa.seq_len.tolist() + [b for _a, b in extra], np.int64)
        for RE in fc.RES + ('GATC,AAGCTT,GCGC,GANTC', ''):
            sites = _sites(RE)
            want = [_count(genome[a:a + b], sites) for a, b in zip(off.tolist(), ln.tolist())]
            got = fa.re_counts_device(sites, off, ln)
            assert got.tolist() == want, RE
            assert np.array_equal(got, _lib.count_re_sites(host, off, ln, sites)), RE
            whole = fa.re_counts_device(sites)
            assert whole.tolist() == [_count(s, sites) for s in strings] and np.array_equal(whole, fa.re_counts(sites))
        gatc = fa.re_counts_device(_sites('GATC'))
        assert gatc[names.index('short')] == 0 and gatc[names.index('empty')] == 0
        assert _count(strings[names.index('left_gatc')] + strings[names.index('right_gatc')], [b'GATC']) == gatc[names.index('left_gatc')] + gatc[names.index('right_gatc')] + 1
        with pytest.raises(RuntimeError, match='out of range'):
            fa.re_counts_device(_sites('GATC'), [len(genome) - 3], [4])
        with pytest.raises(RuntimeError, match='out of range'):
            fa.re_counts_device(_sites('GATC'), [-1], [4])
    finally:
        fa.close()


def test_re_counts_on_a_2_mb_genome():
    case = bc.genome_case()
    fa = _lib.Fasta(case.fasta)
    try:
        genome = fa.sequences().tobytes()
        for RE in ('GATC,GANTC', 'GCGC'):
            sites = _sites(RE)
            got = fa.re_counts_device(sites)
            assert got.tolist() == [_count(genome[a:a + b], sites) for a, b in zip(fa.seq_off.tolist(), fa.seq_len.tolist())]
            assert np.array_equal(got, fa.re_counts(sites))
    finally:
        fa.close()


def test_fetch_ranges(edge):
    text, _names, seqs = edge
    fa = _lib.Fasta(text)
    try:
        genome = b''.join(seqs).upper()
        n = len(genome)
        for off, ln in ((0, 1), (0, 4095), (4090, 12), (4095, 4098), (7, 0), (0, 0), (n, 0), (n - 1, 1), (n - 5000, 5000), (0, n)):
            assert fa.fetch(off, ln) == genome[off:off + ln], (off, ln)
        for off, ln in ((n, 1), (n - 3, 4), (-1, 2), (0, n + 1), (0, -1), (2 ** 62, 2 ** 62)):
            with pytest.raises(RuntimeError, match='hhx_fasta_fetch'):
                fa.fetch(off, ln)
    finally:
        fa.close()


# ------------------------------------------------------------------ Reassign.from_pickle
def _open(tmp_path, table, library=False):
    path = str(tmp_path / 'full_links.pkl')
    (lp.write_library if library else lp.write_python)(table, path)
    h = _lib.LinkPickle.open(path)
    assert h is not None
    return h


def planted(n_ctg, n_keys, seed, n_groups=7, extra=5):
    """a table of n_keys keys over n_ctg names (a multiple of n_groups; every name in some key), about every third key inside a residue class of the
    contig number -> (defaultdict, names in first-seen order, group [names + extra]: the class for most, none or another for the rest)"""
    rng = np.random.default_rng(seed)
    m = 3 * n_keys
    a = np.concatenate([np.arange(n_ctg), rng.integers(0, n_ctg, m)])
    step = n_groups * rng.integers(1, n_ctg // n_groups, a.size) + np.where(rng.random(a.size) < 0.5, 0, rng.integers(1, n_groups, a.size))
    b = (a + step) % n_ctg
    table = defaultdict(int)
    for x, y, v in zip(a.tolist(), b.tolist(), rng.integers(1, 400, a.size).tolist()):
        if len(table) == n_keys:
            break
        if (y, x) not in table:
            table[('ctg%d' % x, 'ctg%d' % y)] = v
    names = {}
    cluster._dict_arrays(table, names)
    group = np.array([int(c[3:]) % n_groups for c in names] + [-1] * extra, np.int32)
    u = rng.random(group.size)
    group[u < 0.15] = -1
    wrong = (u >= 0.15) & (u < 0.25)
    group[wrong] = rng.integers(0, n_groups, int(wrong.sum()))
    group[-1] = 3
    return table, list(names), group


def same_handles(ours, theirs, group0, n_groups, seed):
    """cells, pair sums and one round of two handles, bit for bit"""
    n_ctg = len(group0)
    for a, b in zip(ours.cells(), theirs.cells()):
        assert np.array_equal(a, b)
    rng = np.random.default_rng(seed)
    member, group_of = (rng.random(n_ctg) < 0.8).astype(np.uint8), rng.integers(-1, 4, n_ctg).astype(np.int32)
    for a, b in zip(ours.pair_sums(member, group_of, 4), theirs.pair_sums(member, group_of, 4)):
        assert np.array_equal(a, b)
    ctg_re = rng.integers(8, 400, n_ctg).astype(np.int64)
    order = rng.permutation(n_ctg).astype(np.int32)
    flags = np.full(n_ctg, 3, np.uint8)
    out = []
    for h in (ours, theirs):
        group = np.array(group0, np.int32)
        group_re = np.ones(n_groups, np.int64)
        np.add.at(group_re, group[group >= 0], ctg_re[group >= 0] - 1)
        counts = h.round(group, group_re, ctg_re, order, flags, None, 1, 0.0001, 1.2, 0.8, False, False, 0)
        out.append((group.tolist(), group_re.tolist(), np.asarray(counts).tolist(), [x.tolist() for x in h.cells()]))
    assert out[0] == out[1] and sum(out[0][2]) == n_ctg and out[0][2][1] > 0 and out[0][2][2] > 0
    return out[0][2]


@pytest.mark.parametrize('grid,library', [(1, False), (1, True), (2, False), (2, True), (None, False)],
                         ids=['grid1-python_dialect', 'grid1-library_dialect', 'grid2-python_dialect', 'grid2-library_dialect', 'default_grid-200k_keys'])
def test_from_pickle_equals_the_handle_from_host_arrays(grid, library, tmp_path):
    n_ctg, n_keys = (903, 200_000) if grid is None else (147, 3000)
    table, names, group = planted(n_ctg, n_keys, 17 + n_keys)
    h = _open(tmp_path, table, library)
    _lib.tune('reassign_check_grid', grid)
    try:
        assert h.n_keys == len(table) == n_keys and h.n_names == len(names) and h.names() == names
        i, j, value, is_float, _names = h.arrays()
        assert is_float is None
        n_all, n_groups = len(group), 7
        ours = _lib.Reassign.from_pickle(h, n_all, group, n_groups)           # contigs beyond the table's names: no key, a group or none
        theirs = _lib.Reassign(i, j, value, n_all, group, n_groups)
        assert ours is not None and (ours.n_ctg, ours.n_groups) == (n_all, n_groups)
        same_handles(ours, theirs, group, n_groups, 5)
        ours.close()
        theirs.close()
    finally:
        _lib.tune('reassign_check_grid', None)
        h.close()


def test_from_pickle_without_a_key(tmp_path):
    h = _open(tmp_path, defaultdict(int))
    try:
        group = np.array([0, -1, 1], np.int32)
        ours = _lib.Reassign.from_pickle(h, 3, group, 2)
        assert h.n_keys == 0 and ours is not None
        sums, first = ours.cells()
        assert not sums.any() and (first == -1).all()
        counts = ours.round(group.copy(), np.ones(2, np.int64), np.ones(3, np.int64), np.arange(3, dtype=np.int32), np.ones(3, np.uint8), None, 1, 0.0001,
                            1.2, 0.8, False, False, 0)
        assert counts.tolist() == [0, 0, 0, 3]
        ours.close()
        with pytest.raises(ValueError):
            _lib.Reassign.from_pickle(h, 3, group[:2], 2)
    finally:
        h.close()


BASE = {('a', 'b'): 5, ('b', 'c'): 7, ('a', 'd'): 2, ('e', 'c'): 1}
R = _lib.Reassign
REFUSED = [('self_key', {('c', 'c'): 3}, R.REFUSED_SELF_KEY, 'names one contig twice'), ('negative', {('d', 'e'): -4}, R.REFUSED_NEGATIVE, 'negative'),
           ('most_negative', {('d', 'e'): -2 ** 63}, R.REFUSED_NEGATIVE, 'negative'), ('float', {('d', 'e'): 0.5}, R.REFUSED_FLOAT, 'float'),
           ('total_2_52', {('d', 'e'): 2 ** 52 - 15}, R.REFUSED_TOTAL, '2^53'),
           ('total_beyond_2_64', {('d', 'e'): 2 ** 62, ('a', 'e'): 2 ** 62, ('b', 'e'): 2 ** 62, ('b', 'd'): 2 ** 62}, R.REFUSED_TOTAL, '2^53'),
           ('largest_values', {('d', 'e'): 2 ** 63 - 1, ('a', 'e'): 2 ** 63 - 1, ('b', 'e'): 2}, R.REFUSED_TOTAL, '2^53'),
           ('several', {('c', 'c'): -3, ('d', 'e'): 2 ** 61}, R.REFUSED_SELF_KEY | R.REFUSED_NEGATIVE | R.REFUSED_TOTAL, 'negative')]


@pytest.mark.parametrize('name,extra,flags,reason', REFUSED, ids=[r[0] for r in REFUSED])
def test_from_pickle_refusals(name, extra, flags, reason, tmp_path):
    h = _open(tmp_path, defaultdict(int, {**BASE, **extra}))
    try:
        before = len(R.REFUSALS)
        assert _lib.Reassign.from_pickle(h, 6, np.array([0, 0, 1, -1, 1, 0], np.int32), 2) is None
        assert len(R.REFUSALS) == before + 1 and R.REFUSALS[-1][0] == flags and reason in R.REFUSALS[-1][1]
    finally:
        h.close()


def test_from_pickle_serves_the_total_below_2_52(tmp_path):
    h = _open(tmp_path, defaultdict(int, {**BASE, ('d', 'e'): 2 ** 52 - 16}))
    try:
        i, j, value, _f, _n = h.arrays()
        group = np.array([0, 0, 1, -1, 1, 0], np.int32)
        ours, theirs = _lib.Reassign.from_pickle(h, 6, group, 2), _lib.Reassign(i, j, value, 6, group, 2)
        assert ours is not None
        for a, b in zip(ours.cells(), theirs.cells()):
            assert np.array_equal(a, b)
        ours.close()
        theirs.close()
    finally:
        h.close()
