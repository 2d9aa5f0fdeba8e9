"""output_statistics :2279-2478 on the device (haphic_amd/csrc/hhx_groupstats.hip, haphic_amd/statistics.py) on the GPU:
  * hhx_group_stats against the numpy engine of tests/statistics_cases.py, exact equality on every output, under the default LDS table and under
    one of 64 slots (every contig with more than 64 distinct groups then takes the table in HBM);
  * the cases of tests/golden/statistics.npz (the reference's own files) through the mirror on a real ingest handle, nothing thawed or fetched;
  * hhx_ingest_group_stats after hhx_ingest_drop_links, against the numpy engine on the surviving keys."""
import types

import numpy as np
import pytest

from tests import statistics_cases as sc
from tests.test_statistics_cpu import CASES, check_files, golden, golden_case   # noqa: F401 (golden: fixture)

pytestmark = pytest.mark.gpu

SLOTS = [None, 64]


@pytest.fixture(params=SLOTS, ids=['default_slots', '64_slots'])
def slots(request):
    from haphic_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_reset()
    if request.param is None:
        _lib.tune('groupstats_lds_slots', None)
    else:
        _lib.tune('groupstats_lds_slots', 64)
    yield request.param
    _lib.tune('groupstats_lds_slots', None)
    _lib.profile_enable(False)


def same(got, want, what=''):
    assert got is not None, what
    for name, g, w in zip(('n_cells', 'max_links', 'max_group', 'other_sum'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if name == 'other_sum':
            g, w = g.view(np.uint64), w.view(np.uint64)            # the same doubles, bit for bit
        bad = np.argwhere(g != w)
        assert not len(bad), (what, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def both(args, what='', modes=(0, 1)):
    from haphic_amd import _lib
    for mode in modes:
        same(_lib.group_stats(*args, sum_mode=mode), sc.group_stats(*args, sum_mode=mode), '{} mode {}'.format(what, mode))


def spilled():
    from haphic_amd import _lib
    return _lib.profile_counter('groupstats_spilled')


@pytest.mark.parametrize('name', list(CASES))
def test_hand_built_traps_and_families(slots, name):
    case = CASES[name]
    both((case.fi, case.fj, case.cnt) + case.engine_args(), name)


def test_row_lengths_around_the_workgroup_and_table_sizes(slots):
    for row_len in (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097):
        both(sc.star(row_len, 37, seed=row_len), 'row of {}'.format(row_len))
        both(sc.star(row_len, max(row_len, 1), seed=row_len + 1, extra=50 if row_len > 60 else 0), 'row of {} in as many groups'.format(row_len), modes=(0,))
    assert spilled() > 0                                           # 4097 partners in 4097 groups fit no LDS table


def test_hub_of_5000_contigs_in_300_groups(slots):
    both(sc.star(5000, 300, seed=1, extra=3000), 'hub')
    assert (spilled() > 0) == (slots == 64)


def test_3000_singleton_groups_exceed_every_lds_table(slots):
    args = sc.star(3000, 3000, seed=2)
    assert sc.group_stats(*args)[0][0, 0] == 3000
    both(args, 'singletons')
    assert spilled() > 0


def test_counts_up_to_2_to_the_40(slots):
    args = sc.random_case(300, 6000, [7, 90], seed=3, max_count=2 ** 40)
    assert sc.group_stats(*args)[1].max() > 2 ** 42
    both(args, 'wide counts')


def test_three_sets_with_their_own_offsets(slots):
    fi, fj, cnt, group, n_groups, group_re, ctg_re = sc.random_case(4000, 40000, [2, 37, 3000], seed=4)
    both((fi, fj, cnt, group, n_groups, group_re, ctg_re), 'three sets')
    # every set alone gives its slice of the joint call
    from haphic_amd import _lib
    joint = _lib.group_stats(fi, fj, cnt, group, n_groups, group_re, ctg_re)
    off = np.concatenate(([0], np.cumsum(n_groups)))
    for s in range(3):
        alone = _lib.group_stats(fi, fj, cnt, group[s:s + 1], n_groups[s:s + 1], group_re[off[s]:off[s + 1]], ctg_re)
        same(alone, [a[s:s + 1] for a in joint], 'set {} alone'.format(s))


def test_zero_keys(slots):
    none = np.zeros(0, np.int32)
    group = np.array([[0, 1, -1, 1], [0, 0, 0, 0]], np.int32)
    both((none, none, np.zeros(0, np.int64), group, np.array([2, 1], np.int32), np.array([5, 6, 7], np.int64), np.ones(4, np.int64)), 'zero keys')


def test_seeded_random_case(slots):
    both(sc.random_case(2000, 60000, [5, 50, 400, 1500], seed=5), 'random')


def test_what_the_library_refuses():
    from haphic_amd import _lib
    fi, fj, cnt, group, n_groups, group_re, ctg_re = sc.star(10, 3, seed=6)
    assert _lib.group_stats(fi, fj, cnt, group, n_groups, group_re, ctg_re, sum_mode=2) is None            # HHX_UNSUPPORTED
    assert b'sum_mode' in _lib.load().hhx_last_error()
    bad = group.copy()
    bad[0, 3] = 3                                                  # a group id beyond n_groups: an error, not an out-of-bounds access
    with pytest.raises(RuntimeError, match='group id'):
        _lib.group_stats(fi, fj, cnt, bad, n_groups, group_re, ctg_re)
    with pytest.raises(RuntimeError, match='contig id'):
        _lib.group_stats(fi, fj + 100, cnt, group, n_groups, group_re, ctg_re)


# ------------------------------------------------------------------ on a real ingest handle
def _handle(case, seed=0):
    """the keys of the case as read pairs: the first pair of every key in dict order, the rest shuffled, the two ends swapped at random"""
    from haphic_amd import _lib, cluster
    n = case.n_ctg
    table = cluster.FragTable.for_contigs(np.arange(n, dtype=np.int32), case.lengths, np.ones(n, np.uint8), case.names)
    rng = np.random.default_rng(seed)
    rest = np.repeat(np.arange(len(case.fi)), case.cnt - 1)
    order = np.concatenate((np.arange(len(case.fi)), rng.permutation(rest)))
    a, b = case.fi[order], case.fj[order]
    swap = rng.random(len(order)) < 0.5
    id1, id2 = np.where(swap, b, a).astype(np.int32), np.where(swap, a, b).astype(np.int32)
    pos = np.full(len(order), 10, np.int32)
    dev = _lib.Ingest(table, 0, bins=False, skip_intra=True)
    half = len(order) // 2
    dev.push(id1[:half], pos[:half], id2[:half], pos[:half])
    dev.push(id1[half:], pos[half:], id2[half:], pos[half:])
    dev.finalize()
    return table, dev


def _session(table, dev):
    from haphic_amd import cluster, containers
    args = types.SimpleNamespace(remove_allelic_links=0, remove_concentrated_links=False, max_read_pairs=0, nwindows=50)
    session = cluster.IngestSession(dev, table, None, args, 'int32', 'int32')
    return session, containers.LinkTable(session, 'full')


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.handle])
def test_fixture_cases_through_the_mirror_on_a_real_handle(golden, name, tmp_path, monkeypatch, slots):   # noqa: F811
    import sys
    from haphic_amd import _lib, containers, statistics
    case = golden_case(golden, name)
    monkeypatch.setattr(containers, 'THAW_LOG', [])
    monkeypatch.setattr(statistics, 'SUM_MODE', int(golden['sum_mode']))
    monkeypatch.setitem(sys.modules, 'matplotlib', None)           # the text files are the subject; the drawing has a CPU test
    table, dev = _handle(case)
    try:
        session, full = _session(table, dev)
        assert len(full) == len(case.fi)
        monkeypatch.chdir(tmp_path)
        for label, _clusters in case.sets:
            (tmp_path / 'inflation_{}'.format(label)).mkdir()
        statistics.output_statistics(case.fa_dict(), full, case.result_clusters_list())        # no _original: the device path or an error
        check_files(golden, case)
        assert full.frozen and not containers.THAW_LOG and not session._host, 'nothing thawed, nothing of the table fetched'
        assert statistics.STATS['engine'] == 'device' and isinstance(session.ing, _lib.Ingest)
    finally:
        dev.destroy()


@pytest.mark.parametrize('name', ['ties', 'magnitude'])
def test_handle_after_drop_links_against_the_surviving_keys(name, slots):
    case = CASES[name]
    table, dev = _handle(case, seed=1)
    try:
        got = dev.fetch(want=['full_i', 'full_j', 'full_cnt'])
        assert np.array_equal(got['full_i'], case.fi) and np.array_equal(got['full_j'], case.fj) and np.array_equal(got['full_cnt'], case.cnt)
        args = case.engine_args()
        same(dev.group_stats(*args), sc.group_stats(case.fi, case.fj, case.cnt, *args), 'before the drop')
        drop = (np.random.default_rng(9).random(len(case.fi)) < 0.4).astype(np.uint8)
        drop[[0, -1]] = 1
        assert dev.drop_links(drop, np.ones(table.n_frag, np.uint8)) is not None
        keep = drop == 0
        assert dev.n_full == int(keep.sum())
        for mode in (0, 1):
            same(dev.group_stats(*args, sum_mode=mode), sc.group_stats(case.fi[keep], case.fj[keep], case.cnt[keep], *args, sum_mode=mode),
                 'after the drop, mode {}'.format(mode))
    finally:
        dev.destroy()
