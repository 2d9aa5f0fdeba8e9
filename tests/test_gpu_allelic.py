"""--remove_allelic_links on the device tables (haphic_amd/csrc/hhx_allelic.hip, haphic_amd/allelic.py) on the GPU:
  * hhx_ingest_concordance against the numpy engine of tests/allelic_cases.py (the C oracle's coordinate lists + numpy modal counts) on hand-built
    keys: every m around the thresholds, the first max_read_pairs pairs in stream order across pushes, flooring, w = 1, 64-bit sums;
  * hhx_ingest_drop_links in both table layouts against the same drops on host copies, through every consumer of the tables;
  * the cases of tests/golden/allelic.npz (the reference's own verdicts) and tests/golden/pipeline_c4.npz through the mirror with the real engine."""
import pickle
import types

import numpy as np
import pytest

from tests import allelic_cases
from tests.test_allelic_cases_cpu import CASES, c4, c4_check, c4_run, check_verdict, frozen_groups, golden   # noqa: F401 (c4, golden: fixtures)

pytestmark = pytest.mark.gpu

MIN_RP = 20


def _table(lengths):
    from haphic_amd import cluster
    n = len(lengths)
    names = ['ctg%04d' % ((k * 7919) % 10007) for k in range(n)]            # name order != id order: both orientations of a key occur
    order = sorted(range(n), key=names.__getitem__)
    rank = np.empty(n, np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    return cluster.FragTable.for_contigs(rank, np.asarray(lengths, np.int64), np.ones(n, np.uint8), names)


def _both(table, stream, cuts, bins=False, flank=0, wide=None):
    """the stream through the library and through the numpy engine, pushed in the same pieces"""
    from haphic_amd import _lib
    dev = _lib.Ingest(table, flank, bins=bins, skip_intra=not bins)
    ref = allelic_cases.Ingest(table, flank, bins=bins, skip_intra=not bins)
    for e in (dev, ref):
        e.keep_pairs()
    bounds = [0] + list(cuts) + [len(stream[0])]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        dev.push(*[a[lo:hi] for a in stream], wide=wide)
        ref.push(*[a[lo:hi] for a in stream])
    dev.finalize()
    ref.finalize()
    return dev, ref


def _interleave(rng, per_key):
    """per_key: list of (ctg_a, ctg_b, [(pos_a, pos_b), ...]) with the pairs of a key in the order they must arrive; returns a stream in which
    the keys are interleaved at random, every key keeps its own order, and the two ends are swapped at random"""
    n = sum(len(p) for _a, _b, p in per_key)
    slots = rng.permutation(n)
    id1, p1, id2, p2 = (np.zeros(n, np.int64) for _ in range(4))
    at = 0
    for a, b, pairs in per_key:
        mine = np.sort(slots[at:at + len(pairs)])
        at += len(pairs)
        xy = np.asarray(pairs, np.int64).reshape(-1, 2)
        id1[mine], p1[mine], id2[mine], p2[mine] = a, xy[:, 0], b, xy[:, 1]
    swap = rng.random(n) < 0.5
    return (np.where(swap, id2, id1).astype(np.int32), np.where(swap, p2, p1), np.where(swap, id1, id2).astype(np.int32), np.where(swap, p1, p2))


def _same_counts(dev, ref, max_rp, nwindows=50, min_rp=MIN_RP):
    got, want = dev.concordance_counts(max_rp, nwindows, min_rp), ref.concordance_counts(max_rp, nwindows, min_rp)
    assert np.array_equal(dev.fetch(want=['full_i'])['full_i'], ref.fetch()['full_i'])
    for name, a, b in zip(('m', 'diag', 'anti'), got, want):
        assert a.dtype == np.int32 and np.array_equal(a, b), (name, max_rp, np.flatnonzero(a != b)[:10], a[a != b][:10], b[a != b][:10])
    return got


@pytest.mark.parametrize('max_rp', [2, 40, 200, 257, 1024])
def test_concordance_counts_on_hand_built_keys(max_rp):
    rng = np.random.default_rng(max_rp)
    L, w = 100_000, 2000
    counts = sorted({1, MIN_RP - 1, MIN_RP, 63, 64, 65, max(max_rp - 1, 1), max_rp, max_rp + 7, 3 * max_rp, 255, 256, 257})
    per_key, expect = [], {}
    k = 0

    def add(pairs, want=None):
        nonlocal k
        per_key.append((2 * k, 2 * k + 1, pairs))
        if want is not None:
            expect[(2 * k, 2 * k + 1)] = want
        k += 1
    for c in counts:
        add([(int(rng.integers(0, L)), int(rng.integers(0, L))) for _ in range(c)])                  # anything, y - x negative half of the time
        add([(5000, 5000 + 37)] * c, want=(min(c, max_rp),) * 2)                                      # all values equal
        add([(t * w // 2 % 40_000, (t * w // 2 % 40_000) + (t % 20) * w + 7) for t in range(c)])       # spread diagonals
        # the first max_read_pairs pairs sit on one diagonal, everything after them on another, and there is more of it
        add([(1000 + t, 1000 + t) for t in range(max_rp)] + [(100, 90_000)] * (2 * max_rp + c), want=(max_rp, None))
    # y - x = -1500 and +1500: windows -1 and 0 under floor division, both 0 under truncation
    add([(30_000, 28_500)] * 30 + [(30_000, 31_500)] * 30)
    # a tie between two modes, and all windows distinct
    add([(10, 10)] * 25 + [(10, 10 + 5 * w)] * 25)
    add([(0, t * w) for t in range(45)])
    table = _table([L] * (2 * k))
    stream = _interleave(rng, per_key)
    n = len(stream[0])
    dev, ref = _both(table, stream, [n // 3, n // 3 + 1, 2 * n // 3])
    m, diag, anti = _same_counts(dev, ref, max_rp)
    # spot checks that do not go through the numpy engine
    o = dev.fetch(want=['full_i', 'full_j'])
    row = {(int(min(a, b)), int(max(a, b))): r for r, (a, b) in enumerate(zip(o['full_i'], o['full_j']))}
    for key, (want_diag, want_anti) in expect.items():
        r = row[key]
        if m[r] < min(MIN_RP, max_rp):
            assert (diag[r], anti[r]) == (0, 0)
            continue
        assert diag[r] == want_diag and (want_anti is None or anti[r] == want_anti), (key, m[r], diag[r], anti[r])
    r = row[(2 * (k - 3), 2 * (k - 3) + 1)]
    assert (m[r], diag[r]) == (min(60, max_rp), 30 if max_rp >= 60 else min(30, max_rp))
    if max_rp >= 50:
        r = row[(2 * (k - 2), 2 * (k - 2) + 1)]
        assert (m[r], diag[r]) == (50, 25)
        r = row[(2 * (k - 1), 2 * (k - 1) + 1)]
        assert (m[r], diag[r]) == (45, 1)
    for e in (dev, ref):
        e.destroy()


def test_concordance_counts_window_of_one_base():
    """contigs of exactly nwindows bp: w = 1, every coordinate difference is its own window"""
    rng = np.random.default_rng(3)
    per_key = [(2 * k, 2 * k + 1, [(int(rng.integers(0, 50)), int(rng.integers(0, 50))) for _ in range(c)]) for k, c in enumerate((20, 33, 64, 200, 300))]
    table = _table([50] * 10)
    stream = _interleave(rng, per_key)
    dev, ref = _both(table, stream, [100])
    m, diag, anti = _same_counts(dev, ref, 257)
    assert sorted(m.tolist()) == [20, 33, 64, 200, 257]
    # shorter than nwindows: the window is 0 wide and the library hands the call back
    assert dev.concordance_counts(257, 51, MIN_RP) is None and ref.concordance_counts(257, 51, MIN_RP) is None
    assert dev.concordance_counts(allelic_cases.CAP + 1, 50, MIN_RP) is None
    m2, _d, _a = _same_counts(dev, ref, allelic_cases.CAP)                               # the cap itself is served
    assert sorted(m2.tolist()) == [20, 33, 64, 200, 300]


@pytest.mark.parametrize('top,wide', [(2 ** 31 - 1, False), (2 ** 32 - 8, True)])
def test_concordance_counts_sums_beyond_32_bits(top, wide):
    """coordinates at the end of contigs of 2^31 - 1 bp (int32 stream) and 2^32 - 8 bp (the 64-bit push): y + x needs 33 / 34 bits"""
    rng = np.random.default_rng(9)
    hi = top - 3                                                   # largest 0-based position used
    far = 2 ** 31 if wide else 2 ** 30                             # 64-bit push: the two sums differ by exactly 2^32
    per_key = [
        (0, 1, [(hi - int(rng.integers(0, 1000)), hi - int(rng.integers(0, 1000))) for _ in range(40)]),
        # two groups on one diagonal whose sums lie 2 * far apart: 50 windows between them (one window if 2^32 were lost)
        (2, 3, [(hi, hi)] * 25 + [(hi - far, hi - far)] * 30),
        (4, 5, [(int(rng.integers(0, top)), int(rng.integers(0, top))) for _ in range(100)]),
    ]
    table = _table([top] * 6)
    stream = _interleave(rng, per_key)
    dev, ref = _both(table, stream, [50], wide=True if wide else None)
    m, diag, anti = _same_counts(dev, ref, 200)
    o = dev.fetch(want=['full_i', 'full_j'])
    r = [min(a, b) for a, b in zip(o['full_i'].tolist(), o['full_j'].tolist())].index(2)
    assert (m[r], diag[r], anti[r]) == (55, 55, 30)


# ------------------------------------------------------------------ drop_links
def _case_engines(case, weighted=False):
    from haphic_amd import cluster
    table = cluster.FragTable.from_reference(case.fa_dict(), dict(case.frag_len), set(case.frag_names), set(case.split), case.bin_size)
    stream = (case.id1, case.pos1, case.id2, case.pos2)
    dev, ref = _both(table, stream, [len(case.id1) // 2], bins=bool(case.split), flank=30_000)
    if weighted:
        totals = ref.fetch()['frag_links']
        assert np.array_equal(totals, dev.fetch(want=['frag_links'])['frag_links'])
        dev.weigh_flank(0, per_frag=totals)
        ref.weigh_flank(0, per_frag=totals)
    return table, dev, ref


def _drops(n_full, n_frag):
    rng = np.random.default_rng(n_full)
    ends = np.zeros(n_full, np.uint8)
    ends[[0, -1]] = 1
    some = (rng.random(n_full) < 0.35).astype(np.uint8)
    every = np.ones(n_frag, np.uint8)
    most = (rng.random(n_frag) < 0.8).astype(np.uint8)
    return {'nothing': (np.zeros(n_full, np.uint8), every), 'everything': (np.ones(n_full, np.uint8), every), 'everything, some fragments outside': (np.ones(n_full, np.uint8), most),
            'first and last': (ends, every), 'a third, some fragments outside': (some, most)}


WHICH = ['nothing', 'everything', 'everything, some fragments outside', 'first and last', 'a third, some fragments outside']


@pytest.mark.parametrize('name,weighted,which', [(n, False, w) for n in ('p4', 'p4_bins') for w in WHICH] +
                         [('p4_norm', True, 'first and last'), ('p4_norm', True, 'a third, some fragments outside')])
def test_drop_links_through_every_consumer(tmp_path, name, weighted, which):
    """combined table (p4), fragment table of split contigs (p4_bins), and float64 weights in the flank table (p4_norm)"""
    from haphic_amd import _lib, cluster, containers
    from oracle import oracle as orc
    case = CASES[name]
    table, dev, ref = _case_engines(case, weighted)
    before = ref.fetch()
    weights_before = dev.fetch_flank_values() if weighted else None
    n_flank_before = len(before['flank_i'])
    full_drop, in_set = _drops(dev.n_full, table.n_frag)[which]
    got, want = dev.drop_links(full_drop, in_set), ref.drop_links(full_drop, in_set)
    assert got[:2] == want[:2] and (dev.n_full, dev.n_flank) == want[:2]
    assert np.array_equal(got[2], want[2]) and len(got[2]) == n_flank_before, 'flank_dropped, dict order of the table before the drop'
    assert np.array_equal(got[3], want[3]) and np.array_equal(dev.first_row, ref.first_row), 'remaining / order of first appearance'
    if which == 'a third, some fragments outside':
        # a flank row of a dropped contig pair with a fragment outside in_set stays
        fi, fj = before['flank_i'], before['flank_j']
        outside = ~(in_set[fi].astype(bool) & in_set[fj].astype(bool))
        assert outside.any() and not got[2][outside].any() and got[2].any()
    if which == 'nothing':
        assert not got[2].any() and got[:2] == (len(before['full_i']), n_flank_before)
    if which == 'everything':
        assert dev.n_full == 0 and (bool(case.split) or (dev.n_flank == 0 and not got[3].any()))
    a, b = dev.fetch(), ref.fetch()
    for k in ('full_i', 'full_j', 'full_cnt', 'ht_cnt', 'flank_i', 'flank_j', 'flank_cnt', 'frag_links'):
        assert np.array_equal(a[k], b[k]), k
    if weighted:
        # carried through the drop bit for bit; against the oracle's own weights within the bound of the weighting kernel (tests/test_gpu_pipeline.py:
        # sqrt where the reference has pow(x, 0.5) — 2 ulp of the quotient)
        carried = weights_before[~got[2].astype(bool)]
        assert np.array_equal(dev.fetch_flank_values().view(np.uint64), carried.view(np.uint64)), 'the weights of the surviving keys'
        np.testing.assert_allclose(carried, ref.fetch_flank_values(), rtol=4.5e-16, atol=0)
        assert carried.dtype == np.float64 and (carried != np.round(carried)).any()
        ref.weights = carried
    m, fidx, n_linked = dev.link_matrix(in_set, weighted=weighted)
    rm, ridx, rl = ref.link_matrix(in_set, weighted=weighted)
    assert n_linked == rl and np.array_equal(fidx[:table.n_frag], ridx[:table.n_frag])
    assert all(np.array_equal(u, v) for u, v in zip(m.to_arrays(), rm.to_arrays()))
    m.free()
    # the queued pickle, the frozen tables' len() and the per-group link sums of output_statistics, against host copies with the same drops
    args = types.SimpleNamespace(remove_allelic_links=case.ploidy, remove_concentrated_links=False, max_read_pairs=40, nwindows=50)
    session = cluster.IngestSession(dev, table, None, args, 'int32', 'int32')
    full, flank = containers.LinkTable(session, 'full'), containers.LinkTable(session, 'flank')
    assert (len(full), len(flank)) == (len(b['full_i']), len(b['flank_i']))
    dev.write_link_pickle_async('full', str(tmp_path / 'full_links.pkl'), table.ctg_names)
    _lib.files_join()
    data = (tmp_path / 'full_links.pkl').read_bytes()
    if data or len(b['full_i']):
        wrote, want_dict = pickle.loads(data), pickle.loads(orc.link_pickle(table.ctg_names, b['full_i'], b['full_j'], b['full_cnt']))
        assert type(wrote) is type(want_dict) and list(wrote.items()) == list(want_dict.items()), 'the queued full_links.pkl'
    groups = {n: ('ungrouped' if k % 5 == 0 else 'group%d' % (k % 3)) for k, n in enumerate(table.ctg_names)}
    host = {(table.ctg_names[i], table.ctg_names[j]): int(c) for i, j, c in zip(b['full_i'], b['full_j'], b['full_cnt'])}
    sums, want_sums = cluster.group_link_dict(full, groups), cluster.group_link_dict(host, groups)
    assert full.frozen and list(sums.items()) == list(want_sums.items())
    # the kept read pairs no longer match the tables: said so, not answered wrongly
    if got[2].any() or full_drop.any():
        with pytest.raises(RuntimeError, match='hhx_ingest_drop_links'):
            dev.fetch_pairs(40, a['full_cnt'])
    session.ing = None
    dev.destroy()


# ------------------------------------------------------------------ the reference's verdicts through the real engine
@pytest.fixture()
def device_mirror(monkeypatch):
    from haphic_amd import allelic, cluster, containers
    monkeypatch.setattr(containers, 'THAW_LOG', [])
    return types.SimpleNamespace(cluster=cluster, allelic=allelic, containers=containers)


@pytest.mark.parametrize('name', list(CASES))
def test_reference_verdicts_with_the_device_engine(device_mirror, golden, name):
    """tests/golden/allelic.npz: ratios, stage 1, both removal masks, remaining, the pickle items and the index map; the allele groups of
    ploidy 4 are the frozen ones (no networkx needed)"""
    from haphic_amd import _lib
    case = CASES[name]
    full, *_rest = case.parse(device_mirror.cluster)
    m, diag, anti = full._session.ing.concordance_counts(case.max_read_pairs, 50, case.min_read_pairs)
    eligible = golden[name + '_eligible']
    assert np.array_equal((full.arrays()[2] >= case.max_read_pairs) | (m >= case.min_read_pairs), eligible)
    ratio = np.maximum(diag[eligible] / m[eligible], anti[eligible] / m[eligible])
    assert np.array_equal(ratio.view(np.uint64), golden[name + '_ratio'][eligible].view(np.uint64))
    groups = frozen_groups(golden, case) if case.ploidy > 2 else None
    got = allelic_cases.run_mirror(case, device_mirror.cluster, device_mirror.allelic, groups=groups)
    assert isinstance(got['session'].ing, _lib.Ingest) and not device_mirror.containers.THAW_LOG
    check_verdict(got, golden, case, device_mirror.cluster, exact_weights=False)


def test_pipeline_c4_end_to_end_without_a_thaw(device_mirror, c4):   # noqa: F811
    pytest.importorskip('networkx')
    got = c4_run(c4, device_mirror.cluster, device_mirror.allelic)
    assert not device_mirror.containers.THAW_LOG
    c4_check(c4, got, device_mirror.cluster)
    st = device_mirror.allelic.STATS
    assert (st['keys'], st['stage1_keys']) == (46677, 828)
