"""Stage 2 of --remove_allelic_links on the device (hhx_allelic_nonmax / hhx_lsap_small, haphic_amd/csrc/hhx_allelic.hip) on the GPU:
  * _lib.lsap_small against scipy.optimize.linear_sum_assignment on the matrix families of tests/allelic_stage2_cases.py (ties are the rule),
    counts up to 2^40, batch sizes around the wavefront, with the default grid and on two workgroups (HHX_NONMAX_GRID);
  * _lib.allelic_nonmax against allelic.nonmax_keys (mask and the three counters) on seeded random and hand-built keys and allele groups;
  * the reference's verdicts (tests/golden/allelic.npz, pipeline_c4.npz) through the mirror with the real engine and the device form of stage 2,
    its counters against a host-form run of the same case."""
import types

import numpy as np
import pytest

from tests import allelic_cases, allelic_stage2_cases as s2
from tests.test_allelic_cases_cpu import CASES, c4, c4_check, c4_run, check_verdict, frozen_groups, golden   # noqa: F401 (c4, golden: fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[None, '2'], ids=['default grid', 'two workgroups'])
def grid(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv('HHX_NONMAX_GRID', raising=False)
    else:
        monkeypatch.setenv('HHX_NONMAX_GRID', request.param)
    return request.param


# ------------------------------------------------------------------ the solver
def test_lsap_small_on_the_families(grid):
    from haphic_amd import _lib
    fam, want = s2.families(), s2.family_answers()
    for name, matrices in fam.items():
        got = _lib.lsap_small(-matrices)
        assert got.dtype == np.int32 and got.shape == want[name].shape
        bad = np.flatnonzero((got != want[name]).any(axis=1))
        assert not len(bad), (name, len(bad), matrices[bad[0]].tolist(), got[bad[0]].tolist(), want[name][bad[0]].tolist())


def test_lsap_small_counts_up_to_2_40(grid):
    from haphic_amd import _lib
    matrices = s2.wide_counts()
    assert matrices.shape[1:] == (8, 8) and int(matrices.max()) > 2 ** 39
    assert np.array_equal(_lib.lsap_small(-matrices), s2.scipy_col4row(matrices))


def test_lsap_small_batch_sizes(grid):
    from haphic_amd import _lib
    rng = np.random.default_rng(4097)
    matrices = rng.integers(0, 4, (4097, 5, 5)).astype(np.int64)
    matrices[rng.random(matrices.shape) < 0.4] = 0
    want = s2.scipy_col4row(matrices)
    for n in (1, 63, 64, 65, 4097):
        assert np.array_equal(_lib.lsap_small(-matrices[:n]), want[:n]), n
    assert _lib.lsap_small(np.zeros((0, 3, 3), np.int64)).shape == (0, 3)
    with pytest.raises(RuntimeError, match='hhx_lsap_small'):
        _lib.lsap_small(np.zeros((2, 9, 9), np.int64))


# ------------------------------------------------------------------ the whole of stage 2 against the host form
def _both(names, groups, ki, kj, kcnt):
    """(host mask or None, host stats, what _lib.allelic_nonmax returns)"""
    from haphic_amd import _lib, allelic
    stats = {}
    rank = np.argsort(np.argsort(names)).astype(np.int32)
    want = allelic.nonmax_keys(ki, kj, kcnt, list(groups), names, rank, stats)
    gptr, gmem = s2.group_csr(groups, names)
    return want, stats, _lib.allelic_nonmax(ki, kj, kcnt, len(names), gptr, gmem)


def _same(want, stats, got, what):
    if want is None:
        assert got is None, what
        return
    assert got is not None and got is not NotImplemented, what
    mask, counters = got
    assert mask.dtype == np.uint8 and np.array_equal(mask.astype(bool), want), (what, np.flatnonzero(mask.astype(bool) != want)[:10])
    assert counters.tolist() == [stats['candidates'], stats['group_pairs'], stats['assignments']], (what, counters.tolist(), stats)


RANDOM = [  # seed, contigs, groups, keys, group sizes
    (1, 30, 6, 0, (2, 4)), (2, 30, 6, 40, (2, 4)), (3, 60, 12, 300, (2, 8)), (4, 60, 10, 900, (3, 5)), (5, 120, 30, 2500, (2, 8)),
    (6, 200, 40, 4000, (2, 8)), (7, 200, 25, 3000, (7, 8)), (8, 90, 30, 1500, (2, 2)),
]


@pytest.mark.parametrize('workgroups', [None, '1', '2'], ids=['default grid', 'one workgroup', 'two workgroups'])
@pytest.mark.parametrize('seed,n_ctg,n_groups,n_keys,sizes', RANDOM)
def test_nonmax_on_random_keys_and_groups(monkeypatch, workgroups, seed, n_ctg, n_groups, n_keys, sizes):
    if workgroups is None:
        monkeypatch.delenv('HHX_NONMAX_GRID', raising=False)
    else:
        monkeypatch.setenv('HHX_NONMAX_GRID', workgroups)
    names, groups, ki, kj, kcnt = s2.random_groups_and_keys(seed, n_ctg, n_groups, n_keys, sizes)
    want, stats, got = _both(names, groups, ki, kj, kcnt)
    _same(want, stats, got, seed)
    if n_keys >= 300:
        # the case says something: candidates, problems that were solved, keys in and out of the matchings
        assert want is not None and stats['assignments'] > 0 and want.any() and not want.all()
        assert max(map(len, groups)) <= sizes[1] and len({c for g in groups for c in g}) < sum(map(len, groups)), 'some contig sits in several groups'


@pytest.mark.parametrize('name', list(s2.hand_built()))
def test_nonmax_on_hand_built_cases(grid, name):
    names, groups, keys = s2.hand_built()[name]
    ki, kj, kcnt = (np.array([k[c] for k in keys], dt) for c, dt in ((0, np.int32), (1, np.int32), (2, np.int64)))
    want, stats, got = _both(names, groups, ki, kj, kcnt)
    assert want is not None
    _same(want, stats, got, name)
    expect = {'no groups': (0, 0, 0), 'no candidate': (0, 0, 0), 'no keys': (0, 0, 0), 'a pair reached by a single key': (1, 1, 0),
              'two keys on one row: the cheaper one is not in the matching': (2, 1, 1), 'ga == gb': (4, 1, 1)}
    if name in expect:
        assert tuple(got[1].tolist()) == expect[name]
    if name == 'two keys on one row: the cheaper one is not in the matching':
        assert got[0].tolist() == [1, 0]
    if name == 'both contigs in both groups of a pair':
        assert got[1][1] == 3 and got[1][2] >= 1                 # (g0, g0), (g0, g1), (g1, g1); key (a, b) names (g0, g1) twice


def test_nonmax_assert_case_and_a_group_of_nine():
    """:653 — keys [(a, b)] with groups [(a, b), (a, c)]: group_pair[0] holds ctg_1, group_pair[1] does not hold ctg_2; and a group beyond the solver"""
    from haphic_amd import _lib, allelic
    L = s2.LETTERS
    ki, kj, kcnt = np.array([0], np.int32), np.array([1], np.int32), np.array([5], np.int64)
    groups = [('a', 'b'), ('a', 'c')]
    want, _stats, got = _both(L, groups, ki, kj, kcnt)
    assert want is None and got is None
    assert allelic.nonmax_keys_device(ki, kj, kcnt, groups, L, None) is None
    nine = [tuple(L[:9]), ('j', 'k')]
    gptr, gmem = s2.group_csr(nine, L)
    assert _lib.allelic_nonmax(np.array([0], np.int32), np.array([9], np.int32), kcnt, len(L), gptr, gmem) is NotImplemented
    assert allelic.nonmax_keys_device(np.array([0], np.int32), np.array([9], np.int32), kcnt, nine, L, None) is NotImplemented
    with pytest.raises(RuntimeError, match='outside'):
        _lib.allelic_nonmax(np.array([0], np.int32), np.array([len(L)], np.int32), kcnt, len(L), *s2.group_csr(groups, L))


def test_nonmax_keys_device_fills_the_same_stats():
    from haphic_amd import allelic
    names, groups, ki, kj, kcnt = s2.random_groups_and_keys(5, 120, 30, 2500, (2, 8))
    host, dev = {}, {}
    want = allelic.nonmax_keys(ki, kj, kcnt, groups, names, None, host)
    got = allelic.nonmax_keys_device(ki, kj, kcnt, groups, names, None, dev)
    assert got.dtype == bool and np.array_equal(got, want)
    assert set(dev) == set(host) and dev['assignment_s'] == 0.0
    assert all(dev[k] == host[k] for k in ('candidates', 'group_pairs', 'assignments'))


# ------------------------------------------------------------------ the reference's verdicts through the real engine
@pytest.fixture()
def device_mirror(monkeypatch):
    from haphic_amd import allelic, cluster, containers
    monkeypatch.setattr(containers, 'THAW_LOG', [])
    monkeypatch.delenv('HHX_NONMAX_GRID', raising=False)
    return types.SimpleNamespace(cluster=cluster, allelic=allelic, containers=containers, setenv=monkeypatch.setenv)


COUNTERS = ('candidates', 'group_pairs', 'assignments', 'keys', 'stage1_keys', 'stage2_keys', 'allele_groups')


@pytest.mark.parametrize('name', list(CASES))
def test_reference_verdicts_with_stage_2_on_the_device(device_mirror, golden, name):  # noqa: F811
    from haphic_amd import _lib
    case = CASES[name]
    groups = frozen_groups(golden, case) if case.ploidy > 2 else None
    seen = {}
    for engine in ('device', 'host'):
        device_mirror.setenv('HAPHIC_ALLELIC_STAGE2', engine)
        got = allelic_cases.run_mirror(case, device_mirror.cluster, device_mirror.allelic, groups=groups)
        assert isinstance(got['session'].ing, _lib.Ingest) and not device_mirror.containers.THAW_LOG
        check_verdict(got, golden, case, device_mirror.cluster, exact_weights=False)
        st = dict(device_mirror.allelic.STATS)
        assert st['stage2_engine'] == engine
        seen[engine] = {k: st[k] for k in COUNTERS}
    assert seen['device'] == seen['host'] and seen['device']['stage2_keys'] == int(golden[name + '_nonmax'].sum())


def test_pipeline_c4_with_stage_2_on_the_device(device_mirror, c4):   # noqa: F811
    pytest.importorskip('networkx')
    seen = {}
    for engine in ('device', 'host'):
        device_mirror.setenv('HAPHIC_ALLELIC_STAGE2', engine)
        got = c4_run(c4, device_mirror.cluster, device_mirror.allelic)
        assert not device_mirror.containers.THAW_LOG
        c4_check(c4, got, device_mirror.cluster)
        st = dict(device_mirror.allelic.STATS)
        assert st['stage2_engine'] == engine and (st['keys'], st['stage1_keys']) == (46677, 828)
        seen[engine] = {k: st[k] for k in COUNTERS}
    assert seen['device'] == seen['host'] and seen['device']['assignments'] > 0
