"""CPU: output_statistics :2279-2478 on the device tables (haphic_amd/statistics.py) with the numpy engine of tests/statistics_cases.py in the
library's place, against tests/golden/statistics.npz (the reference's own files), and the engine against the per-key dict restatement."""
import os
import random
import sys
import types

import numpy as np
import pytest

from tests import statistics_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'statistics.npz')
REF = '/root/reference/scripts'
TITLES = ('RE_site_threshold', 'Link_threshold', 'Link_density_threshold', 'Link_density_ratio_threshold')
CASES = {c.name: c for c in sc.fixture_cases()}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


class StandInSession:
    """what a containers.LinkTable needs of its session, from host arrays: a frozen full_link_dict without an ingest handle"""

    def __init__(self, case, values=None):
        self.case = case
        self.table = types.SimpleNamespace(ctg_names=case.names)
        self.values = case.cnt if values is None else values

    def n_keys(self, kind):
        return len(self.case.fi)

    def link_arrays(self, kind):
        return self.case.fi, self.case.fj, self.values, self.case.names

    def note_thawed(self):
        pass


def frozen_full(case, values=None):
    from haphic_amd import containers
    return containers.LinkTable(StandInSession(case, values), 'full')


def golden_case(golden, name):
    """the case as the fixture holds it (the builders of statistics_cases.py must still produce it)"""
    case = CASES[name]
    t = name + '_'
    assert golden[t + 'names'].tolist() == case.names and np.array_equal(golden[t + 'lengths'], case.lengths)
    assert np.array_equal(golden[t + 're_sites'], case.re_sites)
    assert all(np.array_equal(golden[t + k], getattr(case, k)) for k in ('fi', 'fj', 'cnt'))
    assert golden[t + 'labels'].tolist() == [label for label, _c in case.sets]
    for label, clusters in case.sets:
        ptr, ctg = golden['{}cluster_ptr_{}'.format(t, label)], golden['{}cluster_ctg_{}'.format(t, label)]
        assert [ctg[a:b].tolist() for a, b in zip(ptr[:-1], ptr[1:])] == clusters
    return case


def check_files(golden, case, where='.'):
    for label, _clusters in case.sets:
        for title in TITLES:
            with open(os.path.join(where, 'inflation_{}'.format(label), '{}_statistics.txt'.format(title)), 'rb') as f:
                got = f.read()
            want = golden['{}_file_{}_{}'.format(case.name, label, title)].tobytes()
            assert got == want, (case.name, label, title)


def run_mirror(case, link_dict, tmp_path, monkeypatch, engine, original=None, sum_mode=0, draw=False):
    """the mirror in tmp_path with `engine` (a group_stats function) as the library; returns the statistics module.  draw=False: matplotlib does
    not import, the mirror takes the reference's warning branch (the text files are the subject; one test draws)"""
    from haphic_amd import statistics
    if not draw:
        monkeypatch.setitem(sys.modules, 'matplotlib', None)
    monkeypatch.setattr(statistics, '_lib', types.SimpleNamespace(group_stats=engine))
    monkeypatch.setattr(statistics, 'SUM_MODE', sum_mode)
    monkeypatch.chdir(tmp_path)
    for label, _clusters in case.sets:
        os.makedirs('inflation_{}'.format(label), exist_ok=True)
    statistics.output_statistics(case.fa_dict(), link_dict, case.result_clusters_list(), _original=original)
    return statistics


@pytest.mark.parametrize('name', list(CASES))
def test_mirror_on_the_numpy_engine_writes_the_reference_files(golden, name, tmp_path, monkeypatch):
    from haphic_amd import containers
    case = golden_case(golden, name)
    monkeypatch.setattr(containers, 'THAW_LOG', [])
    full = frozen_full(case)
    run_mirror(case, full, tmp_path, monkeypatch, sc.group_stats, sum_mode=int(golden['sum_mode']))
    check_files(golden, case)
    assert full.frozen and not containers.THAW_LOG
    if name.startswith('exact'):
        # the merged key 1000000 prints as whichever came first in fa_dict order: the computed float or the int sentinel
        text = golden['{}_file_2.0_Link_density_ratio_threshold'.format(name)].tobytes().decode()
        assert ('>1000000.0\t' in text) == (name == 'exact_x') and ('>1000000\t' in text) == (name == 'exact_s')


def test_mirror_draws_the_pdf_and_logs_like_the_reference(golden, tmp_path, monkeypatch, caplog):
    pytest.importorskip('matplotlib')
    import logging
    case = golden_case(golden, 'traps')
    with caplog.at_level(logging.INFO, logger='HapHiC_cluster'):
        stats = run_mirror(case, frozen_full(case), tmp_path, monkeypatch, sc.group_stats, sum_mode=int(golden['sum_mode']), draw=True)
    check_files(golden, case)
    for label, _clusters in case.sets:
        with open('inflation_{}/statistics.pdf'.format(label), 'rb') as f:
            assert f.read(5) == b'%PDF-'
    assert stats.STATS['sets'] == 3 and stats.STATS['pdf_s'] > 0
    assert 'Making some statistics for the next HapHiC reassignment step...' in caplog.text


def test_mirror_warns_when_matplotlib_is_missing(golden, tmp_path, monkeypatch, caplog):
    import logging
    case = golden_case(golden, 'exact_x')
    with caplog.at_level(logging.WARNING, logger='HapHiC_cluster'):
        run_mirror(case, frozen_full(case), tmp_path, monkeypatch, sc.group_stats, sum_mode=int(golden['sum_mode']))
    assert 'Module matplotlib is not correctly installed, HapHiC will NOT draw statistical plots' in caplog.text
    assert not os.path.exists('inflation_2.0/statistics.pdf')


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('mode', [0, 1])
def test_numpy_engine_equals_the_dict_restatement(name, mode):
    case = CASES[name]
    args = (case.fi, case.fj, case.cnt) + case.engine_args()
    for got, want in zip(sc.group_stats(*args, mode), sc.dict_group_stats(*args, mode)):
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_the_two_summations():
    """Mode 0 / 1 of the numpy engine against the pure-Python plain / Neumaier loops, and the loop of the running interpreter's kind against sum()
    itself on random lists.  Mode 1 cannot be pinned to the reference's files here: the fixture is written by a CPython 3.10, whose sum() adds
    plainly; it is pinned to CPython 3.12's algorithm as restated in statistics_cases.neumaier_sum, and to sum() itself where 3.12 runs this test."""
    rng = random.Random(5)
    differ = 0
    for _ in range(300):
        xs = [rng.uniform(0, 1) * 10.0 ** rng.randint(-12, 6) for _ in range(rng.randint(0, 40))]
        mine = sc.neumaier_sum(xs) if sys.version_info >= (3, 12) else sc.plain_sum(xs)
        assert mine == sum(xs)
        differ += sc.neumaier_sum(xs) != sc.plain_sum(xs)
    assert differ > 50
    # the engine: a hub with 30 cells of wildly different denominators, both modes against the loops over its own quotients
    fi, fj, cnt, group, n_groups, group_re, ctg_re = sc.star(200, 30, seed=3)
    group_re = (10.0 ** np.random.default_rng(1).uniform(0, 12, 30)).astype(np.int64) + 1
    got = {m: sc.group_stats(fi, fj, cnt, group, n_groups, group_re, ctg_re, m) for m in (0, 1)}
    cells = {}
    for b, v in zip(fj.tolist(), cnt.tolist()):
        g = int(group[0, b])
        if g >= 0:
            cells[g] = cells.get(g, 0) + v
    ranked = sorted(cells.items(), key=lambda x: x[1], reverse=True)
    q = [v / (group_re[g] if g == group[0, 0] else group_re[g] + ctg_re[0] - 1) for g, v in ranked[1:]]
    assert got[0][3][0, 0] == sc.plain_sum(q) and got[1][3][0, 0] == sc.neumaier_sum(q) and len(q) >= 20


def test_families_hold_what_they_are_for():
    """so that the comparison on the GPU means something"""
    ties = CASES['ties']
    assert sum(len(sc.tied_rows(ties, s)) for s in range(len(ties.sets))) >= 20 and len(sc.tied_rows(ties, 1)) >= 20
    mag = CASES['magnitude']
    group, n_groups, group_re, cre = mag.engine_args()
    off = np.concatenate(([0], np.cumsum(n_groups)))
    order_matters = 0
    for s in range(len(mag.sets)):
        gre = group_re[off[s]:off[s + 1]]
        cells = {}
        for a, b, v in zip(mag.fi.tolist(), mag.fj.tolist(), mag.cnt.tolist()):
            for ctg, g in ((a, int(group[s, b])), (b, int(group[s, a]))):
                if g != -1:
                    cells.setdefault(ctg, {}).setdefault(g, 0)
                    cells[ctg][g] += v
        for ctg, inner in cells.items():
            ranked = sorted(inner.items(), key=lambda x: x[1], reverse=True)
            q = [v / (gre[g] if g == group[s, ctg] else gre[g] + cre[ctg] - 1) for g, v in ranked[1:]]
            order_matters += sc.plain_sum(q) != sc.plain_sum(q[::-1])
    assert order_matters >= 20, order_matters
    big = CASES['big']
    assert sc.group_stats(big.fi, big.fj, big.cnt, *big.engine_args())[1].max() > 2 ** 32
    traps = CASES['traps']
    n_cells = sc.group_stats(traps.fi, traps.fj, traps.cnt, *traps.engine_args())[0]
    assert n_cells[0, 7] == 0 and n_cells[0, 8] == 0 and n_cells[0, 6] == 3 and len(sc.tied_rows(traps, 0)) >= 3


def test_patch_reference_binds_the_seam_only_when_asked():
    from haphic_amd import patch, statistics
    H = types.ModuleType('HapHiC_cluster_stand_in')

    def output_statistics(fa_dict, link_dict, result_clusters_list):
        return 'the reference', fa_dict, link_dict, result_clusters_list
    H.output_statistics = output_statistics
    saved = patch.patch_reference(H)
    try:
        assert H.output_statistics is output_statistics and 'output_statistics' not in saved
    finally:
        patch.unpatch_reference(H, saved)
    saved = patch.patch_reference(H, statistics=True)
    try:
        assert H.output_statistics.__wrapped__ is statistics.output_statistics and saved['output_statistics'] is output_statistics
        assert patch.STATISTICS_SEAMS['output_statistics'][0] == 'HapHiC_cluster.py:2279-2478'
        assert H.parse_link_dict.__wrapped__ is patch.cluster.group_link_dict            # still bound underneath
        # a plain dict is the reference function's call
        assert H.output_statistics({'a': ['', 1, 1]}, {}, [])[0] == 'the reference'
    finally:
        patch.unpatch_reference(H, saved)
    assert H.output_statistics is output_statistics
    saved = patch.patch_reference(H, ingest=False, statistics=True)                      # only together with the ingest
    try:
        assert H.output_statistics is output_statistics
    finally:
        patch.unpatch_reference(H, saved)


def test_every_call_the_device_path_does_not_serve_goes_to_the_original(tmp_path, monkeypatch):
    from haphic_amd import ranks, statistics
    case = CASES['traps']
    calls = []

    def original(fa_dict, link_dict, result_clusters_list):
        calls.append(link_dict)
        return 'original'

    def refuse(*a, **k):
        raise AssertionError('the engine must not be asked')

    def run(link_dict, engine=refuse, fa=None):
        monkeypatch.setattr(statistics, '_lib', types.SimpleNamespace(group_stats=engine))
        monkeypatch.chdir(tmp_path)
        n = len(calls)
        out = statistics.output_statistics(fa or case.fa_dict(), link_dict, case.result_clusters_list(), _original=original)
        return out, len(calls) - n

    plain = case.link_dict()
    assert run(plain) == ('original', 1)                                                 # a plain dict
    thawed = frozen_full(case)
    len(thawed), thawed[(case.names[5], case.names[6])]                                  # an item lookup thaws
    assert not thawed.frozen and run(thawed) == ('original', 1)
    assert run(frozen_full(case, case.cnt.astype(np.float64) * 0.5)) == ('original', 1)  # float values
    assert run(frozen_full(case), engine=lambda *a, **k: None) == ('original', 1)        # HHX_UNSUPPORTED
    monkeypatch.setattr(ranks, 'active', lambda: True)                                   # a rank of a multi-rank job
    assert run(frozen_full(case)) == ('original', 1)
    monkeypatch.setattr(ranks, 'active', lambda: False)
    fa = case.fa_dict()
    fa[case.names[3]][2] = 0                                                             # a contig without RE sites: a denominator may be zero
    assert run(frozen_full(case), fa=fa) == ('original', 1)
    fa = case.fa_dict()
    del fa[case.names[7]]                                                                # a contig of the table fa_dict does not have
    assert run(frozen_full(case), fa=fa) == ('original', 1)
    wrong_kind = frozen_full(case)
    wrong_kind._kind = 'flank'
    assert run(wrong_kind) == ('original', 1)
    with pytest.raises(ValueError, match='none was bound'):
        monkeypatch.setattr(statistics, '_lib', types.SimpleNamespace(group_stats=refuse))
        statistics.output_statistics(case.fa_dict(), plain, case.result_clusters_list())


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
@pytest.mark.parametrize('name', ['traps', 'exact_s', 'magnitude'])
def test_bound_seam_in_the_reference_module_serves_frozen_and_plain_dicts(golden, name, tmp_path, monkeypatch):
    """H.output_statistics under patch_reference(H, statistics=True): the frozen table takes the mirror (numpy engine in the library's place) and
    stays frozen; a plain dict goes to the reference's own function, which runs on the parse_link_dict seam; the same files either way"""
    if int(golden['sum_mode']) != (1 if sys.version_info >= (3, 12) else 0):
        pytest.skip('the fixture was written by an interpreter whose sum() adds the other way')
    from haphic_amd import containers, patch, statistics
    H = _load_reference()
    case = golden_case(golden, name)
    monkeypatch.setattr(statistics, '_lib', types.SimpleNamespace(group_stats=sc.group_stats))
    monkeypatch.setattr(containers, 'THAW_LOG', [])
    monkeypatch.setitem(sys.modules, 'matplotlib', None)
    saved = patch.patch_reference(H, statistics=True)
    try:
        for kind in ('frozen', 'plain'):
            where = tmp_path / kind
            where.mkdir()
            monkeypatch.chdir(where)
            for label, _clusters in case.sets:
                os.makedirs('inflation_{}'.format(label))
            link_dict = frozen_full(case) if kind == 'frozen' else case.link_dict()
            H.output_statistics(case.fa_dict(), link_dict, case.result_clusters_list())
            check_files(golden, case)
            if kind == 'frozen':
                assert link_dict.frozen and not containers.THAW_LOG and statistics.STATS['engine'] == 'device'
    finally:
        patch.unpatch_reference(H, saved)


def _load_reference():
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                m = types.ModuleType(name)
                m.__dict__.update(attrs)
                sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import HapHiC_cluster as H
    return H


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
@pytest.mark.parametrize('name', list(CASES))
def test_reference_function_on_each_family_equals_the_fixture(golden, name, tmp_path, monkeypatch):
    if int(golden['sum_mode']) != (1 if sys.version_info >= (3, 12) else 0):
        pytest.skip('the fixture was written by an interpreter whose sum() adds the other way')
    H = _load_reference()
    case = golden_case(golden, name)
    monkeypatch.setitem(sys.modules, 'matplotlib', None)           # the reference's own "not installed" branch: no PDFs, the same text
    monkeypatch.chdir(tmp_path)
    for label, _clusters in case.sets:
        os.makedirs('inflation_{}'.format(label))
    H.output_statistics(case.fa_dict(), case.link_dict(), case.result_clusters_list())
    check_files(golden, case)
