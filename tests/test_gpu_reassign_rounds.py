"""The rounds of `haphic reassign` on the device (haphic_amd/csrc/hhx_reassign.hip, haphic_amd/reassign.py) on the GPU:
  * hhx_reassign_round against tests/golden/reassign_rounds.npz (the reference's own run_reassignment :266-427): every case, every call, the
    rescue round included: groups, group_RE values and the four counts equal;
  * 2 100 groups (more than the LDS table holds: the rows are ordered on a table in HBM) against the numpy engine of tests/reassign_cases.py,
    under both sum modes, on a job whose lists of densities add up differently under the two;
  * windows of one, two and three contigs (hhx_tune "reassign_window") give the same result, with the launch counts they must take;
  * hhx_reassign_pair_sums against the fixture: sums, first positions, the masked-out keys;
  * the three seams of patch_reassign(R, rounds=True) end to end on a stand-in module: dicts with their key order, log lines,
    group_group_links.txt byte for byte, the matrix handed to the clustering; a thaw before the first round equals cluster.parse_link_dict's
    return, a thaw after one raises; every hand-back condition reaches the original function."""
import logging
import os
import types

import numpy as np
import pytest

from tests import reassign_cases as rc

pytestmark = pytest.mark.gpu

CASES = rc.load_cases()


def device_engine(case):
    from haphic_amd import _lib
    return _lib.Reassign(case['fi'], case['fj'], case['links'], len(case['group0']), case['group0'], len(case['group_re0']))


def check_job(case, out, what):
    assert len(out) == len(case['nrounds'])
    for k, (nround, group, group_re, counts) in enumerate(out):
        print(what, 'round', nround, 'counts', counts.tolist(), 'want', case['counts'][k].tolist(), 'groups differing',
              int((group != case['groups'][k]).sum()))
        assert (group == case['groups'][k]).all(), (what, nround)
        assert (group_re == case['group_res'][k]).all(), (what, nround)
        assert counts.tolist() == case['counts'][k].tolist(), (what, nround)


@pytest.fixture
def window():
    from haphic_amd import _lib
    yield lambda w: _lib.tune('reassign_window', w)
    _lib.tune('reassign_window', None)


@pytest.mark.parametrize('name', sorted(CASES))
def test_rounds_against_the_reference(name):
    case = CASES[name]
    engine = device_engine(case)
    sums, first = engine.cells()
    want = rc.NumpyReassign(case['fi'], case['fj'], case['links'], len(case['group0']), case['group0'], len(case['group_re0'])).cells()
    assert (sums == want[0]).all() and (first == want[1]).all()
    check_job(case, rc.run_job(case, engine), name)
    engine.close()


@pytest.mark.parametrize('name', ['ties_gfa', 'dismissal'])
@pytest.mark.parametrize('w', [1, 2, 3])
def test_small_windows_give_the_same_result(name, w, window):
    case = CASES[name]
    window(w)
    engine = device_engine(case)
    launches = []
    check_job(case, rc.run_job(case, engine, on_round=lambda nround: launches.append(engine.launches)), '%s window %d' % (name, w))
    n, movers = len(case['order']), case['counts'][:, 1] + case['counts'][:, 2]
    print('launch pairs per call', launches, 'movers', movers.tolist())
    for got, m in zip(launches, movers.tolist()):
        # every pair judges at most w contigs and ends at its first mover; the last pairs of a batch may find nothing left
        assert (n + w - 1) // w <= got <= n if w > 1 else got == n
        assert got >= m
    assert (movers[0] > n // 5) and (movers[-2:] <= 1).all()               # both regimes: movers closer than the window, and much farther apart
    engine.close()


def many_groups_job():
    """150 contigs, every grouped one in a group of its own among 2 100, all pairs linked: a row holds up to 149 cells"""
    rng = np.random.default_rng(77)
    n_ctg, n_groups = 150, 2100
    fi, fj = np.triu_indices(n_ctg, 1)
    keep = rng.permutation(fi.size)[:9000]
    fi, fj = fi[keep].astype(np.int32), fj[keep].astype(np.int32)
    links = rng.integers(1, 400, fi.size).astype(np.int64)
    group = rng.permutation(n_groups)[:n_ctg].astype(np.int32)
    group[rng.random(n_ctg) < 0.3] = -1
    pairs = rng.permutation(n_ctg)[:60].reshape(-1, 2)                   # some groups of two, so that a contig can be consistent
    group[pairs[:, 1]] = group[pairs[:, 0]]
    ctg_re = rng.integers(20, 300, n_ctg).astype(np.int64)
    group_re = np.ones(n_groups, np.int64)
    np.add.at(group_re, group[group >= 0], ctg_re[group >= 0] - 1)
    ctg_len = ctg_re * 400
    return dict(fi=fi, fj=fj, links=links, group0=group, group_re0=group_re, ctg_re=ctg_re, ctg_len=ctg_len,
                order=np.argsort(-ctg_len, kind='stable').astype(np.int32), gfa=np.bool_(False), max_ctg_len=np.float64(100), min_RE_sites=np.int64(25),
                min_links=np.float64(25), min_link_density=np.float64(0.0001), min_density_ratio=np.float64(40), ambiguous_cutoff=np.float64(0.95),
                min_group_len=np.float64(0), nrounds=np.array([1, 2, 0], np.int32))


@pytest.fixture(scope='module')
def many_groups():
    case = many_groups_job()
    want = {}
    for sum_mode in (0, 1):
        engine = rc.NumpyReassign(case['fi'], case['fj'], case['links'], len(case['group0']), case['group0'], len(case['group_re0']))
        want[sum_mode] = (rc.run_job(case, engine, sum_mode), engine.mode_sensitive)
    return case, want


@pytest.mark.parametrize('sum_mode', [0, 1])
def test_more_groups_than_the_lds_table_holds(many_groups, sum_mode):
    case, want = many_groups
    out_want, mode_sensitive = want[sum_mode]
    print('judgements whose densities add up differently under the two modes:', mode_sensitive)
    assert mode_sensitive > 0                                            # on the host first: the two modes are told apart by this job
    counts = np.array([o[3] for o in out_want])
    print('counts per call', counts.tolist())
    assert (counts[0] > 0).all()                                         # every verdict occurs
    out = rc.run_job(case, device_engine(case), sum_mode)
    for (nround, group, group_re, cnt), (_n, g_want, re_want, c_want) in zip(out, out_want):
        assert (group == g_want).all() and (group_re == re_want).all() and cnt.tolist() == c_want.tolist(), (sum_mode, nround)


def test_what_the_library_does_not_serve():
    from haphic_amd import _lib
    case = CASES['defaults']
    engine = device_engine(case)
    group, group_re = case['group0'].copy(), case['group_re0'].copy()
    args = (case['ctg_re'], case['order'], rc.case_flags(case), None)
    with pytest.raises(_lib.Reassign.Unsupported, match='sum_mode'):
        engine.round(group, group_re, *args, 25, 0.0001, 4, 0.6, False, False, 2)
    with pytest.raises(RuntimeError, match='min_links'):
        engine.round(group, group_re, *args, 0.5, 0.0001, 4, 0.6, False, False, 0)
    assert (group == case['group0']).all() and (group_re == case['group_re0']).all()
    engine.close()


@pytest.mark.parametrize('name', sorted(CASES))
def test_pair_sums_against_the_reference(name):
    case = CASES[name]
    engine = device_engine(case)
    rc.check_pair_sums(case, *engine.pair_sums(case['agg_member'], case['agg_group'], len(case['agg_names'])))
    none = engine.pair_sums(np.zeros_like(case['agg_member']), case['agg_group'], len(case['agg_names']))
    assert not none[0].any() and (none[1] == -1).all()
    engine.close()


# ------------------------------------------------------------------ the seams on a stand-in module
class Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


class RecordingClustering:
    """stands where sklearn's AgglomerativeClustering stands: keeps the matrix it is handed"""
    seen = []

    def __init__(self, **kwargs):
        self.kwargs = kwargs

    @classmethod
    def _get_param_names(cls):
        return ['n_clusters', 'metric', 'linkage', 'distance_threshold']

    def fit_predict(self, X):
        RecordingClustering.seen.append((self.kwargs, np.array(X)))
        return np.arange(len(X)) % self.kwargs['n_clusters']


@pytest.fixture
def stand_in():
    """a module object with the names the mirrors resolve; its own three functions only record that they were reached"""
    R = types.ModuleType('HapHiC_reassign_stand_in')
    R.reached = []
    R.logger = logging.getLogger('HapHiC_reassign_rounds_test')
    R.logger.setLevel(logging.INFO)
    R.logger.propagate = False
    R.lines = Lines()
    R.logger.addHandler(R.lines)
    R.parse_link_dict = lambda link_dict, ctg_group_dict, normalize_by_nlinks=False: R.reached.append(('parse_link_dict',)) or 'theirs'
    R.run_reassignment = lambda *args: R.reached.append(('run_reassignment', type(args[1]).__name__, type(args[4]).__name__)) or 'theirs'
    R.agglomerative_hierarchical_clustering = lambda *args, **kwargs: R.reached.append(('agglomerative_hierarchical_clustering',)) or 'theirs'
    R.split_clm_file = lambda *args: 'theirs'
    R.dict_to_matrix = rc.dense_dict_to_matrix
    R.AgglomerativeClustering = RecordingClustering
    RecordingClustering.seen = []
    from haphic_amd import patch
    saved = patch.patch_reassign(R, rounds=True)
    assert set(saved) == {'parse_link_dict', 'split_clm_file', 'run_reassignment', 'agglomerative_hierarchical_clustering'}
    yield R
    R.logger.removeHandler(R.lines)


def test_seams_end_to_end(stand_in, tmp_path, monkeypatch):
    R, case = stand_in, CASES['defaults']
    d = rc.case_dicts(case)
    keys_before = list(d['ctg_group_dict']), list(d['group_RE_dict'])
    state = []
    rc.drive_rounds(R, d, after_call=lambda nround: state.append((nround, dict(d['ctg_group_dict']), dict(d['group_RE_dict']))))
    assert [s[0] for s in state] == case['nrounds'].tolist() and not R.reached
    for k, (nround, ctg_group, group_re) in enumerate(state):
        want = {d['names'][c]: (d['gnames'][g] if g >= 0 else 'ungrouped') for c, g in enumerate(case['groups'][k].tolist())}
        assert ctg_group == want, nround
        assert group_re == dict(zip(d['gnames'], case['group_res'][k].tolist())), nround
    assert (list(d['ctg_group_dict']), list(d['group_RE_dict'])) == keys_before
    assert all(type(v) is int for v in d['group_RE_dict'].values()) and all(type(v) is str for v in d['ctg_group_dict'].values())
    want_lines = []
    for nround, line in zip(case['nrounds'].tolist(), case['info'].tolist()):
        want_lines += ['Performing reassignment...' if nround else 'Performing additional round of rescue...', line]
    assert R.lines.lines == want_lines
    # ---- the agglomerative step on the fixture's own inputs
    new_names = case['agg_names'].tolist()
    new_ctg_group_dict = {d['names'][c]: new_names[g] for c, g in enumerate(case['agg_group'].tolist()) if g >= 0}
    grouped_ctgs = {d['names'][c] for c in np.flatnonzero(case['agg_member']).tolist()}
    new_old_group_dict = {g: 'old_' + g for g in new_names}
    group_hiconf_RE_dict = {'old_' + g: int(v) for g, v in zip(new_names, case['agg_hiconf_re'].tolist())}
    monkeypatch.chdir(tmp_path)
    os.mkdir('hc_groups')
    hc = R.agglomerative_hierarchical_clustering(d['full_link_dict'], grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict,
                                                 int(case['agg_nclusters']))
    assert open('hc_groups/group_group_links.txt', 'rb').read() == case['agg_txt'].tobytes()
    (kwargs, matrix), = RecordingClustering.seen
    assert kwargs == dict(n_clusters=int(case['agg_nclusters']), metric='precomputed', linkage='average', distance_threshold=None)
    assert matrix.dtype == np.float32 and (matrix.astype(np.float64) == case['agg_matrix']).all()      # the fixture keeps the float32 values widened
    assert sorted(g for v in hc.values() for g in v) == sorted(new_names) and len(hc) == int(case['agg_nclusters'])
    assert R.lines.lines[len(want_lines):] == ['Performing additional agglomerative hierarchical clustering...',
                                               'The parameter "affinity" is not found in AgglomerativeClustering, use "metric" instead']
    assert R.agglomerative_hierarchical_clustering(d['full_link_dict'], grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict, 2,
                                                   normalize_by_nlinks=True) == 'theirs'
    assert R.agglomerative_hierarchical_clustering(dict(d['full_link_dict']), grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict,
                                                   new_old_group_dict, 2) == 'theirs'          # another dict than the handle was built from


def nested(tables):
    return [(c, list(inner.items())) for c, inner in tables[0].items()], [(c, sorted(s)) for c, s in tables[1].items()]


def test_thaw_before_the_first_round_and_after(stand_in):
    from haphic_amd import cluster, reassign
    R, d = stand_in, rc.case_dicts(CASES['dismissal'])
    tables = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
    assert type(tables[0]) is reassign.RoundTable and type(tables[1]) is reassign.RoundTable
    want = cluster.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
    assert tables[0]['c000'] == want[0]['c000'] and type(tables[0]).__name__ == 'Thawed'        # any access thaws
    assert nested(tables) == nested(want) and tables[0].default_factory is dict and tables[1].default_factory is set
    assert tables[0] == want[0] and tables[1] == want[1]
    tables = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
    rc.call_round(R, d, tables, 1)
    assert not R.reached
    for table in tables:
        with pytest.raises(RuntimeError, match='have run on the device'):
            len(table)
    with pytest.raises(RuntimeError, match='have run on the device'):                          # a hand-back now cannot rebuild the dicts
        rc.call_round(R, d, tables, 2, whitelist={'c001'})


def test_every_hand_back_reaches_the_original(stand_in):
    R, case = stand_in, CASES['defaults']
    d = rc.case_dicts(case)

    def fresh():
        return R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])

    def reached(tables, nround=1, **kwargs):
        R.reached.clear()
        before = dict(d['ctg_group_dict']), dict(d['group_RE_dict'])
        assert rc.call_round(R, d, tables, nround, **kwargs) == 'theirs'
        assert (dict(d['ctg_group_dict']), dict(d['group_RE_dict'])) == before
        return R.reached[0]
    thawed = ('run_reassignment', 'Thawed', 'Thawed')
    assert reached(fresh(), whitelist={'c001'}) == thawed
    assert reached(fresh(), min_links=0) == thawed
    assert reached(fresh(), min_links=0.5) == thawed
    R.logger.setLevel(logging.DEBUG)
    assert reached(fresh()) == thawed
    R.logger.setLevel(logging.INFO)
    a, b = fresh(), fresh()
    assert reached((a[0], b[1])) == thawed                                                      # not both from the same parse_link_dict call
    assert reached(({}, {})) == ('run_reassignment', 'dict', 'dict')                            # not ours
    big = dict(d, RE_site_dict=dict(d['RE_site_dict'], c000=2 ** 53))
    R.reached.clear()
    assert rc.call_round(R, big, fresh(), 1) == 'theirs' and R.reached[0] == thawed              # an RE total that reaches 2^53
    other = dict(d, full_link_dict=dict(d['full_link_dict']))
    R.reached.clear()
    assert rc.call_round(R, other, fresh(), 1) == 'theirs' and R.reached[0] == thawed            # another full_link_dict than the tables' own
    # links that reach 2^53, float links and normalize_by_nlinks never become tables of ours
    huge = dict(d['full_link_dict'])
    huge[next(iter(huge))] = 2 ** 52
    tables = R.parse_link_dict(huge, d['ctg_group_dict'])
    assert type(tables[0]).__name__ == 'defaultdict' and type(tables[1]).__name__ == 'defaultdict'
    R.reached.clear()
    floats = dict(d['full_link_dict'])
    floats[next(iter(floats))] = 1.5
    assert R.parse_link_dict(floats, d['ctg_group_dict']) == 'theirs'
    assert R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'], normalize_by_nlinks=True) == 'theirs'
    assert R.reached == [('parse_link_dict',), ('parse_link_dict',)]
    # and nothing above has spent the tables of a fresh call
    check = rc.case_dicts(case)
    R.reached.clear()
    rc.call_round(R, check, R.parse_link_dict(check['full_link_dict'], check['ctg_group_dict']), 1)
    assert not R.reached and list(check['group_RE_dict'].values()) == case['group_res'][0].tolist()
