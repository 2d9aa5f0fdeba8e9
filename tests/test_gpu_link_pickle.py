"""GPU: full_links.pkl / HT_links.pkl read into arrays on the device (_lib.read_link_pickle, csrc/hhx_pickleread.hip) against pickle.load +
cluster._dict_arrays, for every case of tests/link_pickle_cases.py in Python's dialect and in the library's, at the default chunk of the
boundary search and at 512 bytes (a seam everywhere); every hand-back case; the write / read round trip; and the chain of run() from a .pkl file
through patch_reassign(R, rounds=True, pickle=True) on one job of tests/golden/reassign_rounds.npz."""
import logging
import os
import pickle
import types

import numpy as np
import pytest

from haphic_amd import _lib, cluster, containers, patch, reassign
from tests import link_pickle_cases as lp
from tests import reassign_cases as rc

pytestmark = pytest.mark.gpu

ACCEPTED = lp.accepted()
HANDED_BACK = lp.handed_back()
CHUNKS = [None, 512]


@pytest.fixture(params=CHUNKS, ids=['chunk_default', 'chunk_512'])
def chunk(request):
    _lib.tune('pkl_chunk', request.param)
    yield request.param
    _lib.tune('pkl_chunk', None)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """every accepted case written once per dialect, with the dict pickle.load gives back: {(name, dialect): (path, dict)}"""
    root = tmp_path_factory.mktemp('link_pickles')
    out = {}
    for name, d in ACCEPTED.items():
        for dialect in ('python', 'python5', 'library'):
            if dialect == 'library' and not lp.library_can_write(d):
                continue
            path = str(root / ('%s.%s.pkl' % (name, dialect)))
            if dialect == 'library':
                lp.write_library(d, path)
            else:
                lp.write_python(d, path, 5 if dialect == 'python5' else 4)
            out[name, dialect] = (path, pickle.load(open(path, 'rb')))
    return out


@pytest.mark.parametrize('dialect', ['python', 'python5', 'library'])
@pytest.mark.parametrize('name', sorted(ACCEPTED))
def test_arrays_equal_the_oracle(name, dialect, chunk, files):
    if (name, dialect) not in files:
        assert dialect == 'library' and not lp.library_can_write(ACCEPTED[name])
        return
    path, loaded = files[name, dialect]
    lp.check_arrays(_lib.read_link_pickle(path), loaded)


@pytest.mark.parametrize('name', ['full_links', 'HT_links'])
def test_the_files_the_reference_wrote(name, chunk, tmp_path):
    path = str(tmp_path / (name + '.pkl'))
    open(path, 'wb').write(lp.golden()[name])
    lp.check_arrays(_lib.read_link_pickle(path), pickle.load(open(path, 'rb')))


@pytest.mark.parametrize('name', sorted(HANDED_BACK))
def test_hand_backs_give_none_and_the_library_answers_the_next_call(name, chunk, files, tmp_path):
    path = str(tmp_path / 'x.pkl')
    open(path, 'wb').write(HANDED_BACK[name])
    refusals = len(_lib.PICKLE_REFUSALS)
    assert _lib.read_link_pickle(path) is None
    assert len(_lib.PICKLE_REFUSALS) == refusals + 1 and _lib.PICKLE_REFUSALS[-1]
    good, loaded = files['n2', 'python']
    lp.check_arrays(_lib.read_link_pickle(good), loaded)


@pytest.mark.parametrize('name', sorted(HANDED_BACK))
def test_mirror_gives_what_pickle_load_gives_for_a_hand_back(name, tmp_path):
    path = str(tmp_path / 'x.pkl')
    open(path, 'wb').write(HANDED_BACK[name])
    kind, want = lp.load_or_error(HANDED_BACK[name])
    parse_pickle = reassign.bind_pickle(types.SimpleNamespace(logger=logging.getLogger('link_pickle_test')))
    if kind == 'error':
        with pytest.raises(want):
            parse_pickle({}, path)
        return
    got = parse_pickle({}, path)[0]
    assert type(got) is type(want) and list(got.items()) == list(want.items()) and [type(v) for v in got.values()] == [type(v) for v in want.values()]


def test_null_handle_and_missing_file(tmp_path):
    L = _lib.load()
    assert L.hhx_pickle_sizes(None, None, None, None, None) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_pickle_fetch(None, None, None, None, None, None, None) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_pickle_open(None, None) != 0 and L.hhx_pickle_free(None) == 0
    with pytest.raises(RuntimeError, match='cannot open'):
        _lib.read_link_pickle(str(tmp_path / 'missing.pkl'))


def test_round_trip_through_the_writer(chunk, tmp_path):
    rng = np.random.default_rng(7)
    n_names, n_keys = 300, 5000
    names = ['utg%06dl_%d' % (k * 7919 % 1000003, k) for k in range(n_names)]
    flat = rng.choice(n_names * n_names, n_keys, replace=False)
    i, j = (flat // n_names).astype(np.int32), (flat % n_names).astype(np.int32)
    count = rng.integers(1, 70000, n_keys).astype(np.int64)
    count[:6] = [2 ** 31, -2 ** 31 - 1, 2 ** 63 - 1, -2 ** 63, 0, 140]
    path = str(tmp_path / 'full_links.pkl')
    _lib.write_link_pickle(path, i, j, count, names)
    gi, gj, value, is_float, gnames = _lib.read_link_pickle(path)
    assert is_float is None and value.tolist() == count.tolist()
    assert [gnames[k] for k in gi.tolist()] == [names[k] for k in i.tolist()] and [gnames[k] for k in gj.tolist()] == [names[k] for k in j.tolist()]
    lp.check_arrays((gi, gj, value, is_float, gnames), pickle.load(open(path, 'rb')))


def test_thaw_of_the_device_table_is_the_loaded_dict(files):
    for key in (('int_and_float', 'python'), ('floats', 'python'), ('utf8', 'library'), ('n0', 'python')):
        path, loaded = files[key]
        table = reassign.bind_pickle(types.SimpleNamespace(logger=logging.getLogger('link_pickle_test')))({}, path)[0]
        assert type(table) is containers.LinkTable and table.frozen is True and len(table) == len(loaded)
        assert cluster.integral_links(table) is all(type(v) is int for v in loaded.values()) and table.frozen is True
        assert list(table.items()) == list(loaded.items()) and [type(v) for v in table.values()] == [type(v) for v in loaded.values()]
        assert table.frozen is False and table.default_factory is int


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


class _Clustering:
    """stands where sklearn's AgglomerativeClustering stands"""

    def __init__(self, **kwargs):
        self.kwargs = kwargs

    @classmethod
    def _get_param_names(cls):
        return ['n_clusters', 'metric', 'linkage', 'distance_threshold']

    def fit_predict(self, X):
        return np.arange(len(X)) % self.kwargs['n_clusters']


@pytest.mark.parametrize('library', [False, True], ids=['python_dialect', 'library_dialect'])
def test_the_seams_of_run_from_a_pkl_file_on_the_device(library, tmp_path, monkeypatch):
    """parse_pickle, parse_link_dict, the rounds and the agglomerative step through patch_reassign(R, rounds=True, pickle=True) on a stand-in module,
    full_link_dict read from a .pkl file: the dicts, counts and log lines the reference's functions recorded in the golden, nothing thawed"""
    from collections import defaultdict
    case = rc.load_cases()['defaults']
    d = rc.case_dicts(case)
    pkl = str(tmp_path / 'full_links.pkl')
    (lp.write_library if library else lp.write_python)(defaultdict(int, d['full_link_dict']), pkl)
    R = types.ModuleType('HapHiC_reassign_stand_in')
    R.logger = logging.getLogger('HapHiC_reassign_pickle_test')
    R.logger.setLevel(logging.INFO)
    R.logger.propagate = False
    lines = _Lines()
    R.logger.addHandler(lines)
    for name in ('parse_pickle', 'parse_link_dict', 'run_reassignment', 'agglomerative_hierarchical_clustering', 'split_clm_file'):
        setattr(R, name, lambda *args, **kwargs: pytest.fail('handed back to the reference function'))
    R.dict_to_matrix = rc.dense_dict_to_matrix
    R.AgglomerativeClustering = _Clustering
    saved = patch.patch_reassign(R, rounds=True, pickle=True)
    assert set(saved) == {'parse_pickle', 'parse_link_dict', 'split_clm_file', 'run_reassignment', 'agglomerative_hierarchical_clustering'}
    logged = len(containers.THAW_LOG)
    try:
        table, sorted_ctg_list, RE_site_dict = R.parse_pickle(d['fa_dict'], pkl)
        assert sorted_ctg_list == sorted([(ctg, d['fa_dict'][ctg][1]) for ctg in d['fa_dict']], key=lambda x: x[1], reverse=True)
        assert RE_site_dict == d['RE_site_dict'] and type(table) is containers.LinkTable and len(table) == len(d['full_link_dict'])
        d['full_link_dict'], d['sorted_ctg_list'], d['RE_site_dict'] = table, sorted_ctg_list, RE_site_dict
        state = []
        rc.drive_rounds(R, d, after_call=lambda nround: state.append((nround, dict(d['ctg_group_dict']), dict(d['group_RE_dict']))))
        assert [s[0] for s in state] == case['nrounds'].tolist()
        for k, (nround, ctg_group, group_re) in enumerate(state):
            assert ctg_group == {d['names'][c]: (d['gnames'][g] if g >= 0 else 'ungrouped') for c, g in enumerate(case['groups'][k].tolist())}, nround
            assert group_re == dict(zip(d['gnames'], case['group_res'][k].tolist())), nround
        want_lines = ['Parsing input pickle file...']
        for nround, line in zip(case['nrounds'].tolist(), case['info'].tolist()):
            want_lines += ['Performing reassignment...' if nround else 'Performing additional round of rescue...', line]
        assert lines.lines == want_lines
        new_names = case['agg_names'].tolist()
        new_ctg_group_dict = {d['names'][c]: new_names[g] for c, g in enumerate(case['agg_group'].tolist()) if g >= 0}
        grouped_ctgs = {d['names'][c] for c in np.flatnonzero(case['agg_member']).tolist()}
        new_old_group_dict = {g: 'old_' + g for g in new_names}
        group_hiconf_RE_dict = {'old_' + g: int(v) for g, v in zip(new_names, case['agg_hiconf_re'].tolist())}
        monkeypatch.chdir(tmp_path)
        os.mkdir('hc_groups')
        R.agglomerative_hierarchical_clustering(table, grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict, int(case['agg_nclusters']))
        assert open('hc_groups/group_group_links.txt', 'rb').read() == case['agg_txt'].tobytes()
    finally:
        R.logger.removeHandler(lines)
    assert table.frozen is True and len(containers.THAW_LOG) == logged
    assert list(table.items()) == list(rc.case_dicts(case)['full_link_dict'].items()) and table.frozen is False


def test_the_golden_job_from_a_pkl_file_without_the_reference(tmp_path):
    """the same chain on the recorded rounds of tests/golden/reassign_rounds.npz: the groups, group_RE values and counts of every call"""
    case = rc.load_cases()['defaults']
    d = rc.case_dicts(case)
    from collections import defaultdict
    pkl = str(tmp_path / 'full_links.pkl')
    lp.write_python(defaultdict(int, d['full_link_dict']), pkl)
    i, j, value, is_float, names = _lib.read_link_pickle(pkl)
    assert is_float is None and names == list(dict.fromkeys(n for key in d['full_link_dict'] for n in key))
    ids = np.array([int(n[1:]) for n in names], np.int32)
    assert np.array_equal(ids[i], case['fi']) and np.array_equal(ids[j], case['fj']) and np.array_equal(value, case['links'])
    engine = _lib.Reassign(ids[i], ids[j], value, len(case['group0']), case['group0'], len(case['group_re0']))
    out = rc.run_job(case, engine)
    for k, (nround, group, group_re, counts) in enumerate(out):
        assert (group == case['groups'][k]).all() and (group_re == case['group_res'][k]).all() and counts.tolist() == case['counts'][k].tolist(), nround
