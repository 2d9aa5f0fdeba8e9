"""CPU: the parse_pickle seam of `haphic reassign` (HapHiC_reassign.py :38-50) with the host restatement of the reader (tests/link_pickle_cases.py
host_reader) as the stand-in engine.
  * the host reader on every accepted case, in Python's dialect and in the library's: arrays and names equal to the oracle's (pickle.load +
    cluster._dict_arrays); None for every hand-back case.  This pins the engine the mirror's tests lean on — and the grammar the device reader
    is tested against in tests/test_gpu_link_pickle.py;
  * the mirror: the reference's triple, a frozen table whose thaw is pickle.load's dict (order, Python int / float per key), pickle.load's own
    object or exception for the hand-backs;
  * both parse_link_dict mirrors answer "are the links integers" from a frozen table's arrays without thawing it;
  * where the reference checkout is present: the chain run() :824-896 walks from a .pkl file — parse_pickle, parse_link_dict, the rounds, the
    agglomerative step — through patch_reassign(R, rounds=True, pickle=True) with the host engines, against the unpatched functions: same dicts,
    log lines and file, no thaw, the table still frozen at the end."""
import logging
import os
import pickle
import sys
import types

import numpy as np
import pytest

from haphic_amd import cluster, containers, patch, reassign
from tests import link_pickle_cases as lp
from tests import reassign_cases as rc

REF = '/root/reference/scripts'
ACCEPTED = lp.accepted()
HANDED_BACK = lp.handed_back()


class _Module(types.SimpleNamespace):
    """what bind_pickle needs of HapHiC_reassign: its logger"""


def _stand_in():
    return _Module(logger=logging.getLogger('link_pickle_test'))


def _same_dict(a, b):
    assert list(a.items()) == list(b.items())
    assert [type(v) for v in a.values()] == [type(v) for v in b.values()]
    assert a.default_factory is b.default_factory


@pytest.mark.parametrize('name', sorted(ACCEPTED))
def test_host_reader_python_dialect(name, tmp_path):
    d = ACCEPTED[name]
    for protocol in (4, 5):
        path = str(tmp_path / ('p%d.pkl' % protocol))
        lp.write_python(d, path, protocol)
        lp.check_arrays(lp.host_reader(path), pickle.load(open(path, 'rb')))


@pytest.mark.parametrize('name', sorted(n for n, d in ACCEPTED.items() if lp.library_can_write(d)))
def test_host_reader_library_dialect(name, tmp_path):
    d = ACCEPTED[name]
    path = str(tmp_path / 'lib.pkl')
    lp.write_library(d, path)
    loaded = pickle.load(open(path, 'rb'))
    _same_dict(loaded, d)
    lp.check_arrays(lp.host_reader(path), loaded)


def test_the_cases_hold_what_they_are_named_for(tmp_path):
    import pickletools
    ops = {}
    for name in ('n1', 'n1001', 'frames', 'many_slots'):
        path = str(tmp_path / (name + '.pkl'))
        lp.write_python(ACCEPTED[name], path)
        ops[name] = [op.name for op, _arg, _pos in pickletools.genops(open(path, 'rb').read())]
    assert 'MARK' not in [op.name for op, _a, _p in pickletools.genops(pickle.dumps(ACCEPTED['n0'], 4))]
    assert ops['n1'].count('SETITEM') == 1 and 'SETITEMS' not in ops['n1']
    assert ops['n1001'].count('SETITEM') == 1 and ops['n1001'].count('SETITEMS') == 1
    assert ops['frames'].count('FRAME') >= 4 and 'BINGET' not in ops['frames']
    assert ops['many_slots'].count('MEMOIZE') > 65536 + 8 and 'LONG_BINGET' in ops['many_slots']
    path = str(tmp_path / 'lib.pkl')
    lp.write_library(ACCEPTED['many_slots'], path)
    data = open(path, 'rb').read()
    assert 'FRAME' not in {op.name for op, _a, _p in pickletools.genops(data)} and all(b'j' + int(s).to_bytes(4, 'little') in data for s in lp.SLOTS if s >= 256)


@pytest.mark.parametrize('name', ['full_links', 'HT_links'])
def test_host_reader_on_the_files_the_reference_wrote(name, tmp_path):
    import pickletools
    data = lp.golden()[name]
    ops = [op.name for op, _a, _p in pickletools.genops(data)]
    assert ops.count('FRAME') == 1 and 'BINGET' not in ops and ops.count('SHORT_BINUNICODE') == 4 + 2 * ops.count('TUPLE2')     # every name a literal again
    path = str(tmp_path / (name + '.pkl'))
    open(path, 'wb').write(data)
    loaded = pickle.load(open(path, 'rb'))
    assert len(loaded) > 80 and (name != 'HT_links' or all(n[-2:] in ('_H', '_T') for key in loaded for n in key))
    lp.check_arrays(lp.host_reader(path), loaded)


@pytest.mark.parametrize('name', sorted(HANDED_BACK))
def test_host_reader_hands_back(name, tmp_path):
    path = str(tmp_path / 'x.pkl')
    open(path, 'wb').write(HANDED_BACK[name])
    assert lp.host_reader(path) is None


@pytest.mark.parametrize('name', sorted(ACCEPTED))
def test_mirror_returns_the_reference_triple_and_thaws_into_the_loaded_dict(name, tmp_path):
    d = ACCEPTED[name]
    path = str(tmp_path / 'full_links.pkl')
    lp.write_python(d, path)
    fa_dict = {'c%d' % k: [None, 1000 + (k * 37) % 11, k + 1] for k in range(30)}
    parse_pickle = reassign.bind_pickle(_stand_in(), lp.host_reader)
    table, sorted_ctg_list, RE_site_dict = parse_pickle(fa_dict, path)
    assert sorted_ctg_list == sorted([(ctg, fa_dict[ctg][1]) for ctg in fa_dict], key=lambda x: x[1], reverse=True)
    assert RE_site_dict == {ctg: info[2] for ctg, info in fa_dict.items()} and list(RE_site_dict) == list(fa_dict)
    assert type(table) is containers.LinkTable and table.frozen is True and len(table) == len(d)
    integral = all(type(v) is int for v in d.values())
    assert cluster.integral_links(table) is integral and table.frozen is True
    logged = len(containers.THAW_LOG)
    table[('no', 'such key')]                                              # any dict access thaws
    del table[('no', 'such key')]
    assert table.frozen is False and len(containers.THAW_LOG) == logged + 1
    _same_dict(table, pickle.load(open(path, 'rb')))


@pytest.mark.parametrize('name', sorted(HANDED_BACK))
def test_mirror_gives_what_pickle_load_gives_for_a_hand_back(name, tmp_path):
    path = str(tmp_path / 'x.pkl')
    open(path, 'wb').write(HANDED_BACK[name])
    kind, want = lp.load_or_error(HANDED_BACK[name])
    parse_pickle = reassign.bind_pickle(_stand_in(), lp.host_reader)
    if kind == 'error':
        with pytest.raises(want):
            parse_pickle({}, path)
        return
    got = parse_pickle({}, path)[0]
    assert type(got) is type(want) and list(got.items()) == list(want.items()) and [type(v) for v in got.values()] == [type(v) for v in want.values()]


def test_the_log_line(tmp_path, caplog):
    path = str(tmp_path / 'x.pkl')
    lp.write_python(ACCEPTED['n2'], path)
    with caplog.at_level(logging.INFO, logger='link_pickle_test'):
        reassign.bind_pickle(_stand_in(), lp.host_reader)({}, path)
    assert [r.getMessage() for r in caplog.records] == ['Parsing input pickle file...']


def test_tables_of_real_dicts_still_answer_as_before():
    assert cluster.integral_links({('a', 'b'): 1, ('a', 'c'): np.int64(2)}) is True
    assert cluster.integral_links({('a', 'b'): 1, ('a', 'c'): 2.0}) is False
    assert cluster.integral_links({}) is True


# ------------------------------------------------------------------ the chain of run() from a .pkl file, against the unpatched reference
def _reference():
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import HapHiC_reassign as R
    return R


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def job_from_pickle(R, case, pkl, nclusters, tmp):
    """run() :824 and :855-896 through the names R holds, full_link_dict from parse_pickle(fa_dict, pkl) -> (what it leaves behind, full_link_dict)"""
    d = rc.case_dicts(case)
    lines = _Lines()
    R.logger.addHandler(lines)
    level = R.logger.level
    R.logger.setLevel(logging.INFO)
    here = os.getcwd()
    os.makedirs(tmp)
    os.chdir(tmp)
    try:
        d['full_link_dict'], d['sorted_ctg_list'], d['RE_site_dict'] = R.parse_pickle(d['fa_dict'], pkl)
        rc.drive_rounds(R, d)
        os.mkdir('reassigned_groups')
        group_ctg_dict, group_hiconf_RE_dict = R.stat_clusters(d['ctg_group_dict'], d['fa_dict'], d['grouped_ctgs'])
        new_ctg_group_dict, new_group_ctg_dict, new_old_group_dict = R.clusters_output(group_ctg_dict, d['fa_dict'], 'reassigned')
        assert nclusters < len(new_group_ctg_dict)
        os.mkdir('hc_groups')
        hc = R.agglomerative_hierarchical_clustering(d['full_link_dict'], d['grouped_ctgs'], new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict,
                                                     nclusters, normalize_by_nlinks=False)
        files = {}
        for sub in ('reassigned_groups', 'hc_groups'):
            for f in sorted(os.listdir(sub)):
                files[sub + '/' + f] = open(os.path.join(sub, f), 'rb').read()
    finally:
        os.chdir(here)
        R.logger.removeHandler(lines)
        R.logger.setLevel(level)
    out = dict(ctg_group=list(d['ctg_group_dict'].items()), group_re=list(d['group_RE_dict'].items()), lines=lines.lines, files=files,
               sorted_ctg_list=d['sorted_ctg_list'], re_sites=list(d['RE_site_dict'].items()), hc=sorted(sorted(v) for v in hc.values()))
    return out, d['full_link_dict']


def write_case_pickle(case, path, library):
    d = rc.case_dicts(case)
    table = defaultdict_of(d['full_link_dict'])
    if library:
        lp.write_library(table, path)
    else:
        lp.write_python(table, path)


def defaultdict_of(link_dict):
    from collections import defaultdict
    return defaultdict(int, link_dict)


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
@pytest.mark.parametrize('library', [False, True], ids=['python_dialect', 'library_dialect'])
def test_the_chain_of_run_from_a_pkl_file_never_thaws(library, tmp_path):
    R = _reference()
    case = rc.load_cases()['defaults']
    pkl = str(tmp_path / 'full_links.pkl')
    write_case_pickle(case, pkl, library)
    theirs, their_dict = job_from_pickle(R, case, pkl, 2, str(tmp_path / 'theirs'))
    assert type(their_dict).__name__ == 'defaultdict' and theirs['lines'][0] == 'Parsing input pickle file...'
    logged = len(containers.THAW_LOG)
    saved = patch.patch_reassign(R, rounds=True, engine=rc.NumpyReassign, pickle=True, pickle_engine=lp.host_reader)
    try:
        assert set(saved) == {'parse_link_dict', 'split_clm_file', 'run_reassignment', 'agglomerative_hierarchical_clustering', 'parse_pickle'}
        ours, table = job_from_pickle(R, case, pkl, 2, str(tmp_path / 'ours'))
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)
    assert ours == theirs
    assert type(table) is containers.LinkTable and table.frozen is True and len(containers.THAW_LOG) == logged
    assert list(table.items()) == list(their_dict.items()) and table.frozen is False


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_without_pickle_the_reference_function_stays_bound():
    R = _reference()
    original = R.parse_pickle
    saved = patch.patch_reassign(R, rounds=True, engine=rc.NumpyReassign)
    try:
        assert R.parse_pickle is original and 'parse_pickle' not in saved
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)
