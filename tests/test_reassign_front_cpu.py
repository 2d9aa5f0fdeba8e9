"""CPU: the front of `haphic reassign` — parse_fasta and the data preparation of parse_link_dict — through the host engines of
tests/reassign_front_cases.py.
  * containers.FastaRow against a plain list, operation by operation, with the number of fetches;
  * reassign.bind_fasta against tests/golden/reassign_front.npz (the reference's own parse_fasta wrote it) and, where the checkout is present,
    against the reference's function itself; refused files reach the original function; no sequence is fetched;
  * the resident branch of parse_link_dict against today's path: cells, thawed tables and the first round equal, no key copied to the host; every
    refusal lands on today's path with today's result;
  * where the reference is present: run() on a toy job with every seam of the front bound, against the unpatched module, file by file and log line
    by log line."""
import copy
import logging
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest

from haphic_amd import cluster, containers, patch, reassign
from tests import link_pickle_cases as lp
from tests import oracle_lib
from tests import reassign_cases as rc
from tests import reassign_front_cases as fc

REF = '/root/reference/scripts'
HAVE_REF = os.path.isdir(REF)
needs_reference = pytest.mark.skipif(not HAVE_REF, reason='reference checkout not present')
FASTA = fc.fasta_cases()
ACCEPTED = lp.accepted()
INTEGRAL = sorted(n for n, d in ACCEPTED.items() if all(type(v) is int for v in d.values()))


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(cluster, '_lib', oracle_lib)            # cluster.parse_link_dict's group_link_sums without a GPU
    return cluster


_PRIVATE = []


def _reference():
    """HapHiC_reassign.py under a private module name, with modules of its own behind its imports: the `HapHiC_reassign` other test files share
    may still carry their seams"""
    if _PRIVATE:
        return _PRIVATE[0]
    import importlib.util
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    shared = {k: sys.modules.pop(k) for k in list(sys.modules) if k.startswith('HapHiC_') or k == '_version'}
    spec = importlib.util.spec_from_file_location('_haphic_reassign_front_private', os.path.join(REF, 'HapHiC_reassign.py'))
    R = importlib.util.module_from_spec(spec)
    sys.path.insert(0, REF)
    try:
        spec.loader.exec_module(R)
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k.startswith('HapHiC_') or k == '_version']:
            del sys.modules[k]
        sys.modules.update(shared)
    _PRIVATE.append(R)
    return R


def _refuses(what):
    def fn(*_args, **_kwargs):
        raise AssertionError('handed to the reference: ' + what)
    return fn


def _module():
    """HapHiC_reassign where it is present, else what the mirrors need of it: a logger and originals that must not be reached"""
    if HAVE_REF:
        return _reference()
    return types.SimpleNamespace(logger=logging.getLogger('reassign_front_test'), parse_link_dict=_refuses('parse_link_dict'),
                                 run_reassignment=_refuses('run_reassignment'), agglomerative_hierarchical_clustering=_refuses('agglomerative'),
                                 parse_fasta=_refuses('parse_fasta'))


# ------------------------------------------------------------------ 1. FastaRow
class _Source:
    def __init__(self):
        self.calls = []

    def __call__(self, key):
        self.calls.append(key)
        return 'ACGTNacgt'


PLAIN = ['ACGTNacgt', 9, 3]
QUIET = [('row[1]', lambda r: r[1]), ('row[2]', lambda r: r[2]), ('row[-1]', lambda r: r[-1]), ('row[-2]', lambda r: r[-2]), ('len', len),
         ('row[1:]', lambda r: r[1:]), ('row[-2:]', lambda r: r[-2:]), ('row[2:0:-1]', lambda r: r[2:0:-1]), ('row[3:]', lambda r: r[3:]),
         ('bool', bool)]
LOUD = [('row[0]', lambda r: r[0]), ('row[-3]', lambda r: r[-3]), ('row[:]', lambda r: r[:]), ('row[:2]', lambda r: r[:2]), ('row[::-1]', lambda r: r[::-1]),
        ('row[::2]', lambda r: r[::2]), ('iter', lambda r: list(iter(r))), ('unpack', lambda r: (lambda a, b, c: (a, b, c))(*r)),
        ('tuple', tuple), ('reversed', lambda r: list(reversed(r))),
        ('eq', lambda r: r == PLAIN), ('eq_reflected', lambda r: PLAIN == r), ('ne', lambda r: r != PLAIN), ('lt', lambda r: r < ['B', 0, 0]),
        ('repr', repr), ('str', str), ('copy.copy', copy.copy), ('copy', lambda r: r.copy()), ('deepcopy', copy.deepcopy),
        ('pickle', lambda r: pickle.loads(pickle.dumps(r))), ('pickle2', lambda r: pickle.loads(pickle.dumps(r, 2))),
        ('contains', lambda r: 'ACGTNacgt' in r), ('index', lambda r: r.index(9)), ('count', lambda r: r.count('ACGTNacgt')),
        ('add', lambda r: r + [1]), ('radd', lambda r: [1] + r), ('mul', lambda r: r * 2), ('join', lambda r: ''.join(r[:1])),
        ('sorted_key', lambda r: sorted(r, key=str))]
MUTATING = [('sort', lambda r: r.sort(key=str)), ('reverse', lambda r: r.reverse()), ('append', lambda r: r.append(4)), ('extend', lambda r: r.extend([4, 5])),
            ('insert', lambda r: r.insert(0, 'x')), ('pop', lambda r: r.pop()), ('pop0', lambda r: r.pop(0)), ('remove', lambda r: r.remove(9)),
            ('clear', lambda r: r.clear()), ('del0', lambda r: r.__delitem__(0)), ('del2', lambda r: r.__delitem__(2)), ('iadd', lambda r: r.__iadd__([7])),
            ('imul', lambda r: r.__imul__(2)), ('slice_assign', lambda r: r.__setitem__(slice(0, 2), ['x', 'y', 'z']))]


def _row():
    src = _Source()
    return containers.FastaRow(src, 17, 9, 3), src


@pytest.mark.parametrize('name,op', QUIET, ids=[n for n, _ in QUIET])
def test_row_answers_without_a_fetch(name, op):
    row, src = _row()
    got, want = op(row), op(list([None, 9, 3]))
    assert got == want and type(got) is type(want) and src.calls == []


@pytest.mark.parametrize('name,op', LOUD, ids=[n for n, _ in LOUD])
def test_row_fetches_once_when_element_0_is_observed(name, op):
    row, src = _row()
    assert src.calls == []
    got, want = op(row), op(list(PLAIN))
    assert got == want and type(got) is type(want) and src.calls == [17]
    assert op(row) == want and list(row) == PLAIN and src.calls == [17]


@pytest.mark.parametrize('name,op', MUTATING, ids=[n for n, _ in MUTATING])
def test_row_changes_like_a_list(name, op):
    row, src = _row()
    plain = list(PLAIN)
    assert op(row) == op(plain) or name in ('iadd', 'imul')
    assert list(row) == plain and len(row) == len(plain) and src.calls == [17]


ROW_PAIRS = [('eq', lambda a, b: a == b), ('ne', lambda a, b: a != b), ('lt', lambda a, b: a < b), ('le', lambda a, b: a <= b), ('gt', lambda a, b: a > b),
             ('ge', lambda a, b: a >= b), ('add', lambda a, b: a + b), ('iadd', lambda a, b: a.__iadd__(b)), ('extend', lambda a, b: a.extend(b) or a),
             ('nested_eq', lambda a, b: [a] == [b]), ('dict_eq', lambda a, b: {'c': a} == {'c': b}), ('sorted', lambda a, b: sorted([b, a])),
             ('contains', lambda a, b: a in [b]), ('index', lambda a, b: [0, b, a].index(a)), ('count', lambda a, b: [a, b].count(a)),
             ('contains_row', lambda a, b: (a.append(b), b in a)[1]), ('index_row', lambda a, b: (a.append(b), a.index(b))[1]),
             ('count_row', lambda a, b: (a.append(b), a.count(b))[1]), ('remove_row', lambda a, b: (a.append(b), a.remove(b), a)[2]),
             ('slice_assign', lambda a, b: a.__setitem__(slice(1, 1), b) or a), ('min', lambda a, b: min(a, b)), ('max', lambda a, b: max(b, a))]


def _two_rows(second):
    sources = {17: 'ACGTNacgt', 18: second}
    calls = []

    def fetch(key):
        calls.append(key)
        return sources[key]
    return containers.FastaRow(fetch, 17, 9, 3), containers.FastaRow(fetch, 18, 9, 3), calls


@pytest.mark.parametrize('second', ['ACGTNacgt', 'ACGA', 'TTTT'], ids=['same', 'smaller', 'larger'])
@pytest.mark.parametrize('name,op', ROW_PAIRS, ids=[n for n, _ in ROW_PAIRS])
def test_row_against_row(name, op, second):
    a, b, calls = _two_rows(second)
    got, want = op(a, b), op(list(PLAIN), [second, 9, 3])
    assert got == want and type(got) in (type(want), containers.FastaRow) and sorted(calls) == [17, 18]
    assert list(a)[:3] == PLAIN or name in ('slice_assign',)
    assert list(b) == [second, 9, 3]


def test_row_assignment():
    row, src = _row()
    row[1] = 10
    row[-1] = 4
    assert src.calls == [] and row[1:] == [10, 4]
    row[0] = None                                                    # replaced unseen: nothing to fetch any more
    assert list(row) == [None, 10, 4] and src.calls == []
    row, src = _row()
    row[-3] = 'TT'
    assert row == ['TT', 9, 3] and src.calls == []
    row, src = _row()
    assert row[0] == 'ACGTNacgt'
    row[0] = 'A'
    assert row == ['A', 9, 3] and src.calls == [17]
    assert type(pickle.loads(pickle.dumps(_row()[0]))) is list and type(copy.copy(_row()[0])) is list


# ------------------------------------------------------------------ 2. bind_fasta
GOLDEN_TABLES, GOLDEN_SEQS = fc.golden()


def _bound(engine, original=None):
    R = types.SimpleNamespace(logger=logging.getLogger('reassign_front_test'), parse_fasta=original or _refuses('parse_fasta'))
    return reassign.bind_fasta(R, engine)


@pytest.mark.parametrize('keep', [False, True], ids=['upper', 'keep_case'])
@pytest.mark.parametrize('case', [c for c in FASTA if not c[2]], ids=[c[0] for c in FASTA if not c[2]])
def test_bind_fasta_against_the_reference_result(case, keep, tmp_path, caplog):
    name, text, _refused = case
    path = str(tmp_path / 'asm.fa')
    open(path, 'wb').write(text)
    for RE in fc.RES:
        Engine = fc.fasta_engine()
        log = logging.getLogger('reassign_front_test.fasta')
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=log.name):
            fa_dict = _bound(Engine)(path, RE=RE, keep_letter_case=keep, logger=log)
        assert [r.getMessage() for r in caplog.records] == ['Parsing input FASTA file...']
        names, lengths, re_sites = GOLDEN_TABLES[(name, keep, RE)]
        assert type(fa_dict) is dict and list(fa_dict) == names
        assert [fa_dict[c][1] for c in fa_dict] == lengths and [info[2] for info in fa_dict.values()] == re_sites
        assert all(type(v) is containers.FastaRow and len(v) == 3 for v in fa_dict.values())
        assert all(type(v[1]) is int and type(v[2]) is int for v in fa_dict.values())
        assert Engine.fetched == [] and Engine.count_calls == ([len(names)] if names else [])
        if (name, keep) in GOLDEN_SEQS:
            assert ''.join(v[0] for v in fa_dict.values()) == GOLDEN_SEQS[(name, keep)]
            assert [len(v[0]) for v in fa_dict.values()] == lengths and len(Engine.fetched) == len(names)


@needs_reference
@pytest.mark.parametrize('case', FASTA, ids=[c[0] for c in FASTA])
def test_bind_fasta_against_the_reference_function(case, tmp_path):
    name, text, refused = case
    R = _reference()
    path = str(tmp_path / 'asm.fa')
    open(path, 'wb').write(text)
    Engine = fc.fasta_engine()
    ours = reassign.bind_fasta(R, Engine)
    for RE in fc.RES[:2]:
        for keep in (False, True):
            try:
                want = R.parse_fasta(path, RE=RE, keep_letter_case=keep)
            except Exception as e:      # noqa: BLE001 — the reference's own answer
                with pytest.raises(type(e)):
                    ours(path, RE=RE, keep_letter_case=keep)
                continue
            got = ours(path, RE=RE, keep_letter_case=keep)
            assert Engine.fetched == [] or refused
            assert type(got) is dict and list(got.items()) == list(want.items())
            if not refused:
                Engine.fetched.clear()


@pytest.mark.parametrize('case', [c for c in FASTA if c[2]], ids=[c[0] for c in FASTA if c[2]])
def test_refused_files_reach_the_original_function(case, tmp_path):
    _name, text, _refused = case
    path = str(tmp_path / 'asm.fa')
    open(path, 'wb').write(text)
    calls = []

    def original(fasta, RE, keep_letter_case, logger):
        calls.append((fasta, RE, keep_letter_case, logger))
        return 'the reference result'
    log = logging.getLogger('reassign_front_test.fasta')
    assert _bound(fc.fasta_engine(), original)(path, RE='GCGC', keep_letter_case=True, logger=log) == 'the reference result'
    assert calls == [(path, 'GCGC', True, log)]


def test_a_path_that_is_no_file_reaches_the_original_function(tmp_path):
    def original(fasta, RE, keep_letter_case, logger):
        return open(fasta)
    with pytest.raises(FileNotFoundError):
        _bound(fc.fasta_engine(), original)(str(tmp_path / 'no_such.fa'))


def test_patch_reassign_binds_the_fasta_seam_only_when_asked():
    R = _module()
    before = R.parse_fasta
    saved = patch.patch_reassign(R, rounds=True, engine=fc.HostReassign, pickle=True, pickle_engine=fc.HostLinkPickle.open, resident=True)
    try:
        assert 'parse_fasta' not in saved and R.parse_fasta is before
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)
    saved = patch.patch_reassign(R, fasta=True, fasta_engine=fc.fasta_engine())
    try:
        assert set(saved) == {'parse_link_dict', 'split_clm_file', 'parse_fasta'} and R.parse_fasta is not before and saved['parse_fasta'] is before
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)


# ------------------------------------------------------------------ 3. the resident branch of parse_link_dict
def _write(d, path, library):
    (lp.write_library if library else lp.write_python)(d, path)


def _parse(R, path, ctg_group_dict, resident, normalize_by_nlinks=False):
    """parse_pickle + parse_link_dict through fresh mirrors -> (tables, session or None, full_link_dict)"""
    engine = fc.HostLinkPickle.open if resident else lp.host_reader
    parse_pickle = reassign.bind_pickle(R, engine, resident) if resident else reassign.bind_pickle(R, engine)
    mirrors = reassign.bind_rounds(R, fc.HostReassign)
    table = parse_pickle({}, path)[0]
    session = table._session                                        # (a thaw drops the attribute)
    tables = mirrors['parse_link_dict'](table, ctg_group_dict, normalize_by_nlinks)
    return tables, session, table, mirrors


def _one_round(R, mirrors, tables, table, ctg_group_dict, caplog):
    """the first round over copies of the dicts -> (groups, group_RE, log lines)"""
    fa_dict, re_sites, sorted_ctg_list, group_re = fc.round_inputs(ctg_group_dict)
    groups = dict(ctg_group_dict)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=R.logger.name):
        mirrors['run_reassignment'](sorted_ctg_list, tables[0], groups, table, tables[1], fa_dict, re_sites, None, group_re, 10000, 5, 1, 0.0001, 1.2, 0.8,
                                    0, set(), 1)
    return list(groups.items()), list(group_re.items()), [r.getMessage() for r in caplog.records]


def _dump(tables):
    return ([(c, list(inner.items())) for c, inner in tables[0].items()], [(c, sorted(s)) for c, s in tables[1].items()])


def _written(name, library, tmp_path):
    d = ACCEPTED[name]
    if library and not lp.library_can_write(d):
        pytest.skip('not a table the library writes')
    path = str(tmp_path / 'full_links.pkl')
    _write(d, path, library)
    return d, path


@pytest.mark.parametrize('library', [False, True], ids=['python_dialect', 'library_dialect'])
@pytest.mark.parametrize('name', [n for n in INTEGRAL if n not in ('values', 'straddle', 'n0')])
def test_resident_branch_equals_todays_path(name, library, tmp_path, caplog, host_only):
    d, path = _written(name, library, tmp_path)
    names = {}
    cluster._dict_arrays(d, names)
    ctg_group_dict = fc.grouping(names)
    R = _module()
    ours, session, table, mirrors = _parse(R, path, ctg_group_dict, True)
    theirs, _s, their_table, their_mirrors = _parse(R, path, ctg_group_dict, False)
    assert type(ours[0]) is reassign.RoundTable and type(theirs[0]) is reassign.RoundTable
    assert session.resident and session.fetches == 0 and session.handle.key_fetches == 0 and table.frozen is True
    job, their_job = ours[0]._job, theirs[0]._job
    assert job.id_names == their_job.id_names and job.group_names == their_job.group_names and type(job.engine) is fc.HostReassign
    for a, b in zip(job.engine.cells(), their_job.engine.cells()):
        assert np.array_equal(a, b)
    got = _one_round(R, mirrors, ours, table, ctg_group_dict, caplog)
    assert got == _one_round(R, their_mirrors, theirs, their_table, ctg_group_dict, caplog)
    assert 'Total: %d' % len(ctg_group_dict) in got[2][-1]
    assert session.fetches == 0 and len(table) == len(d) and table.frozen is True
    # a second pair, thawed before any round: the reference's containers, and the one copy of the keys that takes
    ours, session, table, _m = _parse(R, path, ctg_group_dict, True)
    theirs, _s, _t, _m = _parse(R, path, ctg_group_dict, False)
    assert _dump(ours) == _dump(theirs) and type(ours[0]).__name__ == 'Thawed'
    assert session.fetches == 1 and table.frozen is True
    assert list(table.items()) == list(d.items()) and session.fetches == 1 and session.handle is None


def _expect_todays_path(R, path, ctg_group_dict, flags, host_only, normalize_by_nlinks=False):
    fc.HostReassign.REFUSALS.clear()
    ours, session, _table, _m = _parse(R, path, ctg_group_dict, True, normalize_by_nlinks)
    theirs, _s, _t, _m = _parse(R, path, ctg_group_dict, False, normalize_by_nlinks)
    assert [w for w, _why in fc.HostReassign.REFUSALS] == ([flags] if flags else [])
    assert type(ours[0]) is type(theirs[0])
    if type(ours[0]) is reassign.RoundTable:                        # today's path builds its handle from the arrays on the host
        assert session.fetches == 1
        for a, b in zip(ours[0]._job.engine.cells(), theirs[0]._job.engine.cells()):
            assert np.array_equal(a, b)
    assert _dump(ours) == _dump(theirs)
    return session


@pytest.mark.parametrize('library', [False, True], ids=['python_dialect', 'library_dialect'])
@pytest.mark.parametrize('name', ['values', 'straddle'])
def test_accepted_files_the_key_pass_refuses_land_on_todays_path(name, library, tmp_path, host_only):
    """negative values and totals beyond 2^52 among the accepted files of tests/link_pickle_cases.py"""
    d, path = _written(name, library, tmp_path)
    assert min(d.values()) < 0 and 2 * sum(v for v in d.values() if v > 0) >= 2 ** 53
    names = {}
    cluster._dict_arrays(d, names)
    _expect_todays_path(_module(), path, fc.grouping(names), fc.HostReassign.NEGATIVE | fc.HostReassign.TOTAL, host_only)


@pytest.mark.parametrize('library', [False, True], ids=['python_dialect', 'library_dialect'])
def test_resident_branch_on_a_table_without_a_key(library, tmp_path, caplog, host_only):
    d, path = _written('n0', library, tmp_path)
    assert len(d) == 0
    R = _module()
    ours, session, table, mirrors = _parse(R, path, GROUPS, True)
    theirs, _s, their_table, their_mirrors = _parse(R, path, GROUPS, False)
    assert type(ours[0]) is reassign.RoundTable and type(theirs[0]) is reassign.RoundTable and session.fetches == 0
    assert ours[0]._job.id_names == theirs[0]._job.id_names == list(GROUPS)
    for a, b in zip(ours[0]._job.engine.cells(), theirs[0]._job.engine.cells()):
        assert np.array_equal(a, b) and a.shape == (6, 2)
    got = _one_round(R, mirrors, ours, table, GROUPS, caplog)
    assert got == _one_round(R, their_mirrors, theirs, their_table, GROUPS, caplog) and 'not rescued: 6' in got[2][-1]
    assert session.fetches == 0


def _table_file(tmp_path, items):
    from collections import defaultdict
    path = str(tmp_path / 'full_links.pkl')
    lp.write_python(defaultdict(int, items), path)
    return path


BASE = {('a', 'b'): 5, ('b', 'c'): 7, ('a', 'd'): 2, ('e', 'c'): 1}
GROUPS = {'a': 'g1', 'b': 'g1', 'c': 'g2', 'd': 'ungrouped', 'e': 'g2', 'f': 'g1'}


@pytest.mark.parametrize('extra,flags', [({('c', 'c'): 3}, fc.HostReassign.SELF_KEY), ({('d', 'e'): -4}, fc.HostReassign.NEGATIVE),
                                         ({('d', 'e'): 2 ** 52 - 15}, fc.HostReassign.TOTAL), ({('d', 'e'): 2 ** 62, ('a', 'e'): 2 ** 62, ('f', 'e'): 2 ** 62,
                                                                                                ('f', 'a'): 2 ** 62}, fc.HostReassign.TOTAL)],
                         ids=['key_names_one_contig_twice', 'negative_value', 'total_reaches_2_52', 'total_beyond_2_64'])
def test_refusals_of_the_key_pass_land_on_todays_path(extra, flags, tmp_path, host_only):
    path = _table_file(tmp_path, {**BASE, **extra})
    _expect_todays_path(_module(), path, GROUPS, flags, host_only)


def test_total_below_2_52_is_served(tmp_path, host_only):
    path = _table_file(tmp_path, {**BASE, ('d', 'e'): 2 ** 52 - 16})
    ours, session, _t, _m = _parse(_module(), path, GROUPS, True)
    assert type(ours[0]) is reassign.RoundTable and session.fetches == 0


def test_a_name_missing_from_ctg_group_dict_lands_on_todays_path(tmp_path, host_only):
    path = _table_file(tmp_path, BASE)
    groups = {c: g for c, g in GROUPS.items() if c != 'e'}
    R = _module()
    fc.HostReassign.REFUSALS.clear()
    parse_pickle = reassign.bind_pickle(R, fc.HostLinkPickle.open, True)
    with pytest.raises(KeyError):                                   # today's answer: cluster.parse_link_dict asks ctg_group_dict for it
        reassign.bind_rounds(R, fc.HostReassign)['parse_link_dict'](parse_pickle({}, path)[0], groups)
    assert fc.HostReassign.REFUSALS == []


@needs_reference
@pytest.mark.parametrize('what', ['float_value', 'no_grouped_contig', 'normalize_by_nlinks'])
def test_cases_of_the_reference_function_still_reach_it(what, tmp_path, host_only):
    items = {**BASE, ('d', 'e'): 0.5} if what == 'float_value' else BASE
    groups = {c: 'ungrouped' for c in GROUPS} if what == 'no_grouped_contig' else GROUPS
    path = _table_file(tmp_path, items)
    session = _expect_todays_path(_reference(), path, groups, 0, host_only, normalize_by_nlinks=what == 'normalize_by_nlinks')
    assert (type(session) is reassign.PickleSession) is (what == 'float_value')


def _recording_module():
    calls = []

    def parse_link_dict(link_dict, ctg_group_dict, normalize_by_nlinks=False):
        calls.append((type(link_dict).__name__, list(link_dict.items()), [type(v) for v in link_dict.values()], dict(ctg_group_dict), normalize_by_nlinks))
        return 'the reference result'
    R = types.SimpleNamespace(logger=logging.getLogger('reassign_front_test'), parse_link_dict=parse_link_dict, run_reassignment=_refuses('run_reassignment'),
                              agglomerative_hierarchical_clustering=_refuses('agglomerative'))
    return R, calls


@pytest.mark.parametrize('what', ['float_value', 'no_grouped_contig', 'normalize_by_nlinks'])
def test_cases_of_the_reference_function_reach_a_stand_in_for_it(what, tmp_path, host_only):
    """the same three without the checkout: the original function is called once, with the same arguments, whether the keys are resident or not"""
    items = {**BASE, ('d', 'e'): 0.5} if what == 'float_value' else BASE
    groups = {c: 'ungrouped' for c in GROUPS} if what == 'no_grouped_contig' else GROUPS
    path = _table_file(tmp_path, items)
    seen = []
    for resident in (True, False):
        R, calls = _recording_module()
        fc.HostReassign.REFUSALS.clear()
        tables, session, _table, _m = _parse(R, path, groups, resident, normalize_by_nlinks=what == 'normalize_by_nlinks')
        assert tables == 'the reference result' and len(calls) == 1 and fc.HostReassign.REFUSALS == []
        assert calls[0][1] == list(items.items()) and calls[0][2] == [type(v) for v in items.values()]
        seen.append(calls[0])
    assert seen[0] == seen[1]


def test_cells_beyond_the_device_go_straight_to_the_original_function(tmp_path, host_only):
    """HHX_UNSUPPORTED from from_pickle: the call the host passes would end in, without copying a key first"""
    class Engine(fc.HostReassign):
        class Unsupported(RuntimeError):
            pass

        def __init__(self, *args):
            raise Engine.Unsupported('two tables of n_ctg * n_groups cells')

        @classmethod
        def from_pickle(cls, link_pickle, n_ctg, group, n_groups):
            raise Engine.Unsupported('two tables of n_ctg * n_groups cells')
    path = _table_file(tmp_path, BASE)
    seen = []
    for resident in (True, False):
        R, calls = _recording_module()
        opener = fc.HostLinkPickle.open if resident else lp.host_reader
        table = (reassign.bind_pickle(R, opener, True) if resident else reassign.bind_pickle(R, opener))({}, path)[0]
        session = table._session
        assert reassign.bind_rounds(R, Engine)['parse_link_dict'](table, GROUPS) == 'the reference result'
        seen.append(calls)
        assert len(calls) == 1 and (session.fetches == 1 if resident else True)      # (the one copy: the stand-in original reads the dict)
    assert seen[0] == seen[1]


def test_n_keys_any_float_and_names_without_the_keys(tmp_path):
    d, path = _written('shared_and_fresh', False, tmp_path)
    R = _module()
    table = reassign.bind_pickle(R, fc.HostLinkPickle.open, True)({}, path)[0]
    session = table._session
    assert len(table) == len(d) and bool(table) and session.any_float is False and session.n_keys('full') == len(d)
    names = {}
    cluster._dict_arrays(d, names)
    assert session.names == list(names) and session.fetches == 0 and session.handle.key_fetches == 0
    assert cluster.integral_links(table) is True and session.fetches == 1
    i, j, v, table_names = table.arrays()
    assert session.fetches == 1 and v.dtype == np.int64 and table_names == list(names)
    _d, path = _written('floats', False, tmp_path)
    assert type(reassign.bind_pickle(R, fc.HostLinkPickle.open, True)({}, path)[0]._session) is reassign.PickleSession


# ------------------------------------------------------------------ 4. run() on a toy job
def _toy_job(directory):
    """FASTA, full_links.pkl, a clusters file and a CLM for HapHiC_reassign.run -> the argv of `haphic reassign`"""
    from collections import defaultdict
    fi, fj, links, group, _ctg_re, _len = rc.build_case(601, 4, 40, 0.35, 0.04, 0.2)
    rng = np.random.default_rng(8)
    names = ['ctg%03d' % k for k in range(len(group))]
    fasta = os.path.join(directory, 'asm.fa')
    with open(fasta, 'wb') as f:
        for k, n in enumerate(names):
            f.write(b'>' + n.encode() + b' len\n' + fc.bc.wrap(fc.bc.bases(rng, int(rng.integers(2000, 9000)), b'ACGTacgtN'), 60))
    table = defaultdict(int)
    for a, b, v in zip(fi.tolist(), fj.tolist(), links.tolist()):
        table[(names[a], names[b])] = int(v)
    pkl = os.path.join(directory, 'full_links.pkl')
    lp.write_python(table, pkl)
    clusters = os.path.join(directory, 'inflation_1.1.clusters.txt')
    with open(clusters, 'w') as f:
        f.write('#Group\tnContigs\tContigs\n')
        for g in range(4):
            members = [names[k] for k in np.flatnonzero(group == g).tolist()]
            f.write('group%d\t%d\t%s\n' % (g + 1, len(members), ' '.join(members)))
    clm = os.path.join(directory, 'paired_links.clm')
    with open(clm, 'w') as f:
        for a, b, v in zip(fi.tolist()[:400], fj.tolist()[:400], links.tolist()[:400]):
            for o in ('++', '+-', '-+', '--'):
                f.write('%s%s %s%s\t%d\t%s\n' % (names[a], o[0], names[b], o[1], v, ' '.join(str(100 + 7 * q) for q in range(v))))
    return [fasta, pkl, clusters, clm, '--nclusters', '3', '--min_group_len', '0', '--min_RE_sites', '5', '--min_links', '5']


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _run(R, argv, directory, monkeypatch):
    os.makedirs(directory)
    lines = _Lines()
    loggers = [R.logger, logging.getLogger('HapHiC_cluster'), reassign.logger]
    loggers = list({id(x): x for x in loggers}.values())
    levels = [x.level for x in loggers]
    for x in loggers:
        x.addHandler(lines)
        x.setLevel(logging.INFO)
    monkeypatch.setattr(sys, 'argv', ['haphic reassign'] + argv)
    here = os.getcwd()
    os.chdir(directory)
    try:
        R.run(R.parse_arguments())
    finally:
        os.chdir(here)
        for x, level in zip(loggers, levels):
            x.removeHandler(lines)
            x.setLevel(level)
    files = {}
    for root, _dirs, names in os.walk(directory):
        for n in names:
            p = os.path.join(root, n)
            files[os.path.relpath(p, directory)] = os.readlink(p) if os.path.islink(p) else open(p, 'rb').read()
    return files, [re.sub(r'\d+(\.\d+)?(e-?\d+)?s\b', '<t>s', line) for line in lines.lines]


@needs_reference
def test_run_on_a_toy_job_against_the_unpatched_module(tmp_path, monkeypatch, host_only):
    R = _reference()
    argv = _toy_job(str(tmp_path))
    theirs = _run(R, argv, str(tmp_path / 'theirs'), monkeypatch)
    assert 'final_groups/final_clusters.txt' in theirs[0] and any(f.startswith('split_clms/') for f in theirs[0])
    Engine = fc.fasta_engine()
    monkeypatch.setattr(reassign, '_device_split', _host_split)
    n_handles = len(fc.HostLinkPickle.opened)
    saved = patch.patch_reassign(R, rounds=True, engine=fc.HostReassign, pickle=True, pickle_engine=fc.HostLinkPickle.open, resident=True, fasta=True,
                                 fasta_engine=Engine)
    try:
        assert set(saved) == {'parse_link_dict', 'split_clm_file', 'run_reassignment', 'agglomerative_hierarchical_clustering', 'parse_pickle', 'parse_fasta'}
        ours = _run(R, argv, str(tmp_path / 'ours'), monkeypatch)
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)
    assert sorted(ours[0]) == sorted(theirs[0])
    for f in theirs[0]:
        assert ours[0][f] == theirs[0][f], f
    assert ours[1] == theirs[1]
    assert Engine.fetched == [] and len(Engine.opened) == 1 and Engine.count_calls == [300]
    assert [h.key_fetches for h in fc.HostLinkPickle.opened[n_handles:]] == [0]      # the keys never came to the host


def _host_split(clm_file, names, group_of_name, paths):
    """reassign._device_split through the contract of tests/clm_split_cases.py"""
    from tests import clm_split_cases as cs
    for p, data in zip(paths, cs.split_spec(open(clm_file, 'rb').read(), names, group_of_name, len(paths))):
        with open(p, 'wb') as f:
            f.write(data)
