"""The front of `haphic sort` on the CPU — HT_links.pkl behind the pickle proxy and get_sub_HT_dict per group (haphic_amd/sort.py bind_heads) — with the
host engine of tests/sort_heads_cases.py against tests/golden/sort_heads.npz (the reference's own items and HT_index_dict, order included), and,
where the checkout exists, against the reference's function and run() itself."""
import gc
import os
import pickle
from collections import defaultdict

import numpy as np
import pytest

from haphic_amd import containers, patch, sort
from tests import sort_cases as sc
from tests import sort_heads_cases as hc

HAVE_REF = os.path.isfile(os.path.join(sc.REFERENCE_SCRIPTS, 'HapHiC_sort.py'))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason='needs the reference checkout (dev container only)')
CASES = {c.name: c for c in hc.cases()}
SERVED = [c.name for c in hc.cases() if c.kind == 'int' and c.name != 'duplicate']


@pytest.fixture(scope='module')
def fx():
    return hc.Fixture()


def bound(S, tmp_path, case, engine=hc.HostPickle.open):
    """-> (table as run() :899-901 gets it through the proxy, the get_sub_HT_dict mirror, the proxy)"""
    proxy, mirror = sort.bind_heads(S, engine)
    path = str(tmp_path / (case.name + '.pkl'))
    hc.write_python(case, path)
    with open(path, 'rb') as f:
        table = proxy.load(f)
    return table, mirror, proxy


def test_fixture_covers_the_corpus(fx):
    assert fx.names == list(CASES)
    for name, case in CASES.items():
        names, ti, tj, tv = fx.table(name)
        i, j, v, want_names = hc.table_arrays(case.items)
        assert names == want_names and np.array_equal(ti, i) and np.array_equal(tj, j) and np.array_equal(tv, v) and tv.dtype == v.dtype, name
        assert fx.n_groups(name) == len(case.groups)
        for g, ctgs in enumerate(case.groups):
            got = fx.group(name, g)
            assert got[0] == list(ctgs)
            assert len(got[4]) == (2 * len(set(ctgs)) if len(ctgs) > 1 else 0), (name, g)        # every end has an index, linked or not
    for k in (0, 1, 63, 64, 65, 255, 256, 257):
        assert fx.group('keep%d' % k, 0)[1].size == k
    assert fx.group('all_keys', 0)[1].size == len(CASES['all_keys'].items) > 16 * hc.PASS_KEYS
    assert len(CASES['borders'].items) % 4 == 3 and fx.group('borders', 0)[1].size > 90
    assert fx.group('n1025', 0)[1].size == 20000 and int(fx.group('n1025', 0)[1].max()) >= 2 * 1024
    w = fx.group('values', 0)[3].tolist()
    assert 2 ** 53 in w and 2 ** 53 + 1 in w and min(w) < 0 and 0 not in w
    assert fx.group('strangers', 3)[1].size == 0 and len(fx.group('strangers', 3)[4]) == 4
    assert fx.group('n2_ab', 0)[3].max() < 5000                                                  # the reversed keys are never found
    assert os.path.getsize(hc.GOLDEN) < 1 << 20


@pytest.mark.parametrize('case', SERVED)
def test_mirror_with_the_host_engine_equals_the_fixture(fx, case, tmp_path):
    """no checkout needed: a call handed to the reference's function would raise"""
    table, mirror, proxy = bound(hc.fake_module(), tmp_path, CASES[case])
    assert isinstance(table, sort.HTTable) and table.frozen and len(table) == len(CASES[case].items)
    engine = table._session.engine
    calls = 0
    for g, ctgs in enumerate(CASES[case].groups):
        sub, index = mirror(list(ctgs), table)
        assert hc.result_pair(sub, index) == hc.expected_pair(fx, case, g), (case, g)
        assert type(index) is dict
        if len(ctgs) < 2:
            assert type(sub) is defaultdict and sub.default_factory is int and sub == {} and index == {}
        else:
            calls += 1
            assert isinstance(sub, sort.HeadsHT) and sub.frozen and sub.i.dtype == np.int32 and sub.j.dtype == np.int32 and sub.w.dtype == np.int64
        assert engine.calls == calls                                                       # fewer than two contigs: no call
    assert table.frozen and proxy.tables[0].thaws == 0


def test_container_thaws_into_the_dict_of_python_ints(fx, tmp_path):
    table, mirror, _proxy = bound(hc.fake_module(), tmp_path, CASES['values'])
    sub, _index = mirror(['s1', 's2', 's3'], table)
    assert sub.frozen and len(sub) == len(fx.group('values', 0)[1]) and bool(sub)
    before = len(containers.THAW_LOG)
    items = list(sub.items())                                                               # the first foreign access
    assert not sub.frozen and items == hc.expected_pair(fx, 'values', 0)[0] and containers.THAW_LOG[before][0] == 'sub_HT_heads'
    assert all(type(v) is int and type(k) is tuple and type(k[0]) is int for k, v in items)
    assert sub[(999, 998)] == 0 and pickle.loads(pickle.dumps(sub)) == dict(sub)


def test_round_one_takes_the_arrays_and_applies_the_refusals(tmp_path):
    """dict_to_matrix of round 1 on a frozen HeadsHT: the arrays go to the engine untouched; negative or over-2^53 values, an empty container and
    a shape below 4 take the reference's path, through a thaw"""
    made = []

    def engine(shape, ei, ej, w):
        made.append((shape, ei, ej, w))
        return sc.NumpyEngine(shape, ei, ej, w)
    S = hc.fake_module()
    handed = []
    S.dict_to_matrix = lambda d, shape, add_self_loops=False: handed.append(dict(d)) or 'reference'
    mirrors = sort.bind(S, engine)
    table, get_sub, _proxy = bound(S, tmp_path, CASES['n3'])
    sub, _index = get_sub(['q', 'p', 'r'], table)
    sort._tls.graph = None
    try:
        g = mirrors['dict_to_matrix'](sub, 6)
        assert isinstance(g, sort.Graph) and sub.frozen and made[0][1] is sub.i and made[0][3] is sub.w and g.source is sub
        assert g.ei is sub.i and g.ej is sub.j and g.alive.all()
        for case, ctgs, shape in (('values', ['s1', 's2', 's3'], 6), ('keep0', CASES['keep0'].groups[0], 48), ('n2_ab', ['a', 'b'], 2)):
            table, get_sub, _proxy = bound(S, tmp_path, CASES[case])
            sub, _index = get_sub(list(ctgs), table)
            sort._tls.graph = None
            want = dict(zip(zip(sub.i.tolist(), sub.j.tolist()), sub.w.tolist()))
            assert mirrors['dict_to_matrix'](sub, shape) == 'reference' and not sub.frozen and handed[-1] == want and sort._tls.graph is False
        assert len(made) == 1
    finally:
        sort._tls.graph = None


def test_removal_in_round_one_keeps_the_container_frozen(tmp_path):
    S = hc.fake_module()
    mirrors = sort.bind(S, sc.NumpyEngine)
    table, get_sub, _proxy = bound(S, tmp_path, CASES['n3'])
    sub, _index = get_sub(['q', 'p', 'r'], table)
    sort._tls.graph = None
    try:
        g = mirrors['dict_to_matrix'](sub, 6)
        pairs = [(0, 3), (1, 2), (4, 5)]
        assert mirrors['remove_shortest_path'](pairs, sub, g) is g and pairs == [(0, 3), (1, 2)]
        assert sub.frozen and len(sub) == int(g.alive.sum()) and not ((sub.i >= 4) | (sub.j >= 4)).any() and len(sub) > 0
    finally:
        sort._tls.graph = None


def test_patch_sort_without_heads_is_unchanged():
    S = hc.fake_module()
    originals = dict(vars(S))
    saved = patch.patch_sort(S, engine=sc.NumpyEngine)
    assert set(saved) == set(patch.SORT_SEAMS) | {'Pool'}
    assert S.pickle is pickle and S.get_sub_HT_dict is originals['get_sub_HT_dict']
    assert set(patch.SORT_HEADS_SEAMS) == {'pickle', 'get_sub_HT_dict'} and not set(patch.SORT_HEADS_SEAMS) & (set(patch.SORT_SEAMS) | set(patch.SORT_VERDICT_SEAMS))
    S = hc.fake_module()
    originals = dict(vars(S))
    saved = patch.patch_sort(S, engine=sc.NumpyEngine, heads=True, heads_engine=hc.HostPickle.open)
    assert set(saved) == set(patch.SORT_SEAMS) | set(patch.SORT_HEADS_SEAMS) | {'Pool'}
    assert saved['pickle'] is pickle and saved['get_sub_HT_dict'] is originals['get_sub_HT_dict']
    assert isinstance(S.pickle, sort.PickleProxy) and S.get_sub_HT_dict.__wrapped__ is originals['get_sub_HT_dict']


def test_proxy_forwards_everything_but_load(tmp_path):
    proxy, _mirror = sort.bind_heads(hc.fake_module(), hc.HostPickle.open)
    for name in ('dump', 'dumps', 'loads', 'Pickler', 'Unpickler', 'HIGHEST_PROTOCOL', 'PickleError', 'UnpicklingError'):
        assert getattr(proxy, name) is getattr(pickle, name)
    with pytest.raises(AttributeError):
        proxy.no_such_thing
    assert proxy.loads(proxy.dumps({1: 2})) == {1: 2}
    # what is no real file at its start is pickle's own: a bytes stream, a file that has been read from, extra arguments
    import io
    data = pickle.dumps(hc.table_of(CASES['n3']), protocol=4)
    got = proxy.load(io.BytesIO(data))
    assert type(got) is defaultdict and got == hc.table_of(CASES['n3'])
    path = str(tmp_path / 'two.pkl')
    with open(path, 'wb') as f:
        f.write(pickle.dumps('first') + data)
    with open(path, 'rb') as f:
        assert proxy.load(f) == 'first' and type(proxy.load(f)) is defaultdict
    with open(path, 'rb') as f:
        assert proxy.load(f, encoding='latin1') == 'first'
    assert proxy.tables == []
    # a file the reader refuses: pickle.load's result
    path = str(tmp_path / 'plain.pkl')
    hc.write_python(CASES['plain_dict'], path)
    with open(path, 'rb') as f:
        got = proxy.load(f)
    assert type(got) is dict and got == dict(CASES['plain_dict'].items) and proxy.tables == []
    with open(str(tmp_path / 'empty.pkl'), 'wb'):
        pass
    with open(str(tmp_path / 'empty.pkl'), 'rb') as f, pytest.raises(EOFError):
        proxy.load(f)


def test_finalizer_closes_the_handle(tmp_path):
    table, mirror, proxy = bound(hc.fake_module(), tmp_path, CASES['n3'])
    engine = table._session.engine
    sub, _index = mirror(['q', 'p', 'r'], table)
    assert not engine.closed
    del table                                                                               # run() :922-923
    gc.collect()
    assert engine.closed and sub.frozen and len(sub) == 12                                  # the groups' containers hold arrays, not the table
    # a thaw closes it too: the dict holds every key then
    table, mirror, proxy = bound(hc.fake_module(), tmp_path, CASES['n3'])
    engine = table._session.engine
    assert ('q_H', 'r_T') in table and not table.frozen and engine.closed and proxy.tables[0].thaws == 1 and proxy.tables[0].engine is None
    assert type(table) is containers.Thawed and list(table.items()) == CASES['n3'].items


# ------------------------------------------------------------------ against the reference's own code
@pytest.fixture(scope='module')
def reference():
    return sc.load_reference_sort(name='_haphic_sort_reference_heads_plain')


@needs_ref
@pytest.mark.parametrize('case', list(CASES))
def test_mirror_equals_the_reference_function(reference, fx, case, tmp_path):
    """every case, the hand-backs included: items, both insertion orders, and the table a hand-back thaws into"""
    S = sc.load_reference_sort(name='_haphic_sort_reference_heads_' + case)
    table, mirror, proxy = bound(S, tmp_path, CASES[case])
    with open(str(tmp_path / (case + '.pkl')), 'rb') as f:
        plain = pickle.load(f)
    handed_back = CASES[case].kind != 'int' or case == 'duplicate'
    assert (type(table) is type(plain)) == (CASES[case].kind == 'plain_dict')
    for g, ctgs in enumerate(CASES[case].groups):
        sub, index = mirror(list(ctgs), table)
        want_sub, want_index = reference.get_sub_HT_dict(list(ctgs), plain)
        assert hc.result_pair(sub, index) == (list(want_sub.items()), list(want_index.items())), (case, g)
        if CASES[case].kind != 'float':
            assert hc.result_pair(sub, index) == hc.expected_pair(fx, case, g)
        assert type(sub) is type(want_sub) or sub.frozen
        assert [type(v) for v in dict(sub).values()] == [type(v) for v in want_sub.values()]
    if handed_back and CASES[case].kind != 'plain_dict':
        assert not table.frozen and proxy.tables[0].thaws == 1
    if CASES[case].kind != 'plain_dict':
        assert list(table.items()) == list(plain.items()) and table.default_factory is int and isinstance(table, defaultdict)
        assert [type(v) for v in table.values()] == [type(v) for v in plain.values()]


@needs_ref
def test_front_of_run_on_a_toy_job_equals_the_reference(tmp_path, monkeypatch):
    """run() :847-959 whole, in quick view, with and without the heads seams (host engines): the same tour files and links; no thaw on the way"""
    made, tables = [], []
    outs = []
    for k, heads in enumerate((False, True)):
        S = sc.load_reference_sort(name='_haphic_sort_reference_heads_job%d' % k)
        tmp = tmp_path / ('job%d' % k)
        tmp.mkdir()
        argv = hc.toy_job(str(tmp))
        if heads:
            def engine(shape, ei, ej, w):
                made.append(sc.NumpyEngine(shape, ei, ej, w))
                return made[-1]
            patch.patch_sort(S, engine=engine, heads=True, heads_engine=hc.HostPickle.open)
            tables = S.pickle.tables
            front = []
            inner = S.get_sub_HT_dict
            S.get_sub_HT_dict = lambda ctgs, t, _inner=inner: front.append(_inner(ctgs, t)) or front[-1]
        before = len(containers.THAW_LOG)
        outs.append(hc.run_job(S, str(tmp), argv, monkeypatch))
    assert outs[0] == outs[1] and set(outs[0]) == {'group1.tour', 'group2.tour', 'final_tours'}
    assert len(made) == 2 and len(tables) == 1 and tables[0].thaws == 0 and len(containers.THAW_LOG) == before
    gc.collect()
    assert tables[0].engine.closed                                                          # del HT_link_dict; gc.collect() :922-923
    assert [len(sub) for sub, _ in front] == [len(m.ea) for m in made] and all(sub.frozen for sub, _ in front)


def test_wrapper_binds_the_heads_seams_unless_told_not_to(monkeypatch, tmp_path):
    """`python -m haphic_amd sort [--keep-reference-heads] ...`: the flag never reaches the reference's parser, and without it the two seams are bound
    after patch_sort"""
    import sys
    import types
    from haphic_amd import __main__ as cli
    from haphic_amd import _lib
    (tmp_path / 'HapHiC_cluster.py').write_text('')
    seen = {'heads': 0}
    fake = types.ModuleType('HapHiC_sort')
    fake.parse_arguments = lambda: seen.__setitem__('argv', list(sys.argv))
    fake.run = lambda args, log: None
    monkeypatch.setitem(sys.modules, 'HapHiC_sort', fake)
    monkeypatch.setattr(_lib, 'load', lambda: types.SimpleNamespace(hhx_set_device=lambda d: 0))
    monkeypatch.setattr(patch, 'patch_sort', lambda S, **kw: seen.__setitem__('kw', kw))
    monkeypatch.setattr(patch, 'patch_sort_heads', lambda S, engine=None: seen.__setitem__('heads', seen['heads'] + 1))
    monkeypatch.setattr(sys, 'argv', list(sys.argv))
    monkeypatch.setattr(sys, 'path', list(sys.path))
    monkeypatch.setattr(sort, 'DEVICE', None)
    rest = ['asm.fa', 'HT_links.pkl', 'split_clms', 'group1.txt']
    assert cli.main(['sort', '--reference', str(tmp_path), '--keep-reference-heads'] + rest) == 0
    assert seen['argv'] == ['haphic sort'] + rest and seen['heads'] == 0 and seen['kw'] == {'verdict': True}
    assert cli.main(['sort', '--reference', str(tmp_path)] + rest) == 0
    assert seen['argv'] == ['haphic sort'] + rest and seen['heads'] == 1
    assert '--keep-reference-heads' in cli.__doc__
