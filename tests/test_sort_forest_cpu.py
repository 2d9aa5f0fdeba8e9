"""The forest block of `haphic sort`'s fast sorting without a GPU: the host engine of tests/sort_forest_cases.py against tests/golden/sort_forest.npz,
and — where the reference and networkx are at hand — the reference's fast_sort with patch_sort(S, forest=True) against the unpatched module."""
import os

import numpy as np
import pytest

from . import sort_cases as sc
from . import sort_forest_cases as fc

HAVE_REFERENCE = os.path.isfile(os.path.join(sc.REFERENCE_SCRIPTS, 'HapHiC_sort.py'))
needs_reference = pytest.mark.skipif(not HAVE_REFERENCE, reason='the reference scripts are not on this machine')
FORKED = ('fork0', 'fork1', 'fork2', 'fork3')


def test_fixture_conditions():
    """what the generator demanded of the fixture as a whole, read back from the file"""
    fx = fc.fixture()
    assert fx.names == fc.all_case_names()
    larger = not_paths = rounds = 0
    for case in fx.names:
        for it in fc.forest_rounds(fx, case):
            rounds += 1
            not_paths += int(fx.get(case, 'f_not_paths', it))
            if fx.has(case, 'f_paths', it):
                p, off = fx.get(case, 'f_paths', it), fx.get(case, 'f_path_off', it)
                larger += int((p[off[:-1]] > p[off[1:] - 1]).sum())
    assert rounds >= 90 and larger >= 20 and not_paths >= 3
    assert int(fx.get('path600', 'shape')) == 1200 and len(fx.get('path600', 'f_eu', 0)) == 1199


@pytest.mark.parametrize('case', fc.all_case_names())
def test_host_engine_equals_fixture(case):
    fx = fc.fixture()
    seen = []

    def on_forest(it, eng, maxs, got):
        fc.check_forest(fx, case, it, eng, maxs, got)
        seen.append(it)
    eng = fc.play_forest(fc.HostForestEngine, fx, case, on_forest)
    assert seen == fc.forest_rounds(fx, case) and seen
    assert eng.forest_stats()['confidence_copies'] == len(seen)            # check_forest's own fetches, nothing else


def test_host_engine_refuses_what_the_library_refuses():
    eng = fc.HostForestEngine(4, [3, 3], [1, 2], [10, 10])
    with pytest.raises(RuntimeError):
        eng.forest(1.0)
    with pytest.raises(RuntimeError):
        eng.fetch_confidence()
    eng.density([5e5] * 4, 'sum')
    eng.confidence_device([0, 1], [3, 2])
    with pytest.raises(RuntimeError):
        eng.forest(float('nan'))


# ------------------------------------------------------------------ the patched reference
class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


class _CountedTree:
    def __init__(self, module):
        self._module, self.calls = module, 0

    def __getattr__(self, name):
        return getattr(self._module, name)

    def maximum_spanning_tree(self, *a, **kw):
        self.calls += 1
        return self._module.maximum_spanning_tree(*a, **kw)


def _run(S, case):
    try:
        return sc.run_fast_sort(S, case)
    except AssertionError as e:
        return ('AssertionError', str(e))


_plain = {}


def _plain_result(case):
    """the unpatched module's answer, computed once per case"""
    if case.name not in _plain:
        _plain[case.name] = _run(sc.load_reference_sort(name='_haphic_sort_reference_forest_plain'), case)
    return _plain[case.name]


def _patched(engines, touch=None):
    """a private copy of the reference with networkx's two entries counted, then patched with the forest seams on the host engine"""
    from haphic_amd import patch
    S = sc.load_reference_sort(name='_haphic_sort_reference_forest_patched')
    tree, paths = _CountedTree(S.nxtree), _Counted(S.shortest_path)
    S.nxtree, S.shortest_path = tree, paths

    def make(shape, ei, ej, w):
        engines.append(fc.HostForestEngine(shape, ei, ej, w))
        return engines[-1]
    patch.patch_sort(S, engine=make, forest=True)
    if touch is not None:
        inner = S.filter_confidence_graph

        def filter_confidence_graph(confidence_graph, sub_HT_dict, cutoff):
            touch(confidence_graph)
            return inner(confidence_graph, sub_HT_dict, cutoff)
        S.filter_confidence_graph = filter_confidence_graph
    return S, tree, paths


@needs_reference
@pytest.mark.parametrize('case', fc.fast_sort_cases(), ids=lambda c: c.name)
def test_patched_fast_sort_equals_reference(case):
    pytest.importorskip('networkx')
    want = _plain_result(case)
    engines = []
    S, tree, paths = _patched(engines)
    got = _run(S, case)
    assert got == want
    assert (want[0] == 'AssertionError') == (case.name in FORKED)
    assert len(engines) == 1
    stats = engines[0].forest_stats()
    forests = stats['lds_forests'] + stats['hbm_forests']
    assert forests >= 1
    if case.name in FORKED:                                # the forked round went to the reference's block on the fetched array
        assert (tree.calls, stats['confidence_copies']) == (1, 1)
    else:
        assert (tree.calls, paths.calls, stats['confidence_copies']) == (0, 0, 0)


@needs_reference
@pytest.mark.parametrize('name', ['n33', 'removal', 'quant3', 'cycle4'])
def test_token_touched_by_foreign_code_thaws(name):
    pytest.importorskip('networkx')
    case = next(c for c in fc.fast_sort_cases() if c.name == name)
    engines, arrays = [], []
    S, tree, paths = _patched(engines, touch=lambda token: arrays.append(np.asarray(token)))
    assert _run(S, case) == _plain_result(case)
    assert all(a.dtype == np.float64 and a.ndim == 2 for a in arrays) and arrays
    stats = engines[0].forest_stats()
    assert stats['confidence_copies'] == len(arrays) == tree.calls and stats['lds_forests'] + stats['hbm_forests'] == 0
    assert paths.calls > 0


@needs_reference
def test_engine_without_forest_keeps_the_reference_block():
    pytest.importorskip('networkx')
    from haphic_amd import patch
    case = next(c for c in sc.cases() if c.name == 'n33')
    S = sc.load_reference_sort(name='_haphic_sort_reference_forest_patched')
    tree = _CountedTree(S.nxtree)
    S.nxtree = tree
    patch.patch_sort(S, engine=sc.NumpyEngine, forest=True)
    assert _run(S, case) == _plain_result(case) and tree.calls > 0


@needs_reference
def test_patch_sort_without_forest_leaves_the_globals():
    from haphic_amd import patch
    S = sc.load_reference_sort(name='_haphic_sort_reference_forest_patched')
    before = {name: getattr(S, name) for name in ('Graph', 'nxtree', 'shortest_path', 'connected_components')}
    saved = patch.patch_sort(S, engine=sc.NumpyEngine)
    assert all(getattr(S, name) is obj for name, obj in before.items()) and not set(saved) & set(before)
    patch.unpatch_reference(S, saved)
    saved = patch.patch_sort(S, engine=fc.HostForestEngine, forest=True)
    assert S.connected_components is before['connected_components']
    assert all(getattr(S, name) is not before[name] for name in ('Graph', 'nxtree', 'shortest_path'))
    assert set(patch.SORT_FOREST_SEAMS) <= set(saved)
    patch.unpatch_reference(S, saved)
    assert all(getattr(S, name) is obj for name, obj in before.items())


def test_forest_paths_mapping():
    """the stand-in for dict(shortest_path(tree))[source][target]: both directions, inner nodes, and dict() of it"""
    from haphic_amd import sort
    pos = {7: 0, 2: 1, 9: 2, 4: 3}
    paths = sort.ForestPaths([2, 4, 7, 9], pos)
    assert dict(paths)[7][4] == [7, 2, 9, 4] and dict(paths)[4][7] == [4, 9, 2, 7] and paths[2][9] == [2, 9] and paths[9][9] == [9]
    assert sorted(dict(paths)) == [2, 4, 7, 9] and len(paths) == 4


def test_wrapper_binds_the_forest_seams_unless_told_not_to(monkeypatch, tmp_path):
    """`python -m haphic_amd sort [--keep-reference-forest] ...`: the flag never reaches the reference's parser; without it the seams are bound after
    patch_sort, whose own arguments stay what they were"""
    import sys
    import types
    from haphic_amd import __main__ as cli
    from haphic_amd import _lib, patch, sort
    (tmp_path / 'HapHiC_cluster.py').write_text('')
    seen = {'forest': 0}
    fake = types.ModuleType('HapHiC_sort')
    fake.parse_arguments = lambda: seen.__setitem__('argv', list(sys.argv))
    fake.run = lambda args, log: None
    monkeypatch.setitem(sys.modules, 'HapHiC_sort', fake)
    monkeypatch.setattr(_lib, 'load', lambda: types.SimpleNamespace(hhx_set_device=lambda d: 0))
    monkeypatch.setattr(patch, 'patch_sort', lambda S, **kw: seen.__setitem__('kw', kw))
    monkeypatch.setattr(patch, 'patch_sort_heads', lambda S, engine=None: None)
    monkeypatch.setattr(patch, 'patch_sort_forest', lambda S: seen.__setitem__('forest', seen['forest'] + 1))
    monkeypatch.setattr(sys, 'argv', list(sys.argv))
    monkeypatch.setattr(sys, 'path', list(sys.path))
    monkeypatch.setattr(sort, 'DEVICE', None)
    rest = ['asm.fa', 'HT_links.pkl', 'split_clms', 'group1.txt']
    assert cli.main(['sort', '--reference', str(tmp_path), '--keep-reference-forest'] + rest) == 0
    assert seen['argv'] == ['haphic sort'] + rest and seen['forest'] == 0 and seen['kw'] == {'verdict': True}
    assert cli.main(['sort', '--reference', str(tmp_path)] + rest) == 0
    assert seen['argv'] == ['haphic sort'] + rest and seen['forest'] == 1
    assert '--keep-reference-forest' in cli.__doc__ and 'shape' in cli.__doc__
