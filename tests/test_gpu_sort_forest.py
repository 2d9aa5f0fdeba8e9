"""The forest block of `haphic sort`'s fast sorting on the device (hhx_sort_graph_confidence_device / _forest / _fetch_forest / _fetch_confidence,
haphic_amd/csrc/hhx_sort.hip) against tests/golden/sort_forest.npz: every recorded round of every group, replayed as tests/sort_cases.py play()
replays the dense seams, gives the fixture's chosen edges in Kruskal's order, labels, positions and not_paths, in both forms of the call."""
import ctypes as C

import numpy as np
import pytest

from haphic_amd import _lib
from tests import sort_forest_cases as fc

pytestmark = pytest.mark.gpu
SEAMS = {'lds': None, 'hbm': 0, 'seam100': 100}          # hhx_tune "sort_forest_lds": the default (2048), always HBM, the seam inside the corpus


@pytest.fixture(autouse=True)
def default_seam():
    yield
    _lib.tune('sort_forest_lds', None)


def _host(seam):
    return type('Seam', (fc.HostForestEngine,), {'forest_lds': fc.FOREST_LDS_SHAPE if seam is None else seam})


@pytest.mark.parametrize('seam', list(SEAMS))
@pytest.mark.parametrize('case', fc.all_case_names())
def test_device_forest_equals_the_fixture(case, seam):
    fx = fc.fixture()
    _lib.tune('sort_forest_lds', SEAMS[seam])
    seen = []

    def on_forest(it, eng, maxs, got):
        assert eng.forest_stats()['confidence_copies'] == len(seen)        # confidence_device and forest copy no array; check_forest fetches one
        fc.check_forest(fx, case, it, eng, maxs, got)
        seen.append(it)
    eng = fc.play_forest(_lib.SortGraph, fx, case, on_forest)
    host = fc.play_forest(_host(SEAMS[seam]), fx, case, lambda *a: None)
    assert seen == fc.forest_rounds(fx, case) and seen
    stats, want = eng.forest_stats(), host.forest_stats()
    assert (stats['lds_forests'], stats['hbm_forests']) == (want['lds_forests'], want['hbm_forests'])
    assert stats['lds_forests'] + stats['hbm_forests'] == len(seen) and stats['jump_rounds'] == want['jump_rounds']
    if seam == 'hbm':
        assert stats['lds_forests'] == 0
    if seam == 'lds':
        assert stats['hbm_forests'] == 0
    if seam == 'seam100' and case == 'quant2':           # shapes 148 | 24, 14, 10, 6, 2: both forms inside one group
        assert stats['lds_forests'] > 0 and stats['hbm_forests'] > 0
    if case == 'path600' and seam != 'seam100':
        assert stats['jump_rounds'] == 11                # 1200 nodes on one path
    eng.close()


def test_more_edges_than_the_lds_form_holds_take_the_other_form():
    """The seam in edges: at shape 2048 the one-workgroup form holds 4096 edges beside its node arrays.  Random graphs on 1024 contigs, cutoff 0 so
    that every edge stays: 3 * 1024 edges and the 1024 sister pairs fill it exactly and stay in LDS; 5 * 1024 do not fit, the kernel says so and
    the call is redone in HBM.  Dense random graphs also give Boruvka long hook chains.  Both against the restatement."""
    rng = np.random.default_rng(5)
    n = 1024
    for per_end, form in ((3, 'lds_forests'), (5, 'hbm_forests')):
        cells = set()
        while len(cells) < per_end * n:
            a, b = (int(x) for x in rng.integers(0, 2 * n, 2))
            if a != b and (a ^ 1) != b:
                cells.add((max(a, b), min(a, b)))
        e = np.array(sorted(cells), np.int64)
        w = rng.integers(1, 1000, len(e))
        pairs = np.arange(2 * n, dtype=np.int32).reshape(-1, 2)
        got, want = [], []
        for make, out in ((_lib.SortGraph, got), (fc.HostForestEngine, want)):
            eng = make(2 * n, e[:, 0], e[:, 1], w)
            eng.density(np.full(2 * n, 1e6), 'sum')
            eng.confidence_device(pairs[:, 0], pairs[:, 1])
            out.extend(eng.forest(0.0))                  # every edge with a density stays: far more than 1.5 * shape
            out.append(eng.forest_stats()[form])
            eng.close()
        assert got[4] == want[4] is True and got[5] == want[5] == 1
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4]))


def test_bad_arguments_are_refused():
    L = _lib.load()
    n, bad = C.c_int64(0), C.c_int32(0)
    out = np.zeros(64, np.float64)
    idx = np.zeros(8, np.int32)
    assert L.hhx_sort_graph_forest(None, 1.0, C.byref(n), C.byref(bad)) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_sort_graph_confidence_device(None, 0, None, None, _lib.ptr(out)) != 0
    assert L.hhx_sort_graph_fetch_confidence(None, _lib.ptr(out)) != 0
    assert L.hhx_sort_graph_fetch_forest(None, _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx)) != 0
    assert L.hhx_sort_graph_forest_stats(None, None) != 0
    eng = _lib.SortGraph(6, [5, 3, 4], [1, 0, 2], [10, 20, 30])
    assert L.hhx_sort_graph_forest(eng.h, 1.0, C.byref(n), C.byref(bad)) != 0 and b'no confidence' in L.hhx_last_error()      # before any confidence
    assert L.hhx_sort_graph_fetch_confidence(eng.h, _lib.ptr(out)) != 0 and b'no confidence' in L.hhx_last_error()
    assert L.hhx_sort_graph_fetch_forest(eng.h, _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx)) != 0 and b'no forest' in L.hhx_last_error()
    eng.density([1e6] * 6, 'sum')
    assert L.hhx_sort_graph_confidence_device(eng.h, 3, None, None, _lib.ptr(out)) != 0
    assert L.hhx_sort_graph_confidence_device(eng.h, 3, _lib.ptr(idx), _lib.ptr(idx), None) != 0
    maxs = eng.confidence_device([0, 2, 4], [1, 3, 5])
    assert type(maxs) is np.float64 and maxs == 2.0
    assert L.hhx_sort_graph_forest(eng.h, float('nan'), C.byref(n), C.byref(bad)) != 0 and b'not a number' in L.hhx_last_error()
    assert L.hhx_sort_graph_fetch_forest(eng.h, _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx), _lib.ptr(idx)) != 0           # nothing computed yet
    assert L.hhx_sort_graph_forest(eng.h, 1.0, None, None) == 0
    assert L.hhx_sort_graph_fetch_forest(eng.h, _lib.ptr(idx), _lib.ptr(idx), None, _lib.ptr(idx)) != 0
    host = fc.HostForestEngine(6, [5, 3, 4], [1, 0, 2], [10, 20, 30])
    host.density([1e6] * 6, 'sum')
    host.confidence_device([0, 2, 4], [1, 3, 5])
    got, want = eng.forest(1.0), host.forest(1.0)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and len(got[0]) == 5 and not got[4]
    eng.drop(5, 4)                                       # the array on the device was laid out for shape 6
    assert L.hhx_sort_graph_forest(eng.h, 1.0, C.byref(n), C.byref(bad)) != 0 and L.hhx_sort_graph_fetch_confidence(eng.h, _lib.ptr(out)) != 0
    with pytest.raises(RuntimeError):
        _lib.tune('sort_forest', 1)
    eng.close()
