"""`haphic sort`'s fast sorting on the device (hhx_sort_graph_*, haphic_amd/csrc/hhx_sort.hip) against tests/golden/sort.npz — the reference's own
arrays of every seam, case and round — bit for bit, chained: the edges one re-aggregation returns are what the next round's matrix is made of."""
import os
import subprocess
import sys

import numpy as np
import pytest

from haphic_amd import _lib
from tests import sort_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fx():
    return sc.Fixture()


@pytest.fixture(autouse=True)
def default_seam():
    yield
    _lib.tune('sort_lds_shape', None)


@pytest.mark.parametrize('case', [c.name for c in sc.cases()])
def test_device_equals_the_reference(fx, case):
    eng, over = sc.play(_lib.SortGraph, fx, case)
    host, host_over = sc.play(sc.NumpyEngine, fx, case)
    assert over == host_over and (sum(over) > 0) == (case == 'overflow')        # cells past 2^24: as many as numpy predicts, none elsewhere
    stats, want = eng.stats(), host.stats()
    assert (stats['lds_aggregations'], stats['global_aggregations']) == (want['lds_aggregations'], want['global_aggregations'])
    if case == 'seam_lds':                               # new shapes 192 and 2: both inside the LDS of a workgroup
        assert (stats['lds_aggregations'], stats['global_aggregations']) == (2, 0)
    if case == 'seam_global':                            # new shape 194: one step past the seam, global atomics; then 2
        assert (stats['lds_aggregations'], stats['global_aggregations']) == (1, 1)
    eng.close()


@pytest.mark.parametrize('case', ['n33', 'n129', 'chain160', 'overflow', 'removal'])
@pytest.mark.parametrize('seam', [0, 20])
def test_every_seam_setting_gives_the_same_bits(fx, case, seam):
    """"sort_lds_shape": the other re-aggregation path for the same cases (0: global atomics always; 20: the seam in the middle of the late rounds)"""
    _lib.tune('sort_lds_shape', seam)
    eng, _over = sc.play(_lib.SortGraph, fx, case)
    host, _over = sc.play(type('Seam', (sc.NumpyEngine,), {'lds_shape': seam}), fx, case)
    stats, want = eng.stats(), host.stats()
    assert (stats['lds_aggregations'], stats['global_aggregations']) == (want['lds_aggregations'], want['global_aggregations'])
    if seam == 0:
        assert stats['lds_aggregations'] == 0 and stats['global_aggregations'] > 0
    elif case == 'chain160':                             # new shapes 80, 46, 24 | 12, 6: both paths inside one group
        assert stats['lds_aggregations'] > 0 and stats['global_aggregations'] > 0
    eng.close()


def random_graph(seed, shape, n_edges, w_max):
    rng = np.random.default_rng(seed)
    cells = rng.permutation(shape * shape)
    cells = cells[cells // shape > cells % shape][:n_edges]
    assert cells.size == n_edges
    i, j = cells // shape, cells % shape
    swap = rng.integers(0, 2, n_edges).astype(bool)
    return np.where(swap, j, i), np.where(swap, i, j), rng.integers(1, w_max, n_edges)


@pytest.mark.parametrize('new_shape,w_max', [(2, 9), (190, 9), (192, 9), (194, 9), (64, 1 << 23)])
def test_reaggregation_paths_against_numpy(new_shape, w_max):
    """random maps (trimmed ends, several old ends per new end) on 400 old ends: the LDS path up to shape 192, global atomics past it and
    whenever the weights of the group sum to 2^32 or more (w_max 2^23 x 6000 edges), several workgroups in both"""
    ei, ej, w = random_graph(new_shape, 400, 6000, w_max)
    rng = np.random.default_rng(new_shape + 1)
    index_map = rng.integers(-1, new_shape, 400).astype(np.int32)
    dev, host = _lib.SortGraph(400, ei, ej, w), sc.NumpyEngine(400, ei, ej, w)
    got, want = dev.aggregate(new_shape, index_map), host.aggregate(new_shape, index_map)
    for g, h, what in zip(got, want, ('i', 'j', 'w', 'cells over')):
        assert np.array_equal(g, h), what
    sc.assert_same_bits(dev.matrix(), host.matrix(), 'matrix')
    assert dev.stats() == host.stats()
    assert (dev.stats()['lds_aggregations'] == 1) == (new_shape <= sc.LDS_SHAPE and int(w.sum()) < 1 << 32)
    if w_max > 1 << 20:
        assert got[3].size > 0
        ordinal = np.searchsorted(got[0].astype(np.int64) * new_shape + got[1], got[3])
        values = got[2][ordinal] + np.float32(2)
        dev.patch_cells(got[3], ordinal, values)
        host.patch_cells(got[3], ordinal, values)
        sc.assert_same_bits(dev.matrix(), host.matrix(), 'patched matrix')
    dev.close()


def test_geometric_mean_pairs_on_a_rounding_boundary_are_reported():
    """equal lengths whose root is an odd integer above 2^24 sit exactly on a float32 rounding boundary: the pair is reported, patched, and the
    density equals the numpy engine's; ordinary lengths report nothing"""
    ei, ej, w = random_graph(3, 8, 20, 1000)
    lengths = np.array([16777217.0, 16777217.0, 5e5, 7e5, 16777219.0, 16777219.0, 3e5, 16777217.0])
    dev, host = _lib.SortGraph(8, ei, ej, w), sc.NumpyEngine(8, ei, ej, w)
    got, want = dev.density(lengths, 'geometric_mean'), host.density(lengths, 'geometric_mean')
    assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())) and {(0, 1), (0, 7), (1, 7), (4, 5)} <= set(map(tuple, got.tolist()))
    L = [np.float32((lengths[a] * lengths[b]) ** 0.5) for a, b in got.tolist()]
    dev.patch_len(got, L)
    host.patch_len(got, L)
    sc.assert_same_bits(dev.density_graph(), host.density_graph(), 'density')
    assert len(dev.density(np.arange(1, 9) * 1e5 + 0.5, 'geometric_mean')) == 0
    dev.close()


def test_bad_arguments_are_error_codes():
    L = _lib.load()
    C = _lib.C
    n = C.c_int64(0)
    out = np.zeros(17, np.float64)
    assert L.hhx_sort_graph_density(None, _lib.ptr(out), 0, C.byref(n)) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_sort_graph_confidence(None, 0, None, None, _lib.ptr(out)) != 0
    assert L.hhx_sort_graph_aggregate(None, 2, None, C.byref(n), C.byref(n)) != 0
    assert L.hhx_sort_graph_drop(None, 1, 0) != 0 and L.hhx_sort_graph_stats(None, None) != 0 and L.hhx_sort_graph_destroy(None) == 0
    h = C.c_void_p()
    ei, ej, w = np.array([0], np.int32), np.array([1], np.int32), np.array([5], np.int64)
    assert L.hhx_sort_graph_create(2, 1, _lib.ptr(ei), _lib.ptr(ej), _lib.ptr(w), C.byref(h)) != 0 and not h.value and b'shape 2' in L.hhx_last_error()
    assert L.hhx_sort_graph_create(4, 0, None, None, None, C.byref(h)) != 0 and not h.value
    ej[0] = 4
    assert L.hhx_sort_graph_create(4, 1, _lib.ptr(ei), _lib.ptr(ej), _lib.ptr(w), C.byref(h)) != 0 and b'outside' in L.hhx_last_error()
    with pytest.raises(RuntimeError):
        _lib.SortGraph(2, [0], [1], [5])
    g = _lib.SortGraph(6, [0, 2], [3, 5], [5, 7])
    with pytest.raises(RuntimeError):
        g.drop(0, 1)                                     # not the last two indices
    with pytest.raises(RuntimeError):
        g.aggregate(4, np.array([0, 1, 2, 3, 4, -1]))    # a new index outside the new shape
    with pytest.raises(RuntimeError):
        g.aggregate(8, np.zeros(6, np.int32))            # a new shape above the old one
    with pytest.raises(RuntimeError):
        g.density(np.array([1.0, 2.0, 0.0, 1.0, 1.0, 1.0]), 'sum')
    g.drop(5, 4)
    assert g.shape == 4
    with pytest.raises(RuntimeError):
        g.drop(3, 2)                                     # two paths left: nothing to spare
    g.close()


def test_sort_is_a_command_now():
    """a child process with no reference path ends at the checkout check, not at the refusal of the command"""
    env = {k: v for k, v in os.environ.items() if k != 'HAPHIC_REFERENCE'}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    p = subprocess.run([sys.executable, '-m', 'haphic_amd', 'sort', 'asm.fa', 'HT_links.pkl', 'split_clms', 'group1.txt'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and 'HapHiC checkout not found' in p.stderr and 'steps only' not in p.stderr
    p = subprocess.run([sys.executable, '-m', 'haphic_amd', 'sort', '--gpus', '2'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert '--gpus is a flag of the "cluster" step only' in p.stderr
