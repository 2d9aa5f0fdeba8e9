"""Each group's H/T links from HT_links.pkl on the device (hhx_pickle_group_heads, haphic_amd/csrc/hhx_pickleread.hip) against
tests/golden/sort_heads.npz — the reference's own get_sub_HT_dict: items and HT_index_dict, insertion order included — through the seams of
haphic_amd/sort.py bind_heads, in both pickle dialects and under both settings of the LDS-bitmap knob."""
import gc
import os

import numpy as np
import pytest

from haphic_amd import _lib, containers, sort
from tests import sort_cases as sc
from tests import sort_heads_cases as hc

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in hc.cases()}
SERVED = [c.name for c in hc.cases() if c.kind == 'int' and c.name != 'duplicate']
WRITERS = {'python': hc.write_python, 'library': hc.write_library}


@pytest.fixture(scope='module')
def fx():
    return hc.Fixture()


@pytest.fixture(autouse=True)
def default_knob():
    yield
    _lib.tune('heads_bitmap', None)
    _lib.tune('heads_grid', None)


def load(S, path):
    proxy, mirror = sort.bind_heads(S)
    with open(path, 'rb') as f:
        return proxy.load(f), mirror, proxy


@pytest.mark.parametrize('dialect', sorted(WRITERS))
@pytest.mark.parametrize('case', SERVED)
def test_device_equals_the_reference(fx, case, dialect, tmp_path):
    path = str(tmp_path / 'HT_links.pkl')
    WRITERS[dialect](CASES[case], path)
    table, mirror, proxy = load(hc.fake_module(), path)                  # a call handed to the reference's function would raise
    assert isinstance(table, sort.HTTable) and table.frozen and len(table) == len(CASES[case].items)
    # "heads_grid" 1: four wavefronts in all, so a wavefront walks its range in several steps wherever the table has more than 1024 keys (22 at
    # n1025: the next step's ids loaded ahead, the running offset carried from step to step in both passes); 2: the same with two workgroups
    for bitmap, grid in ((1, None), (0, None), (None, 1), (0, 1), (1, 2)):
        _lib.tune('heads_bitmap', bitmap)
        _lib.tune('heads_grid', grid)
        for g, ctgs in enumerate(CASES[case].groups):                    # one after the other from one handle
            sub, index = mirror(list(ctgs), table)
            assert hc.result_pair(sub, index) == hc.expected_pair(fx, case, g), (case, g, bitmap, grid)
            if len(ctgs) > 1:
                assert sub.frozen and sub.i.dtype == np.int32 and sub.j.dtype == np.int32 and sub.w.dtype == np.int64
    assert table.frozen and proxy.tables[0].thaws == 0
    engine = proxy.tables[0].engine
    del table
    gc.collect()
    assert engine.h is None                                              # the finalizer freed the table on the device


def test_several_steps_per_wavefront_at_the_default_grid(tmp_path):
    """the shape every job has: more keys than one step of the whole grid takes (1536 workgroups x 4 wavefronts x 64 lanes x 4 keys = 1.57 M), so
    every wavefront walks several steps.  3.5 M keys in the library dialect, two groups of 1000 contigs, survivors in every step of the ranges;
    arrays and order against the numpy engine on the same arrays, under both settings of the bitmap knob"""
    n_keys = 3_500_000
    i, j, value, names, groups, member = hc.big_table(n_keys, 17)
    per_wave = -(-(-(-(n_keys // 4) // hc.GRID_WAVES)) // 64) * 64                     # quads of a wavefront's range: whole steps
    n_steps = per_wave // 64
    assert n_steps >= 3 and n_keys > hc.GRID_WAVES * hc.PASS_KEYS
    path = str(tmp_path / 'HT_links.pkl')
    _lib.write_link_pickle(path, i, j, value, names)
    table, mirror, proxy = load(hc.fake_module(), path)
    assert table.frozen and len(table) == n_keys
    _proxy, host_mirror = sort.bind_heads(hc.fake_module(), hc.HostPickle.open)
    host = sort.HTTable(hc.HostPickle.from_arrays(i, j, value, names))
    for g, ctgs in enumerate(groups):
        keep = member[g][i >> 1] & member[g][j >> 1] & (value != 0)
        steps = np.unique(((np.flatnonzero(keep) // 4) % per_wave) // 64)
        assert steps.tolist() == list(range(n_steps))                                  # survivors in the first, the middle and the last steps
        want, want_index = host_mirror(ctgs, host)
        assert len(want) == int(keep.sum()) > 100_000
        for bitmap in (1, 0):
            _lib.tune('heads_bitmap', bitmap)
            sub, index = mirror(ctgs, table)
            assert np.array_equal(sub.i, want.i) and np.array_equal(sub.j, want.j) and np.array_equal(sub.w, want.w), (g, bitmap)
            assert list(index.items()) == list(want_index.items())
    assert table.frozen and proxy.tables[0].thaws == 0


def test_hand_backs_reach_the_reference_function_with_the_thawed_table(tmp_path):
    """a duplicated contig, a table of floats: the original function is called on exactly the dict pickle.load gives; a file the reader refuses
    is pickle.load's from the start"""
    import pickle
    for case, ctgs in (('duplicate', ['d1', 'd2', 'd1']), ('floats', ['d1', 'd2', 'd3'])):
        S = hc.fake_module()
        seen = []
        S.get_sub_HT_dict = lambda c, t: seen.append((c, list(t.items()), type(t), t.default_factory)) or 'reference'     # the look at the items thaws
        path = str(tmp_path / (case + '.pkl'))
        hc.write_python(CASES[case], path)
        table, mirror, proxy = load(S, path)
        assert table.frozen
        with open(path, 'rb') as f:
            plain = pickle.load(f)
        assert mirror(ctgs, table) == 'reference' and not table.frozen and proxy.tables[0].thaws == 1
        assert seen == [(ctgs, list(plain.items()), containers.Thawed, int)]
        assert [type(v) for _k, v in seen[0][1]] == [type(v) for v in plain.values()] and isinstance(table, type(plain))
    refused = len(_lib.PICKLE_REFUSALS)
    path = str(tmp_path / 'plain.pkl')
    hc.write_python(CASES['plain_dict'], path)
    table, mirror, proxy = load(hc.fake_module(), path)
    assert type(table) is dict and table == dict(CASES['plain_dict'].items) and len(_lib.PICKLE_REFUSALS) == refused + 1 and proxy.tables == []


def test_bad_arguments_are_error_codes(tmp_path):
    L, C = _lib.load(), _lib.C
    n = C.c_int64(0)
    slot, rank = np.zeros(4, np.int32), np.zeros(2, np.int32)
    assert L.hhx_pickle_group_heads(None, 2, _lib.ptr(slot), _lib.ptr(rank), C.byref(n)) != 0 and b'null handle' in L.hhx_last_error()
    assert L.hhx_pickle_group_heads_fetch(None, None, None, None) != 0 and b'null handle' in L.hhx_last_error()
    path = str(tmp_path / 'n3.pkl')
    hc.write_python(CASES['n3'], path)
    h = _lib.LinkPickle.open(path)
    assert h.n_names == 6 and h.names() == hc.table_arrays(CASES['n3'].items)[3] and h.n_keys == 12 and not h.any_float
    good_slot, good_rank = np.full(6, -1, np.int32), np.array([0, 1], np.int32)
    for n_ctg, s, r in ((1, good_slot, good_rank[:1]), (2, np.full(6, 4, np.int32), good_rank), (2, np.full(6, -2, np.int32), good_rank),
                        (2, good_slot, np.array([0, 0], np.int32)), (2, good_slot, np.array([0, 2], np.int32))):
        with pytest.raises(RuntimeError):
            h.group_heads(n_ctg, s, r)
    with pytest.raises(ValueError):
        h.group_heads(2, good_slot[:5], good_rank)
    ei, ej, w = h.group_heads(2, good_slot, good_rank)                   # no name of the group in the file
    assert ei.size == ej.size == w.size == 0
    h.close()
    h.close()
    hc.write_python(CASES['floats'], path)
    h = _lib.LinkPickle.open(path)
    assert h.any_float
    with pytest.raises(RuntimeError, match='float'):
        h.group_heads(2, np.full(h.n_names, -1, np.int32), good_rank)
    h.close()


def test_front_of_a_toy_job_through_round_one(tmp_path):
    """what run() :898-923 and round 1 of fast_sort do with the seams bound, on the device: no thaw anywhere, the round-1 link matrix equals the
    one the host engines build from the same files, and deleting the table frees it.  NOT tour parity on the device: fast_sort and the tour writer
    are the reference's code, which is not where the GPU is; the tours of run() with and without the seams are compared with host engines in
    tests/test_sort_heads_cpu.py, and from an equal round-1 matrix on the rounds are those of tests/test_gpu_sort.py"""
    hc.toy_job(str(tmp_path))
    matrices = {}
    for engines in ('host', 'device'):
        S = hc.fake_module()
        mirrors = sort.bind(S, sc.NumpyEngine if engines == 'host' else None)
        proxy, get_sub = sort.bind_heads(S, hc.HostPickle.open if engines == 'host' else None)
        before = len(containers.THAW_LOG)
        with open(str(tmp_path / 'HT_links.pkl'), 'rb') as f:
            table = proxy.load(f)
        for group in ('group1.txt', 'group2.txt'):
            with open(str(tmp_path / group)) as f:
                info = [(line.split()[0], int(line.split()[2])) for line in f if not line.startswith('#')]
            info.sort(key=lambda x: x[1], reverse=True)
            sub, index = get_sub([c for c, _ in info], table)
            assert sorted(index.values()) == list(range(2 * len(info))) and len(sub) > len(info)
            sort._tls.graph = None
            try:
                g = mirrors['dict_to_matrix'](sub, 2 * len(info))
                assert isinstance(g, sort.Graph) and sub.frozen and g.thaws == 0
                matrices[engines, group] = g.engine.matrix()
                g.close()
            finally:
                sort._tls.graph = None
        assert table.frozen and proxy.tables[0].thaws == 0 and len(containers.THAW_LOG) == before
        engine = proxy.tables[0].engine
        del table
        gc.collect()
        assert engine.closed if engines == 'host' else engine.h is None
    for group in ('group1.txt', 'group2.txt'):
        sc.assert_same_bits(matrices['device', group], matrices['host', group], group)
        assert np.count_nonzero(matrices['host', group]) > 0
