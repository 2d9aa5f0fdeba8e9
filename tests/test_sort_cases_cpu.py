"""`haphic sort` on the CPU: the numpy engine of tests/sort_cases.py against tests/golden/sort.npz (which pins the per-row top-3 and the
scatter-add restatements to the reference's arrays), the mirrors of haphic_amd/sort.py with that engine against the reference's own fast_sort
(where the checkout exists), and the thread pool against the serial run."""
import os

import numpy as np
import pytest

from tests import sort_cases as sc

HAVE_REF = os.path.isfile(os.path.join(sc.REFERENCE_SCRIPTS, 'HapHiC_sort.py'))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason='needs the reference checkout (dev container only)')


@pytest.fixture(scope='module')
def fx():
    return sc.Fixture()


def test_fixture_covers_the_corpus(fx):
    assert fx.names == [c.name for c in sc.cases()]
    shapes = {n: int(fx.get(n, 'shape')) for n in fx.names}
    for name, shape in (('n2', 4), ('n3', 6), ('n4', 8), ('n32', 64), ('n33', 66), ('n128', 256), ('n129', 258), ('n130', 260)):
        assert shapes[name] == shape
    assert int(fx.get('seam_lds', 'new_shape', 0)) == sc.LDS_SHAPE and int(fx.get('seam_global', 'new_shape', 0)) == sc.LDS_SHAPE + 2
    flags = [int(fx.get('removal', 'removed', it)) for it in range(int(fx.get('removal', 'n_iter')))]
    assert flags[-3:] == [1, 1, 0] and fx.has('removal', 'map', len(flags) - 1)          # removed twice in a row, then an update
    assert int(fx.get('chain160', 'n_iter')) >= 5
    assert {str(fx.get(n, 'method')) for n in fx.names} == {'sum', 'multiplication', 'geometric_mean'}
    assert {float(fx.get(n, 'cutoff')) for n in fx.names} == {1.0, 1.5}
    assert 2.0 in fx.get('ties', 'conf_v', 0) and 1.0 in fx.get('ties', 'conf_v', 0)      # an unrivalled edge; tied maxima counted with multiplicity
    for name in ('n130', 'chain160', 'flank_geo'):                                      # the flank rule trims some ends, not all
        maps = [fx.get(name, 'map', it) for it in range(int(fx.get(name, 'n_iter'))) if fx.has(name, 'map', it)]
        assert any((m == -1).any() for m in maps) and all((m >= 0).any() for m in maps), name
    assert os.path.getsize(sc.GOLDEN) < 1 << 20


@pytest.mark.parametrize('case', [c.name for c in sc.cases()])
def test_numpy_engine_equals_the_reference(fx, case):
    eng, over = sc.play(sc.NumpyEngine, fx, case)
    if case == 'overflow':
        assert sum(over) > 0                             # the cells the reference's float32 running sum rounds are reported ...
    else:
        assert sum(over) == 0                            # ... and only there


def test_overflow_cells_differ_from_the_plain_rounding(fx):
    """the case is worth its name: at a reported cell float32(exact sum) is NOT what the reference holds"""
    differs = 0
    for it in range(int(fx.get('overflow', 'n_iter'))):
        if not fx.has('overflow', 'map', it):
            continue
        m = fx.get('overflow', 'map', it).astype(np.int64)
        ns = int(fx.get('overflow', 'new_shape', it))
        ei, ej, w = fx.get('overflow', 'edge_i', 0), fx.get('overflow', 'edge_j', 0), fx.get('overflow', 'edge_w', 0).astype(np.int64)
        i, j = m[ei], m[ej]
        ok = (i >= 0) & (j >= 0) & (i != j) & ((i ^ 1) != j)
        acc = np.zeros(ns * ns, np.int64)
        np.add.at(acc, np.maximum(i, j)[ok] * ns + np.minimum(i, j)[ok], w[ok])
        cells = fx.get('overflow', 'new_i', it).astype(np.int64) * ns + fx.get('overflow', 'new_j', it)
        differs += int((acc[cells].astype(np.float32) != fx.get('overflow', 'new_w', it)).sum())
    assert differs > 0


def test_engine_refuses_small_shapes_and_foreign_drops():
    with pytest.raises(RuntimeError):
        sc.NumpyEngine(2, [0], [1], [5])
    eng = sc.NumpyEngine(6, [0, 2], [3, 5], [5, 7])
    with pytest.raises(RuntimeError):
        eng.drop(0, 1)
    eng.drop(5, 4)
    assert eng.shape == 4


# ------------------------------------------------------------------ the mirrors against the reference's own fast_sort
@pytest.fixture(scope='module')
def modules():
    from haphic_amd import patch
    plain = sc.load_reference_sort(name='_haphic_sort_reference_plain')
    ours = sc.load_reference_sort(name='_haphic_sort_reference_patched')
    made = []

    def engine(shape, ei, ej, w):
        made.append(sc.NumpyEngine(shape, ei, ej, w))
        return made[-1]
    saved = patch.patch_sort(ours, engine=engine)
    return plain, ours, made, saved


@needs_ref
@pytest.mark.parametrize('case', sc.cases(), ids=lambda c: c.name)
def test_fast_sort_with_the_mirrors_equals_the_reference(modules, fx, case):
    plain, ours, made, _saved = modules
    del made[:]
    want = sc.run_fast_sort(plain, case)
    got = sc.run_fast_sort(ours, case)
    assert got[0] == want[0]
    assert got[1] == want[1] and want[1].decode().splitlines()[1] == str(fx.get(case.name, 'tour'))
    assert got[2] == want[2] and any('MAXS' in line for line in want[2])
    assert len(made) == 1                                # the device path took the group (no silent hand-over to the reference's functions)


@needs_ref
def test_uncovered_groups_go_to_the_reference_functions(modules):
    """weights that are not integers: decided once in round 1, the whole group runs the original functions and gives the reference's result"""
    plain, ours, made, _saved = modules
    case = sc.chain_case('floats', 12, 5)
    case = case._replace(links={k: v + 0.5 for k, v in case.links.items()})
    del made[:]
    assert sc.run_fast_sort(ours, case) == sc.run_fast_sort(plain, case)
    assert made == []


@needs_ref
def test_container_thaws_into_the_reference_dict(modules):
    from haphic_amd import sort
    plain, ours, made, _saved = modules
    case = [c for c in sc.cases() if c.name == 'n33'][0]
    seen = {}
    for S, key in ((plain, 'want'), (ours, 'got')):
        inner = S.update

        def update(*a, _inner=inner, _key=key, **k):
            res = _inner(*a, **k)
            seen.setdefault(_key, res[1])
            return res
        S.update = update
        try:
            sc.run_fast_sort(S, case)
        finally:
            S.update = inner
    got, want = seen['got'], seen['want']
    assert isinstance(got, sort.SubHT) and got.frozen and len(got) == len(want)
    items = list(got.items())                            # the first foreign access thaws it
    assert not got.frozen and items == list(want.items())
    assert all(type(v) is np.float32 and type(k[0]) is int and k[0] > k[1] for k, v in items)
    assert [k for k, _ in items] == sorted(k for k, _ in items)


@needs_ref
def test_thread_pool_gives_the_serial_tours(modules):
    """run()'s pool is the ThreadPool after patch_sort: two groups at once give what one after the other gives"""
    from multiprocessing.pool import ThreadPool
    plain, ours, _made, saved = modules
    assert ours.Pool is ThreadPool and saved['Pool'] is not ThreadPool
    two = [c for c in sc.cases() if c.name in ('n129', 'chain160')]
    serial = [sc.run_fast_sort(ours, c)[1] for c in two]
    pool = ours.Pool(2)
    results = [pool.apply_async(sc.run_fast_sort, args=(ours, c)) for c in two]
    pool.close()
    pool.join()
    assert [r.get()[1] for r in results] == serial == [sc.run_fast_sort(plain, c)[1] for c in two]
