"""--dense_matrix Markov clustering without a GPU: the numpy host model of tests/dense_mcl_cases.py (what the GPU tests compare the device
against) reproduces what the REFERENCE's dense mode did on every case (tests/golden/dense_mcl.npz, tests/golden/make_golden_dense.py), and the
binding: patch_reference(H) leaves a dense call with the original function, patch_reference(H, dense=True) routes it to the mirror, the
wrapper command removes --keep-reference-dense."""
import sys
import types

import numpy as np
import pytest

from tests import dense_mcl_cases as dc
from tests.conftest import load_golden


@pytest.fixture(scope='module')
def golden():
    return load_golden('dense_mcl.npz')


def source_of(golden, case):
    if case.public:
        return golden[case.source + '_matrix']
    s = case.source
    return int(golden[s + '_n']), golden[s + '_i'].astype(np.int64), golden[s + '_j'].astype(np.int64), golden[s + '_cnt'].astype(np.float32)


def final_of(golden, case, n):
    m = np.zeros((n, n), np.float32)
    m[golden[case.name + '_final_i'].astype(np.int64), golden[case.name + '_final_j'].astype(np.int64)] = golden[case.name + '_final_x']
    return m


def clusters_of(golden, case):
    if not bool(golden[case.name + '_valid']):
        return None
    ptr, mem = golden[case.name + '_cluster_ptr'].tolist(), golden[case.name + '_cluster_members'].tolist()
    return [tuple(mem[a:b]) for a, b in zip(ptr[:-1], ptr[1:])]


def test_golden_holds_every_case(golden):
    assert sorted(golden['cases'].tolist()) == sorted(c.name for c in dc.cases())
    fresh = dc.sources()
    for name, (n, i, j, cnt) in fresh.items():                     # the frozen inputs are the ones the case file describes
        assert int(golden[name + '_n']) == n and np.array_equal(golden[name + '_i'], i) and np.array_equal(golden[name + '_j'], j)
        assert np.array_equal(golden[name + '_cnt'], cnt)
    for name, a in dc.crafted().items():
        assert np.array_equal(golden[name + '_matrix'], a)
    errs = [float(golden[c.name + '_ref_step_err']) for c in dc.cases()]
    assert max(errs) < 5e-7                                        # float32 round-off of column-stochastic operands, nothing else


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', dc.cases(), ids=repr)
def test_host_model_reproduces_the_reference(golden, case, dtype):
    """round count, converged flag, log line and clusters exactly; the final matrix within the step yardstick"""
    src = source_of(golden, case)
    if case.public:
        pre = src.astype(dtype)
    else:
        pre = dc.pre_expand(dc.matrix_from_edges(*src).astype(dtype), case.expansion)
    m, rounds, converged, _ = dc.mcl(pre, case.expansion, case.inflation, case.max_iter, case.pruning)
    assert m.dtype == dtype
    assert (rounds, converged) == (int(golden[case.name + '_rounds']), bool(golden[case.name + '_converged']))
    assert dc.clusters(m) == clusters_of(golden, case)
    want = final_of(golden, case, m.shape[0])
    err = float(golden[case.name + '_ref_step_err'])
    assert np.array_equal(m != 0, want != 0)
    # a converged trajectory is contracting: what is left of the round-off of the rounds before is of the size of one step's
    assert np.abs(m.astype(np.float64) - want).max() <= 4 * err


def test_crafted_cases_are_what_they_claim(golden):
    a = dc.crafted()['tie8']
    p = dc.prune(a, 0.3)
    # column 0: the maximum 0.25 (rows 1 and 5) is below the threshold, everything is pruned and the FIRST maximum comes back alone
    assert np.array_equal(np.flatnonzero(p[:, 0]), [1]) and p[1, 0] == 1.0
    # column 3: the tie 0.5 / 0.5 survives the threshold as it is
    assert p[2, 3] == 0.5 and p[3, 3] == 0.5
    # round 0 of mcl(): column 4 is a four-fold tie at 0.25 after inflate + normalise, below 0.3: row 4 wins
    first = dc.step(a, 0, 2, 2.0, 0.3)
    assert np.array_equal(np.flatnonzero(first[:, 4]), [4]) and first[4, 4] == 1.0
    z = dc.crafted()['zerocol12']
    assert not z[:, 5].any() and np.allclose(np.delete(z.sum(axis=0), 5), 1.0)
    for name, rounds, conv in (('planted33_e2_i2.0_iter1', 1, False), ('planted33_e2_i2.0_iter2', 2, False), ('planted33_e2_i2.0_iter3', 3, False),
                               ('planted97_e2_i1.2_iter6', 6, False)):
        assert (int(golden[name + '_rounds']), bool(golden[name + '_converged'])) == (rounds, conv)


# ------------------------------------------------------------------ binding
SEAM_ARGS = {'mcl': (None, 2, 2.0, 10, 1e-4), 'prune': (None, 1e-4), 'interpret_result': (None,),
             'run_mcl_clustering': (None, set(), {}, {}, 2, 1.1, 1.2, 0.1, 10, 1e-4, {}, 2)}


@pytest.fixture
def stub_lib(monkeypatch):
    from haphic_amd import patch
    import haphic_amd._lib as real                      # patch_reference only asks it to load: no library needed for the routing
    monkeypatch.setattr(real, 'load', lambda: None)
    return patch


def test_patch_reference_routes_dense_calls_only_on_request(stub_lib, monkeypatch):
    patch = stub_lib
    from haphic_amd import cluster
    calls = []
    for name in patch.DENSE_ARG:
        monkeypatch.setattr(cluster, name, (lambda nm: lambda *a, **k: calls.append(nm) or 'mirror')(name))
        monkeypatch.setitem(patch.SEAMS, name, (patch.SEAMS[name][0], getattr(cluster, name)))
    for kwargs, routed in (({}, False), ({'dense': False}, False), ({'dense': True}, True)):
        H = types.ModuleType('H')
        for name in patch.DENSE_ARG:
            setattr(H, name, lambda *a, **k: 'reference')
        saved = patch.patch_reference(H, ingest=False, matrix_build=False, **kwargs)
        assert cluster.DENSE_SEAM_BOUND is routed
        for name, idx in patch.DENSE_ARG.items():
            args = SEAM_ARGS[name]
            assert len(args) == idx
            del calls[:]
            assert getattr(H, name)(*args, True) == ('mirror' if routed else 'reference'), (name, kwargs)          # positional, as the reference calls it
            assert getattr(H, name)(*args, dense_matrix=True) == ('mirror' if routed else 'reference'), (name, kwargs)
            assert calls == ([name, name] if routed else [])
            assert getattr(H, name)(*args, False) == 'mirror'                                                      # the sparse mode: ours either way
        patch.unpatch_reference(H, saved)
        assert cluster.DENSE_SEAM_BOUND is False
        assert all(getattr(H, name)() == 'reference' for name in patch.DENSE_ARG)


@pytest.mark.parametrize('argv,world,want', [(['x.fa', 'x.pairs', '3', '--dense_matrix'], '1', True),
                                             (['x.fa', '--keep-reference-dense', 'x.pairs', '3', '--dense_matrix'], '1', False),
                                             (['x.fa', 'x.pairs', '3', '--keep-reference-statistics'], '1', True)])
def test_wrapper_flag_is_removed_and_honoured(monkeypatch, tmp_path, argv, world, want):
    """python -m haphic_amd cluster: --keep-reference-dense never reaches the reference's parser and turns the dense seam off; --dense_matrix
    itself is the reference's flag and goes through"""
    import haphic_amd
    from haphic_amd import __main__ as wrapper
    from haphic_amd import patch, ranks
    (tmp_path / 'HapHiC_cluster.py').write_text('')
    seen = {}
    H = types.ModuleType('HapHiC_cluster')
    H.parse_arguments = lambda: seen.setdefault('argv', list(sys.argv))
    H.run = lambda args, log: seen.setdefault('ran', True)
    monkeypatch.setitem(sys.modules, 'HapHiC_cluster', H)
    raw = types.SimpleNamespace(hhx_set_device=lambda d: 0)
    monkeypatch.setattr(haphic_amd, '_lib', types.SimpleNamespace(load=lambda: raw, check=lambda rc: None, files_join=lambda: None))
    monkeypatch.setattr(patch, 'patch_reference', lambda H_, **kw: seen.setdefault('patch', kw))
    monkeypatch.setattr(ranks, 'run_rank', lambda fn: fn() and 0)
    monkeypatch.setenv('WORLD_SIZE', world)
    monkeypatch.setattr(sys, 'argv', list(sys.argv))
    monkeypatch.setattr(sys, 'path', list(sys.path))
    wrapper.main(['cluster', '--reference', str(tmp_path)] + argv)
    assert seen['ran'] and '--keep-reference-dense' not in seen['argv']
    assert seen['argv'][1:] == [a for a in argv if not a.startswith('--keep-reference-')]
    assert seen['patch']['dense'] is want
    assert '--keep-reference-dense' in wrapper.__doc__
