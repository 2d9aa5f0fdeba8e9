"""--remove_allelic_links on the array-backed containers (haphic_amd/allelic.py) without a GPU: the mirror with the numpy engine of
tests/allelic_cases.py (the C oracle's ingest + the two engine methods restated in numpy) against what the REFERENCE's
remove_allelic_HiC_links :474-692 did on the same inputs (tests/golden/allelic.npz, tests/golden/make_golden_allelic.py), the fall-backs to
the reference's function, and the binding (patch_reference(allelic=), --keep-reference-allelic)."""
import logging
import sys
import types

import numpy as np
import pytest

from tests import allelic_cases
from tests.conftest import load_golden

CASES = {c.name: c for c in allelic_cases.cases()}


@pytest.fixture()
def mirror(monkeypatch):
    """haphic_amd.cluster / allelic bound to the oracle-backed library, and an empty THAW_LOG"""
    import haphic_amd
    from haphic_amd import allelic, cluster, containers
    lib = allelic_cases.library()
    monkeypatch.setattr(cluster, '_lib', lib)
    monkeypatch.setattr(haphic_amd, '_lib', lib)
    monkeypatch.setattr(containers, 'THAW_LOG', [])
    return types.SimpleNamespace(cluster=cluster, allelic=allelic, containers=containers, lib=lib)


def frozen_groups(g, case):
    t = case.name + '_'
    ptr = g[t + 'group_ptr'].tolist()
    return [tuple(case.names[c] for c in g[t + 'group_ctg'][a:b]) for a, b in zip(ptr[:-1], ptr[1:])]


def check_verdict(got, g, case, cluster, exact_weights=True):
    """what run_mirror() returns against the frozen reference run.  exact_weights=False (the HIP library): normalize_by_nlinks divides by
    sqrt(a * b) where Python's (a * b) ** 0.5 is C pow(), which is not always the correctly rounded root — the divisor may be 1 ulp off, the
    quotient then 2 ulp (4.5e-16 relative), in a small share of the keys: the bound tests/test_gpu_pipeline.py sets for that kernel."""
    t = case.name + '_'
    n_ctg, n_frag = len(case.names), len(case.frag_names)
    assert case.checksum == int(g[t + 'checksum']), 'the case is not the one the fixture was made from'
    pre_i, pre_j = got['pre_full']
    assert np.array_equal(pre_i, g[t + 'full_i']) and np.array_equal(pre_j, g[t + 'full_j'])
    assert np.array_equal(got['pre_flank'][0], g[t + 'flank_i']) and np.array_equal(got['pre_flank'][1], g[t + 'flank_j'])
    s1 = g[t + 'stage1']
    assert np.array_equal(got['stage1'][0], pre_i[s1]) and np.array_equal(got['stage1'][1], pre_j[s1]), 'stage-1 keys (inter_allele_dict, in order)'
    full, flank = got['full'], got['flank']
    assert full.frozen and flank.frozen
    fi, fj, cnt, _ = full.arrays()
    assert np.array_equal(allelic_cases.removed_mask(pre_i, pre_j, fi, fj, n_ctg), g[t + 'full_removed'])
    assert np.array_equal(fi, g[t + 'pkl_i']) and np.array_equal(fj, g[t + 'pkl_j']) and np.array_equal(cnt, g[t + 'pkl_cnt']), 'full_links.pkl items'
    ki, kj, val, _ = flank.arrays()
    assert np.array_equal(allelic_cases.removed_mask(got['pre_flank'][0], got['pre_flank'][1], ki, kj, n_frag), g[t + 'flank_removed'])
    assert (len(full), len(flank)) == (len(fi), len(ki)) == (int((~g[t + 'full_removed']).sum()), int((~g[t + 'flank_removed']).sum()))
    if case.normalize:
        assert val.dtype == np.float64 and len(val) == len(g[t + 'flank_val'])
        if exact_weights:
            assert np.array_equal(val, g[t + 'flank_val']), 'the weights of the surviving flank keys'
        else:
            np.testing.assert_allclose(val, g[t + 'flank_val'], rtol=4.5e-16, atol=0)
            assert (val != g[t + 'flank_val']).mean() < 0.01
    remaining = got['remaining']
    assert isinstance(remaining, set) and [f in remaining for f in case.frag_names] == g[t + 'remaining'].tolist()
    mat, fidx = cluster.dict_to_matrix(flank, remaining, dense_matrix=False, add_self_loops=True, _device=True)
    assert [fidx.get(f, -1) for f in case.frag_names] == g[t + 'frag_index'].tolist() and mat.nnz == int(g[t + 'matrix_nnz'])


@pytest.fixture(scope='module')
def golden():
    return load_golden('allelic.npz')


@pytest.mark.parametrize('name', list(CASES))
def test_concordance_ratios_of_the_numpy_engine(mirror, golden, name):
    """max(diag / m, anti / m) from the integer counts == cal_concordance_ratio of the reference for every eligible key, bit for bit"""
    case = CASES[name]
    full, _flank, _fl, _coord, _c2f = case.parse(mirror.cluster)
    m, diag, anti = full._session.ing.concordance_counts(case.max_read_pairs, 50, case.min_read_pairs)
    cnt = full.arrays()[2]
    eligible = (cnt >= case.max_read_pairs) | (m >= case.min_read_pairs)
    assert np.array_equal(eligible, golden[name + '_eligible'])
    assert not diag[~eligible].any() and not anti[~eligible].any()
    ratio = np.maximum(diag[eligible] / m[eligible], anti[eligible] / m[eligible])
    assert np.array_equal(ratio.view(np.uint64), golden[name + '_ratio'][eligible].view(np.uint64))
    assert not mirror.containers.THAW_LOG


@pytest.mark.parametrize('name', list(CASES))
def test_mirror_reproduces_the_reference_verdict_with_frozen_groups(mirror, golden, name):
    case = CASES[name]
    groups = frozen_groups(golden, case) if case.ploidy > 2 else None
    got = allelic_cases.run_mirror(case, mirror.cluster, mirror.allelic, groups=groups)
    assert not mirror.containers.THAW_LOG, mirror.containers.THAW_LOG
    check_verdict(got, golden, case, mirror.cluster)
    assert mirror.allelic.STATS['stage2_keys'] == int(golden[name + '_nonmax'].sum()) and mirror.allelic.STATS['group_pairs'] > 0


@pytest.mark.parametrize('name', list(CASES))
def test_allele_groups_and_the_whole_mirror(mirror, golden, name):
    """with networkx: the cliques, split as :511-550 do, are the reference's allele groups, and the mirror needs nothing injected"""
    pytest.importorskip('networkx')
    case = CASES[name]
    got = allelic_cases.run_mirror(case, mirror.cluster, mirror.allelic)
    check_verdict(got, golden, case, mirror.cluster)
    s1 = golden[name + '_stage1']
    full_i, full_j = golden[name + '_full_i'][s1], golden[name + '_full_j'][s1]
    # the groups themselves (the counts matter for the weakest edge: take them from a fresh parse)
    full, *_ = case.parse(mirror.cluster)
    cnt = full.arrays()[2][s1]
    groups = mirror.allelic.allele_groups(full_i, full_j, cnt, case.names, case.ploidy)
    assert sorted(groups) == sorted(frozen_groups(golden, case)) and len(set(groups)) == len(groups)


def test_dense_matrix_graph_equals_the_edge_list_graph(mirror, golden):
    """_edges_graph builds what networkx makes of the dense float32 matrix of dict_to_matrix :603-606: same nodes, same adjacency ORDER"""
    nx = pytest.importorskip('networkx')
    case = CASES['p4']
    s1 = golden['p4_stage1']
    full, *_ = case.parse(mirror.cluster)
    fi, fj, cnt, _ = full.arrays()
    graph, index_ctg = mirror.allelic._edges_graph(fi[s1], fj[s1], cnt[s1])
    n = len(index_ctg)
    dense = np.zeros((n, n), np.float32)
    at = {c: k for k, c in enumerate(index_ctg.tolist())}
    for a, b, c in zip(fi[s1].tolist(), fj[s1].tolist(), cnt[s1].tolist()):
        dense[at[a], at[b]] = dense[at[b], at[a]] = c
    want = nx.Graph(dense)
    assert list(want.nodes) == list(graph.nodes)
    assert [(u, list(nb.items())) for u, nb in want.adjacency()] == [(u, list(nb.items())) for u, nb in graph.adjacency()]
    assert list(want.edges(data=True)) == list(graph.edges(data=True))


# ------------------------------------------------------------------ fall-backs
def _call(mirror, case, tweak, engine=None, groups=()):
    """remove_allelic_HiC_links with one precondition broken by `tweak(kw)`; the original is a stand-in that walks the dicts as :579 / :634 do"""
    full, flank, frag_link, coord, c2f = case.parse(mirror.cluster)
    calls = []

    def original(fa_dict, ctg_coord_dict, full_link_dict, args, flank_link_dict=None, filtered_frags=None, ctg_pair_to_frag=None, logger=None):
        calls.append((ctg_coord_dict, full_link_dict, flank_link_dict))
        for key, _data in ctg_coord_dict.items():
            full_link_dict[key]
        if flank_link_dict:
            for _key in flank_link_dict:
                pass
        return {'from the original'}
    kw = dict(fa_dict=case.fa_dict(), ctg_coord_dict=coord, full_link_dict=full, args=case.args(), flank_link_dict=flank,
              filtered_frags=set(case.filtered), ctg_pair_to_frag=c2f, _original=original, _engine=engine)
    tweak(kw)
    real = mirror.allelic.allele_groups
    mirror.allelic.allele_groups = lambda *a: list(groups)
    try:
        out = mirror.allelic.remove_allelic_HiC_links(**kw)
    finally:
        mirror.allelic.allele_groups = real
    return out, calls, kw


def _set(obj, name, value):
    setattr(obj, name, value)


class _NoMethods:
    pass


class _Refuses:
    def concordance_counts(self, *a, **k):
        return None

    def drop_links(self, *a, **k):
        raise AssertionError('not reached')


FALLBACKS = {
    'concentrated links on': lambda kw: _set(kw['args'], 'remove_concentrated_links', True),
    'ultra-long reads': lambda kw: _set(kw['args'], 'ul', 'ul.bam'),
    'no filtered_frags': lambda kw: kw.update(filtered_frags=None),
    'flank dict empty': lambda kw: kw.update(flank_link_dict={}),
    'flank dict already a real dict': lambda kw: kw.update(flank_link_dict=dict(kw['flank_link_dict'].items())),
    'full dict thawed': lambda kw: kw['full_link_dict']._thaw(),
    'coordinate lists thawed': lambda kw: kw['ctg_coord_dict']._thaw(),
    'a contig shorter than nwindows': lambda kw: _set(kw['args'], 'nwindows', 10 ** 7),
    'max_read_pairs beyond the cap': lambda kw: _set(kw['args'], 'max_read_pairs', allelic_cases.CAP + 1),
    'a name outside the table': lambda kw: kw['filtered_frags'].add('not_a_fragment'),
    'ctg_pair_to_frag on unsplit contigs': lambda kw: kw.update(ctg_pair_to_frag={('a', 'b'): {('a', 'b')}}),
    'debug logger': lambda kw: kw.update(logger=_debug_logger()),
    'engine without the methods': lambda kw: kw.update(_engine=_NoMethods()),
    'engine refuses': lambda kw: kw.update(_engine=_Refuses()),
}


def _debug_logger():
    log = logging.getLogger('allelic_test_debug')
    log.setLevel(logging.DEBUG)
    log.propagate = False
    return log


@pytest.mark.parametrize('why', list(FALLBACKS))
def test_falls_back_to_the_original_which_thaws(mirror, why):
    case = CASES['p2']
    out, calls, kw = _call(mirror, case, FALLBACKS[why])
    assert out == {'from the original'} and len(calls) == 1, why
    # the same objects, in the reference's argument order, and the walk of the original thawed what was still frozen
    assert calls[0] == (kw['ctg_coord_dict'], kw['full_link_dict'], kw['flank_link_dict'])
    assert not getattr(kw['full_link_dict'], 'frozen', False) and not getattr(kw['ctg_coord_dict'], 'frozen', False)
    thawed = {k for k, _n, _s in mirror.containers.THAW_LOG}
    assert {'full', 'crd'} <= thawed
    assert len(kw['full_link_dict']) == len(kw['ctg_coord_dict']) == 5053      # nothing was dropped before the hand-over


def test_without_an_original_the_fallback_is_an_error(mirror):
    case = CASES['p2']
    with pytest.raises(ValueError, match='reference function'):
        _call(mirror, case, lambda kw: (kw.update(_original=None), _set(kw['args'], 'ul', 'x')))


def test_assert_of_the_reference_goes_to_the_original(mirror):
    """:653 — group_pair[0] holds ctg_1 but group_pair[1] does not hold ctg_2: nonmax_keys reports it, the mirror lets the reference raise"""
    from haphic_amd import allelic
    names = ['a', 'b', 'c', 'd']
    rank = np.arange(4, dtype=np.int32)
    # key (a, c): a is in both groups, c only in the lower-ranked one -> for group_1 = (a, d), group_2 = (a, c): pair = ((a, c), (a, d)), ctg_1 = a is
    # in pair[0] and ctg_2 = c is not in pair[1]
    got = allelic.nonmax_keys(np.array([0]), np.array([2]), np.array([5]), [('a', 'c'), ('a', 'd')], names, rank)
    assert got is None
    ok = allelic.nonmax_keys(np.array([0]), np.array([2]), np.array([5]), [('a', 'b'), ('c', 'd')], names, rank)
    assert ok is not None and ok.tolist() == [False]


def test_nonmax_keys_against_the_loop_of_the_reference_restated(mirror):
    """:621-667 written out per key (dicts, one assignment per group pair) on random groups and keys == nonmax_keys on arrays"""
    from scipy.optimize import linear_sum_assignment
    from haphic_amd import allelic
    rng = np.random.default_rng(5)
    names = ['c%03d' % k for k in range(60)]
    order = sorted(range(60), key=names.__getitem__)
    rank = np.empty(60, np.int32)
    rank[order] = np.arange(60)
    groups = []
    pool = rng.permutation(60)
    for k in range(0, 48, 4):                                     # disjoint groups of 2-4, plus two that share contigs with others
        groups.append(tuple(sorted(names[c] for c in pool[k:k + int(rng.integers(2, 5))])))
    groups.append(tuple(sorted(names[c] for c in (pool[0], pool[5], pool[50]))))
    groups.append(tuple(sorted(names[c] for c in (pool[9], pool[51]))))
    in_group = [set(g) for g in groups]
    keys = {}
    while len(keys) < 600:
        a, b = sorted(rng.integers(0, 60, 2).tolist(), key=lambda c: names[c])
        if a != b and not any(names[a] in g and names[b] in g for g in in_group):
            keys[(a, b)] = int(rng.integers(1, 6))                # small counts: ties in the assignment problems
    si, sj, scnt = np.array([k[0] for k in keys]), np.array([k[1] for k in keys]), np.array(list(keys.values()))
    got = allelic.nonmax_keys(si, sj, scnt, groups, names, rank)
    full = {(names[a], names[b]): c for (a, b), c in keys.items()}
    by_ctg = {}
    for g in groups:
        for c in g:
            by_ctg.setdefault(c, set()).add(g)
    want, hit_assert = [], False
    for (c1, c2) in full:
        bad = False
        for g1 in by_ctg.get(c1, ()):
            for g2 in by_ctg.get(c2, ()) if c1 in by_ctg else ():
                pair = tuple(sorted([g1, g2]))
                d = max(len(pair[0]), len(pair[1]))
                mat = np.zeros((d, d), dtype=int)
                for i1, x in enumerate(pair[0]):
                    for i2, y in enumerate(pair[1]):
                        mat[i1, i2] = full.get(tuple(sorted([x, y])), 0)
                sol = linear_sum_assignment(-mat)
                if c1 in pair[0]:
                    if c2 not in pair[1]:
                        hit_assert = True
                        continue
                    i1, i2 = pair[0].index(c1), pair[1].index(c2)
                else:
                    i1, i2 = pair[0].index(c2), pair[1].index(c1)
                bad |= sol[1][i1] != i2
        want.append(bool(bad) if c1 in by_ctg and c2 in by_ctg else False)
    if hit_assert:
        assert got is None
    else:
        assert got.tolist() == want and any(want) and not all(want)


# ------------------------------------------------------------------ binding
def test_patch_reference_binds_the_seam_only_on_request(mirror, monkeypatch):
    from haphic_amd import patch
    monkeypatch.setattr(patch, '_lib', mirror.lib, raising=False)
    sentinel = lambda *a, **k: 'reference'                       # noqa: E731
    for kwargs, bound in (({}, False), ({'allelic': False}, False), ({'allelic': True}, True), ({'allelic': True, 'ingest': False}, False)):
        H = types.ModuleType('H')
        H.remove_allelic_HiC_links = sentinel
        saved = patch.patch_reference(H, **kwargs)
        assert (H.remove_allelic_HiC_links is not sentinel) == bound, kwargs
        assert ('remove_allelic_HiC_links' in saved) == bound
        if bound:
            assert H.remove_allelic_HiC_links.__wrapped__ is mirror.allelic.remove_allelic_HiC_links
            assert saved['remove_allelic_HiC_links'] is sentinel
            # the original travels with the seam: a call the array path does not serve reaches it with the reference's arguments
            assert H.remove_allelic_HiC_links({}, {}, {}, types.SimpleNamespace(), {}, set()) == 'reference'
        patch.unpatch_reference(H, saved)
        assert H.remove_allelic_HiC_links is sentinel
    assert 'remove_allelic_HiC_links' not in patch.SEAMS and 'remove_allelic_HiC_links' not in patch.OPTIONAL


@pytest.mark.parametrize('argv,world,want', [(['x.fa', 'x.pairs', '3', '--remove_allelic_links', '4'], '1', True),
                                             (['x.fa', '--keep-reference-allelic', 'x.pairs', '3'], '1', False),
                                             (['x.fa', 'x.pairs', '3', '--keep-reference-ingest'], '1', True)])
def test_wrapper_flag_is_removed_and_honoured(mirror, monkeypatch, tmp_path, argv, world, want):
    """python -m haphic_amd cluster: --keep-reference-allelic never reaches the reference's parser and turns the seam off"""
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
    assert seen['ran'] and '--keep-reference-allelic' not in seen['argv']
    assert seen['argv'][1:] == [a for a in argv if a not in ('--keep-reference-allelic', '--keep-reference-ingest')]
    assert seen['patch']['allelic'] is want and seen['patch']['ingest'] is ('--keep-reference-ingest' not in argv)
    assert '--keep-reference-allelic' in wrapper.__doc__


# ------------------------------------------------------------------ the existing fixtures
def test_ratio_from_integer_counts_equals_coord_stats():
    """tests/golden/coord_stats.npz: cal_concordance_ratio of the reference on 60 coordinate lists"""
    g = load_golden('coord_stats.npz')
    n = len(g['shorter'])
    counts = allelic_cases.modal_counts(g['ptr'], g['coords'], g['shorter'], np.arange(n), np.arange(n), 50, 0)
    m, diag, anti = counts
    assert np.array_equal(np.maximum(diag / m, anti / m).view(np.uint64), g['concordance'].view(np.uint64))


@pytest.fixture(scope='module')
def c4():
    from haphic_amd import synth
    g = load_golden('pipeline_c4.npz')
    base = synth.make_genome(3, 3_000_000, 60_000, cv=0.3, min_len=8000, seed=4040)
    gen = synth.make_polyploid(base, 4)
    id1, p1, id2, p2 = [t.numpy() for t in synth.sample_pairs(gen, 400_000, seed=4041, cis=0.9)]
    id1, p1, id2, p2 = synth.add_allelic_pairs(gen, base.n, 4, id1, p1, id2, p2, 0.08, 4042)
    keep = id1 != id2
    id1, p1, id2, p2 = id1[keep], p1[keep], id2[keep], p2[keep]
    if int(id1.sum() + p1.sum() + id2.sum() + p2.sum()) != int(g['pairs_checksum']):
        pytest.skip('torch CPU generator differs from the one that made the fixture')
    return g, gen, (id1, p1, id2, p2)


def c4_run(c4, cluster, allelic):
    """pipeline_c4.npz (624 contigs, 46,677 keys, ploidy 4) through the mirror: (full, flank, remaining, names, session)"""
    g, gen, (id1, p1, id2, p2) = c4
    names = list(gen.names)
    fa_dict = {n: [None, int(l), int(r)] for n, l, r in zip(names, gen.length, gen.re_sites)}
    args = types.SimpleNamespace(flank=500, remove_allelic_links=4, remove_concentrated_links=False, max_read_pairs=40, min_read_pairs=20,
                                 concordance_ratio_cutoff=0.2, nwindows=50, ul=None, skip_clustering=True)
    aln = cluster.IdArrays(names, id1, p1, id2, p2)
    full, flank, _ht, _clm, _fl, coord = cluster.parse_alignments_for_ctgs(aln, fa_dict, args, {n: fa_dict[n][1] for n in names}, set(names), 'int32', 'int32')
    pre = full.arrays()[:2], flank.arrays()[:2]
    remaining = allelic.remove_allelic_HiC_links(fa_dict, coord, full, args, flank, set(names))
    return full, flank, remaining, names, pre


def c4_check(c4, got, cluster):
    g = c4[0]
    full, flank, remaining, names, (pre_full, pre_flank) = got
    n = len(names)
    fi, fj, _c, _n = full.arrays()
    ki, kj, _v, _n = flank.arrays()
    assert np.array_equal(allelic_cases.removed_mask(*pre_full, fi, fj, n), g['full_removed'])
    assert np.array_equal(allelic_cases.removed_mask(*pre_flank, ki, kj, n), g['flank_removed'])
    assert [f in remaining for f in names] == g['remaining'].tolist()
    mat, fidx = cluster.dict_to_matrix(flank, remaining, dense_matrix=False, add_self_loops=True, _device=True)
    assert [fidx.get(f, -1) for f in names] == g['frag_index'].tolist()


def test_pipeline_c4_collapsed_ratios_from_integer_counts(mirror, c4):
    """coord_ratio of tests/golden/pipeline_c4.npz (the [ratio, 1] entries the reference collapsed at max_read_pairs, :460-465), bit for bit"""
    g, gen, (id1, p1, id2, p2) = c4
    names = list(gen.names)
    table = mirror.cluster.FragTable.for_contigs(gen.lexical_rank(), gen.length, np.ones(len(names), np.uint8), names)
    ing = mirror.lib.Ingest(table, 500_000, bins=False, skip_intra=True)
    ing.push(id1, p1, id2, p2)
    m, diag, anti = ing.concordance_counts(40, 50, 20)
    o = ing.fetch()
    assert np.array_equal(o['full_i'], g['coord_i']) and np.array_equal(o['full_j'], g['coord_j'])
    col = g['coord_collapsed']
    assert np.array_equal(col, o['full_cnt'] >= 40) and int(col.sum()) == 1260
    assert np.array_equal(np.maximum(diag[col] / m[col], anti[col] / m[col]).view(np.uint64), g['coord_ratio'][col].view(np.uint64))


def test_pipeline_c4_whole_mirror(mirror, c4):
    pytest.importorskip('networkx')
    g = c4[0]
    got = c4_run(c4, mirror.cluster, mirror.allelic)
    assert not mirror.containers.THAW_LOG
    c4_check(c4, got, mirror.cluster)
    st = mirror.allelic.STATS
    assert (st['keys'], st['stage1_keys'], st['stage1_keys'] + st['stage2_keys']) == (46677, 828, int(g['full_removed'].sum()))
