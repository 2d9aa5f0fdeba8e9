"""Writes tests/golden/sort_forest.npz from the reference's own forest block (scripts/HapHiC_sort.py fast_sort :567-595) and networkx.

    python tests/golden/make_golden_sort_forest.py [path/to/HapHiC/scripts]

Every group of tests/sort_cases.py cases() and tests/sort_forest_cases.py forest_cases() runs through the unmodified fast_sort, traced as
make_golden_sort.py traces it, with two more seams: filter_confidence_graph (the filtered array) and nxtree.maximum_spanning_tree (forest.edges()
in networkx's order; then networkx's own connected_components / subgraph / degree / shortest_path asked on that forest exactly as :576-590 ask
them, for the paths in the reference's order and direction).  The DIRECT rounds of sort_forest_cases.py go through the reference's
get_unfiltered_confidence_graph and filter_confidence_graph and the same networkx calls.

Beside what the reference produced, every round keeps the canonical answer (sort_forest_cases.forest_of_cells), and this script ASSERTS that the
canonical answer, turned into a networkx graph the way haphic_amd/sort.py bind_forest does it (nodes 0 .. shape - 1, then the chosen edges in
order) and asked the same networkx questions, gives the reference's paths, order and direction included.  It also fails unless the fixture holds
at least 20 paths that start at their larger-index end, 10 cycles cut at a tie and 3 rounds that are no set of paths.  Data only."""
import os
import sys

import networkx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden_sort as mg                  # noqa: E402
from tests import sort_cases as sc             # noqa: E402
from tests import sort_forest_cases as fc      # noqa: E402

TALLY = dict(rounds=0, paths=0, from_larger_end=0, tie_cuts=0, not_paths=0)


def reference_paths(forest):
    """what fast_sort :576-590 reads off a forest -> the paths in its order and direction, or None where it asserts"""
    paths = []
    for subnodes in networkx.connected_components(forest):
        tree = forest.subgraph(subnodes)
        ends = [node for node, degree in tree.degree() if degree == 1]
        if len(ends) != 2:
            return None
        paths.append(dict(networkx.shortest_path(tree))[ends[0]][ends[1]])
    return paths


def mirror_paths(n, eu, ev, pos):
    """the same through the graph bind_forest builds from the canonical answer; the path itself comes from pos"""
    T = networkx.Graph()
    T.add_nodes_from(range(n))
    T.add_edges_from(zip(eu.tolist(), ev.tolist()))
    paths = []
    for subnodes in networkx.connected_components(T):
        tree = T.subgraph(subnodes)
        source, target = [node for node, degree in tree.degree() if degree == 1]
        along = sorted(tree, key=lambda x: pos[x])
        paths.append(along if pos[source] < pos[target] else along[::-1])
    return paths


def record_round(C, cutoff, forest):
    """C: the filtered confidence graph; forest: what networkx's maximum_spanning_tree made of Graph(C) -> the f_* keys of one round"""
    n = C.shape[0]
    assert np.array_equal(C, C.T)
    ci, cj = np.nonzero(np.triu(C, 1))
    ref_edges = np.array([(u, v) for u, v in forest.edges()], np.int32).reshape(-1, 2)
    eu, ev, label, pos, not_paths = fc.forest_of_cells(n, ci, cj, C[ci, cj])
    paths = reference_paths(forest)
    assert (paths is None) == not_paths
    # networkx lists forest.edges() by node, the canonical answer in Kruskal's order: the same set
    assert sorted(map(tuple, ref_edges.tolist())) == sorted(zip(eu.tolist(), ev.tolist()))
    kruskal = list(networkx.tree.maximum_spanning_edges(networkx.Graph(C), algorithm='kruskal', data=False))
    assert kruskal == list(zip(eu.tolist(), ev.tolist())), 'emission order'
    out = dict(f_cutoff=np.float64(cutoff), f_filt_i=ci.astype(np.int32), f_filt_j=cj.astype(np.int32), f_filt_v=C[ci, cj],
               f_ref_eu=ref_edges[:, 0], f_ref_ev=ref_edges[:, 1], f_eu=eu, f_ev=ev, f_label=label, f_pos=pos, f_not_paths=np.int32(not_paths))
    TALLY['rounds'] += 1
    TALLY['not_paths'] += int(not_paths)
    if paths is not None:
        assert mirror_paths(n, eu, ev, pos) == paths, 'the canonical answer does not reproduce the reference\'s paths'
        out['f_paths'] = np.array([x for p in paths for x in p], np.int32)
        out['f_path_off'] = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
        TALLY['paths'] += len(paths)
        TALLY['from_larger_end'] += sum(p[0] > p[-1] for p in paths)
        chosen = set(zip(eu.tolist(), ev.tolist()))
        where = {}
        for p in paths:
            for k, x in enumerate(p):
                where[x] = (id(p), k, p)
        for u, v in zip(ci.tolist(), cj.tolist()):            # an edge left out closed a cycle: tied when an edge of that cycle weighs the same
            if (u, v) not in chosen:
                _pid, a, p = where[u]
                b = where[v][1]
                lo, hi = min(a, b), max(a, b)
                TALLY['tie_cuts'] += any(C[p[k], p[k + 1]] == C[u, v] for k in range(lo, hi))
    return out


def trace(S, case):
    """make_golden_sort.trace plus the forest rounds; a group whose forest forks ends at the reference's assert and keeps its rounds up to there"""
    forests = {}
    state = dict(it=-1, C=None, cutoff=None)
    orig_conf, orig_filter, orig_tree, orig_run = S.get_unfiltered_confidence_graph, S.filter_confidence_graph, S.nxtree, sc.run_fast_sort

    def get_unfiltered_confidence_graph(*a):
        state['it'] += 1
        return orig_conf(*a)

    def filter_confidence_graph(C, sub_HT_dict, cutoff):
        orig_filter(C, sub_HT_dict, cutoff)
        state.update(C=C.copy(), cutoff=cutoff)

    class Tree:
        def __getattr__(self, name):
            return getattr(orig_tree, name)

        def maximum_spanning_tree(self, G, **kw):
            assert kw == {'algorithm': 'kruskal'}
            forest = orig_tree.maximum_spanning_tree(G, **kw)
            forests[state['it']] = record_round(state['C'], state['cutoff'], forest)
            return forest

    def run_fast_sort(S_, case_, log=None):
        try:
            return orig_run(S_, case_, log)
        except AssertionError:
            return None, b'#\nFORKED\n', []

    S.get_unfiltered_confidence_graph, S.filter_confidence_graph, S.nxtree, sc.run_fast_sort = (get_unfiltered_confidence_graph, filter_confidence_graph,
                                                                                                Tree(), run_fast_sort)
    try:
        out, its = mg.trace(S, case)
    finally:
        S.get_unfiltered_confidence_graph, S.filter_confidence_graph, S.nxtree, sc.run_fast_sort = orig_conf, orig_filter, orig_tree, orig_run
    for it, rec in forests.items():
        for key, v in rec.items():
            out['{}/{}'.format(it, key)] = v
    for key in [k for k in out if k.split('/')[-1] in ('density', 'conf_i', 'conf_j', 'conf_v', 'new_i', 'new_j') or
                (k.split('/')[-1].startswith('edge_') and k.split('/')[0] != '0')]:
        del out[key]                                       # pinned by tests/golden/sort.npz already; not needed to replay
    return out, its, forests


def direct(S, spec):
    """one round from edges, equal lengths ('sum') and sister pairs, through the reference's confidence and filter functions"""
    n = spec['shape']
    e = np.array(spec['edges'], np.int64)
    lengths = np.full(n, 500_000.0)
    sub = {(int(a), int(b)): int(w) for a, b, w in e}
    Smat = np.zeros((n, n), np.float32)
    Smat[e[:, 0], e[:, 1]] = e[:, 2]
    Smat[e[:, 1], e[:, 0]] = e[:, 2]
    L = (lengths[:, None] + lengths[None, :]).astype(np.float32)
    np.fill_diagonal(L, 1)
    pairs = [tuple(p) for p in spec['pairs']]
    C, maxs = S.get_unfiltered_confidence_graph(n, pairs, sub, Smat / L)
    S.filter_confidence_graph(C, sub, spec['cutoff'])
    forest = S.nxtree.maximum_spanning_tree(S.Graph(C), algorithm='kruskal')
    out = dict(shape=np.int32(n), method=np.array('sum'), cutoff=np.float64(spec['cutoff']), flank=np.int64(0), n_iter=np.int32(1), tour=np.array('DIRECT'))
    it = dict(edge_i=e[:, 0].astype(np.int32), edge_j=e[:, 1].astype(np.int32), edge_w=e[:, 2].astype(np.float64), lengths=lengths,
              pairs=np.array(pairs, np.int32), maxs=np.float64(maxs), removed=np.int32(0))
    it.update(record_round(C, spec['cutoff'], forest))
    for key, v in it.items():
        out['0/{}'.format(key)] = v
    return out


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith('--')]
    S = sc.load_reference_sort(argv[0] if argv else sc.REFERENCE_SCRIPTS, '_haphic_sort_reference_forest_golden')
    data = {'cases': np.array(fc.all_case_names())}
    for case in fc.fast_sort_cases():
        out, its, forests = trace(S, case)
        print('{:14s} shape {:4d}  {}  forests {}  {}'.format(case.name, int(out['shape']), mg.describe(its), len(forests), str(out['tour'])[:6]))
        for key, v in out.items():
            data['{}/{}'.format(case.name, key)] = v
    for name, spec in fc.DIRECT.items():
        for key, v in direct(S, spec).items():
            data['{}/{}'.format(name, key)] = v
    for name, want in (('direct_sisters_only', 0), ('direct_twin', 0), ('direct_twin_fork', 1)):
        assert int(data[name + '/0/f_not_paths']) == want, name
    assert len(data['direct_sisters_only/0/f_eu']) == 2 and len(data['cycle4/0/f_eu']) == 3
    removed_then_forest = own_list = False
    for case in fc.fast_sort_cases():
        seen_removed = False
        for it in range(int(data[case.name + '/n_iter'])):
            has = '{}/{}/f_cutoff'.format(case.name, it) in data
            own_list |= has and it > 0 and any('{}/{}/map'.format(case.name, k) in data for k in range(it))
            removed_then_forest |= has and seen_removed and '{}/{}/lengths'.format(case.name, it) not in data
            seen_removed = bool(data['{}/{}/removed'.format(case.name, it)])
    print(TALLY, 'forest after a removal:', removed_then_forest, 'forest on a re-aggregated list:', own_list)
    assert removed_then_forest and own_list
    assert TALLY['from_larger_end'] >= 20 and TALLY['tie_cuts'] >= 10 and TALLY['not_paths'] >= 3, TALLY
    np.savez_compressed(fc.GOLDEN, **data)
    size = os.path.getsize(fc.GOLDEN)
    print(fc.GOLDEN, size, 'bytes')
    assert size < 1 << 20


if __name__ == '__main__':
    main()
