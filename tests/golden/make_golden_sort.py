"""Writes tests/golden/sort.npz from the reference's own fast_sort (scripts/HapHiC_sort.py:470-615).

    python tests/golden/make_golden_sort.py [path/to/HapHiC/scripts]
    python tests/golden/make_golden_sort.py --search-removal        (prints REMOVAL_LENGTHS / REMOVAL_LINKS for tests/sort_cases.py)

Every case of tests/sort_cases.py runs through the unmodified fast_sort with its seams traced.  Per case and loop iteration the fixture keeps what
went into and came out of each seam: the edges of sub_HT_dict when the link matrix was built (edge_i, edge_j, edge_w), the length of every index
and the density at the edges, the sister pairs, the confidence graph as an edge list (upper triangle, non-zero) and MAXS, whether the iteration
took the removal branch, and for update() the map old index -> new index with the aggregated edges.  Per case: shape, method, cutoff, flank, the
final tour line.  Data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import sort_cases as sc      # noqa: E402


def trace(S, case):
    """{key: array} of one case; S is a private copy of the reference module"""
    out, its = {}, []
    pending = {}
    orig = {n: getattr(S, n) for n in ('dict_to_matrix', 'get_density_graph', 'get_unfiltered_confidence_graph', 'remove_shortest_path', 'update')}
    fa_dict, data = sc.group_inputs(S, case)
    HT_index_dict = data[3]

    def dict_to_matrix(d, shape, add_self_loops=False):
        if not add_self_loops:
            keys = np.array(list(d.keys()), np.int32).reshape(-1, 2)
            pending.update(edge_i=keys[:, 0], edge_j=keys[:, 1], edge_w=np.array(list(d.values()), np.float64))
        return orig['dict_to_matrix'](d, shape, add_self_loops)

    def get_density_graph(m, shape, index_HT_dict, fa, flank_HT_dict, method):
        D = orig['get_density_graph'](m, shape, index_HT_dict, fa, flank_HT_dict, method)
        pending['lengths'] = np.array([flank_HT_dict[index_HT_dict[k]][1] if index_HT_dict[k] in flank_HT_dict else S.get_len(index_HT_dict[k], fa)
                                       for k in range(shape)], np.float64)
        assert D.dtype == np.float32 and np.array_equal(D, D.T)
        pending['density'] = D[pending['edge_i'], pending['edge_j']]
        assert np.count_nonzero(D) == 2 * np.count_nonzero(pending['density'])
        return D

    def get_unfiltered_confidence_graph(shape, index_pairs, sub_HT_dict, density_graph):
        C, maxs = orig['get_unfiltered_confidence_graph'](shape, index_pairs, sub_HT_dict, density_graph)
        assert type(maxs) is np.float64 and np.array_equal(C, C.T)
        ci, cj = np.nonzero(np.triu(C, 1))
        it = dict(pending, pairs=np.array(index_pairs, np.int32).reshape(-1, 2), conf_i=ci, conf_j=cj, conf_v=C[ci, cj], maxs=np.float64(maxs),
                  removed=np.int32(0))
        pending.clear()
        its.append(it)
        return C, maxs

    def remove_shortest_path(index_pairs, sub_HT_dict, density_graph):
        its[-1]['removed'] = np.int32(1)
        return orig['remove_shortest_path'](index_pairs, sub_HT_dict, density_graph)

    def update(path_list, old, index_HT_dict, HT_idx, flank_HT_dict, fa, known_adjacency, flank):
        res = orig['update'](path_list, old, index_HT_dict, HT_idx, flank_HT_dict, fa, known_adjacency, flank)
        new_index_HT_dict, sub = res[0], res[1]
        index_map = np.full(len(HT_idx), -1, np.int32)
        for k, HT in new_index_HT_dict.items():
            for ht in S.format_HTs(flank_HT_dict[HT][0] if HT in flank_HT_dict else HT):
                assert index_map[HT_idx[ht]] == -1
                index_map[HT_idx[ht]] = k
        keys = np.array(list(sub.keys()), np.int32).reshape(-1, 2)
        vals = list(sub.values())
        assert all(type(v) is np.float32 for v in vals)
        its[-1].update(map=index_map, new_shape=np.int32(2 * len(path_list)), new_i=keys[:, 0], new_j=keys[:, 1], new_w=np.array(vals, np.float32))
        return res

    for n, fn in (('dict_to_matrix', dict_to_matrix), ('get_density_graph', get_density_graph), ('get_unfiltered_confidence_graph', get_unfiltered_confidence_graph),
                  ('remove_shortest_path', remove_shortest_path), ('update', update)):
        setattr(S, n, fn)
    try:
        paths, tour, _log = sc.run_fast_sort(S, case)
    finally:
        for n, fn in orig.items():
            setattr(S, n, fn)
    out['shape'] = np.int32(len(HT_index_dict))
    out['method'] = np.array(case.method)
    out['cutoff'] = np.float64(case.cutoff)
    out['flank'] = np.int64(case.flank)
    out['n_iter'] = np.int32(len(its))
    out['tour'] = np.array(tour.decode().splitlines()[1])
    for k, it in enumerate(its):
        for key, v in it.items():
            out['{}/{}'.format(k, key)] = v
    return out, its


def describe(its):
    return ' '.join('{}{}'.format('R' if it['removed'] else ('u%d' % it['new_shape'] if 'map' in it else 'end'), '' if 'lengths' in it else '*') for it in its)


def search_removal(S):
    """the first small random group whose trace removes a path twice in a row and then goes on to an update"""
    for seed in range(100000):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(5, 9))
        lengths = sorted((int(v) for v in rng.integers(2, 20, n) * 100_000), reverse=True)
        links = []
        for _ in range(int(rng.integers(n, 3 * n))):
            x, y = (int(v) for v in rng.integers(0, n, 2))
            if x != y:
                links.append((x, 'HT'[rng.integers(0, 2)], y, 'HT'[rng.integers(0, 2)], int(rng.choice([10, 10, 20, 30]))))
        sc.REMOVAL_LENGTHS, sc.REMOVAL_LINKS = tuple(lengths), tuple(links)
        try:
            _out, its = trace(S, sc.removal_case())
        except AssertionError:
            continue
        flags = [int(it['removed']) for it in its]
        for k in range(len(flags) - 2):
            if flags[k:k + 3] == [1, 1, 0] and (k == 0 or flags[k - 1] == 0) and 'map' in its[k + 2]:
                print('# seed', seed, describe(its))
                print('REMOVAL_LENGTHS =', tuple(lengths))
                print('REMOVAL_LINKS =', tuple(links))
                return
    raise SystemExit('no such case found')


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith('--')]
    S = sc.load_reference_sort(argv[0] if argv else sc.REFERENCE_SCRIPTS, '_haphic_sort_reference_golden')
    if '--search-removal' in sys.argv:
        return search_removal(S)
    data = {'cases': np.array([c.name for c in sc.cases()])}
    for case in sc.cases():
        out, its = trace(S, case)
        print('{:12s} shape {:4d}  {}'.format(case.name, int(out['shape']), describe(its)))
        for key, v in out.items():
            data['{}/{}'.format(case.name, key)] = v
    np.savez_compressed(sc.GOLDEN, **data)
    print(sc.GOLDEN, os.path.getsize(sc.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
