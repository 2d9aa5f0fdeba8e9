#!/usr/bin/env python3
"""Measures the device work of `haphic sort`'s fast sorting (haphic_amd/csrc/hhx_sort.hip) on one synthetic group and writes
profiles/sort_bench.json.  A record, not a gate.

    python tools/sort_bench.py [--contigs 3000] [--out profiles/sort_bench.json]
    python tools/sort_bench.py --reference-only --reference path/to/HapHiC/scripts [--prefix 600]      (no GPU: times the reference alone)
    python tools/sort_bench.py --forest-bench [--sizes 3000,10000] [--repeats 3] [--parent FILE]       (writes profiles/sort_forest_bench.json)

--forest-bench times the forest block of every round both ways on the same groups in one process: the host way (the confidence array copied to the
host, filtered there, networkx's Graph / maximum_spanning_tree / one shortest_path per tree) and the device way of haphic_amd/sort.py bind_forest
(confidence_device, one forest() call, the networkx graph of the chosen edges with networkx's components and ends, the paths read off the
positions).  --parent: a JSON file {contigs: [wall seconds ...]} measured with this tool's loop at the parent commit in the same session.

The group: --contigs contigs (default 3000, shape 6000) planted as a chain in a random order and orientation (tests/sort_cases.chain_case: strong
links between neighbours, weaker ones two and three steps away, noise), default density method ('multiplication'), cutoff 1, no flanking region.
The device run drives _lib.SortGraph through the rounds with a loop of its own — the reference checkout does not exist where the GPU is — that does
what fast_sort :529-605 does per round: density, confidence, filter, networkx's maximum spanning forest, paths, the map old end -> new end (each
path cut into two halves of about the same length; the stand-in for the work update() does on names), re-aggregation.  Per round and in total it
reports the HIP-event time of every kernel class and of the copy of the confidence array, the wall time of each call, of the forest and of
the map-making.  For scale the reference's own functions are timed where the checkout exists, inside its unmodified fast_sort on one core, on
the largest prefix of the same group (the first --prefix contigs along the planted chain and the links among them) that finishes in a few minutes there; elsewhere that
record is carried over, labelled `stored: true`.  The two records are different sizes on different machines: read them side by side, not as a ratio."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sort_cases as sc      # noqa: E402

KERNELS = ('sort_matrix', 'sort_density', 'sort_confidence', 'sort_aggregate', 'sort_emit')
COPIES = ('sort_confidence_copy',)
FOREST_KERNELS = ('sort_forest_lds', 'sort_forest_edges', 'sort_forest_round', 'sort_forest_emit', 'sort_forest_jump')      # the radix sort of the HBM form is untimed
SEED = 4242


def group(n):
    return sc.chain_case('bench%d' % n, n, SEED, strong=(60, 120), noise=3.0)


def prefix_of(case, n):
    """the first n contigs along the planted chain (neighbours are the contigs joined by a strong link: 60 or more) and the links among them"""
    near = {}
    for (a, b), w in case.links.items():
        if w >= 60:
            near.setdefault(a[:-2], []).append(b[:-2])
            near.setdefault(b[:-2], []).append(a[:-2])
    at = min(c for c, v in near.items() if len(v) == 1)
    keep, last = [at], None
    while len(keep) < n:
        step = [c for c in near[at] if c != last]
        if not step:
            break
        last, at = at, step[0]
        keep.append(at)
    keep = set(keep)
    links = {k: v for k, v in case.links.items() if k[0][:-2] in keep and k[1][:-2] in keep}
    return case._replace(name='%s_prefix%d' % (case.name, n), ctgs=[c for c in case.ctgs if c[0] in keep], links=links)


def edges_of(case):
    """contig k (by length, longest first) -> ends 2k (H), 2k + 1 (T); -> shape, (i, j, w), the length of every end"""
    info = sorted(case.ctgs, key=lambda x: x[1], reverse=True)
    index = {}
    for k, (c, _) in enumerate(info):
        index[c + '_H'], index[c + '_T'] = 2 * k, 2 * k + 1
    keys = np.array([(index[a], index[b]) for a, b in case.links], np.int32)
    return 2 * len(info), (keys[:, 0], keys[:, 1], np.array(list(case.links.values()), np.int64)), np.repeat([ln / 2 for _, ln in info], 2)


def device_run(case, cutoff=1.0, profile=True, forest='host'):
    """forest: 'host' — the array comes to the host and networkx builds the forest; 'device' — SortGraph.forest and the read-out of bind_forest"""
    import networkx as nx
    from haphic_amd import _lib
    from haphic_amd import sort as hsort
    kernels = KERNELS + (FOREST_KERNELS if forest == 'device' else ())
    shape, (ei, ej, w), end_len = edges_of(case)
    clock = time.perf_counter
    rounds = []
    t_all = clock()
    _lib.profile_reset()
    _lib.profile_enable(profile)
    try:
        t0 = clock()
        eng = _lib.SortGraph(shape, ei, ej, w)
        create_s = clock() - t0
        create_events = {k: _lib.profile_get(k)[0] for k in kernels + COPIES}
        members = [[k] for k in range(shape)]            # the old ends behind every current index
        cur_i, cur_j = ei.astype(np.int64), ej.astype(np.int64)
        pairs = np.arange(shape, dtype=np.int32).reshape(-1, 2)
        fresh = True
        while len(pairs) > 1:
            _lib.profile_reset()
            rec = {'shape': eng.shape, 'edges': int(cur_i.size)}
            if fresh:
                t0 = clock()
                eng.density([float(sum(end_len[m] for m in ms)) for ms in members], 'multiplication')
                rec['density_call_s'] = clock() - t0
            t0 = clock()
            if forest == 'device':
                C, maxs = None, eng.confidence_device(pairs[:, 0], pairs[:, 1])
            else:
                C, maxs = eng.confidence(pairs[:, 0], pairs[:, 1])
                rec['confidence_bytes'] = int(C.nbytes)
            rec['confidence_call_s'] = clock() - t0
            rec['maxs'] = float(maxs)
            if maxs <= cutoff:
                if len(pairs) <= 2:
                    rec['events_ms'] = {k: _lib.profile_get(k)[0] for k in kernels + COPIES}
                    rounds.append(rec)
                    break
                a, b = (int(v) for v in pairs[-1])
                pairs = pairs[:-1]
                keep = ~(np.isin(cur_i, (a, b)) | np.isin(cur_j, (a, b)))
                cur_i, cur_j = cur_i[keep], cur_j[keep]
                eng.drop(a, b)
                fresh = False
                rec['removed'] = True
                rec['events_ms'] = {k: _lib.profile_get(k)[0] for k in kernels + COPIES}
                rounds.append(rec)
                continue
            paths = []
            if forest == 'device':
                t0 = clock()
                eu, ev, _label, pos, not_paths = eng.forest(cutoff)
                rec['forest_call_s'] = clock() - t0
                assert not not_paths
                t0 = clock()
                T = nx.Graph()
                T.add_nodes_from(range(eng.shape))
                T.add_edges_from(zip(eu.tolist(), ev.tolist()))
                pos = pos.tolist()
                trees = []
                for nodes in nx.connected_components(T):
                    tree = T.subgraph(nodes)
                    trees.append((tree, [v for v, d in tree.degree() if d == 1]))
                rec['tree_ends_s'] = clock() - t0
                t0 = clock()
                for tree, ends in trees:
                    path = dict(hsort.ForestPaths(tree, pos))[ends[0]][ends[1]]
                    paths.append((path, sum(end_len[m] for v in path for m in members[v])))
                rec['paths_s'] = clock() - t0
            else:
                t0 = clock()
                low = C[cur_i, cur_j] <= cutoff
                C[cur_i[low], cur_j[low]] = 0
                C[cur_j[low], cur_i[low]] = 0
                rec['filter_s'] = clock() - t0
                t0 = clock()
                host_forest = nx.tree.maximum_spanning_tree(nx.Graph(C), algorithm='kruskal')
                rec['forest_s'] = clock() - t0
                t0 = clock()
                for nodes in nx.connected_components(host_forest):
                    tree = host_forest.subgraph(nodes)
                    ends = [v for v, d in tree.degree() if d == 1]
                    path = nx.shortest_path(tree, ends[0], ends[1])
                    paths.append((path, sum(end_len[m] for v in path for m in members[v])))
                rec['paths_s'] = clock() - t0
            paths.sort(key=lambda p: -p[1])
            t0 = clock()
            index_map = np.full(shape, -1, np.int32)
            new_members = []
            for n, (path, length) in enumerate(paths):
                old = [m for v in path for m in members[v]]
                acc, cut = 0.0, len(old) // 2
                for k, m in enumerate(old):               # the cut nearest to half the length
                    acc += end_len[m]
                    if acc >= length / 2:
                        cut = min(max(k + 1, 1), len(old) - 1)
                        break
                for half, new in ((old[:cut], 2 * n), (old[cut:], 2 * n + 1)):
                    index_map[half] = new
                    new_members.append(half)
            rec['update_host_s'] = clock() - t0
            t0 = clock()
            ni, nj, _nw, over = eng.aggregate(2 * len(paths), index_map)
            rec['aggregate_call_s'] = clock() - t0
            rec['cells_over'] = int(over.size)
            members = new_members
            cur_i, cur_j = ni.astype(np.int64), nj.astype(np.int64)
            pairs = np.arange(2 * len(paths), dtype=np.int32).reshape(-1, 2)[:, ::-1].copy()
            fresh = True
            rec['new_shape'] = 2 * len(paths)
            rec['events_ms'] = {k: _lib.profile_get(k)[0] for k in kernels + COPIES}
            rounds.append(rec)
        stats = eng.stats()
        if forest == 'device':
            stats.update(eng.forest_stats())
        eng.close()
    finally:
        _lib.profile_enable(False)
    total_s = clock() - t_all
    tot = lambda key: round(sum(r.get(key, 0.0) for r in rounds), 6)      # noqa: E731
    events = {k: round(create_events[k] + sum(r['events_ms'][k] for r in rounds), 3) for k in kernels + COPIES}
    for r in rounds:
        for k, v in list(r.items()):
            if isinstance(v, float):
                r[k] = round(v, 6)
        r['events_ms'] = {k: round(v, 3) for k, v in r['events_ms'].items()}
    totals = {'wall_s': round(total_s, 3), 'create_call_s': round(create_s, 6), 'kernels_ms': round(sum(events[k] for k in kernels), 3),
              'copies_ms': round(sum(events[k] for k in COPIES), 3), 'events_ms_by_class': events, 'density_calls_s': tot('density_call_s'),
              'confidence_calls_s': tot('confidence_call_s'), 'aggregate_calls_s': tot('aggregate_call_s'), 'filter_s': tot('filter_s'),
              'forest_s': tot('forest_s'), 'paths_s': tot('paths_s'), 'update_host_s': tot('update_host_s')}
    if forest == 'device':
        totals.update(forest_calls_s=tot('forest_call_s'), tree_ends_s=tot('tree_ends_s'), forest_events_ms=round(sum(events[k] for k in FOREST_KERNELS), 3))
    parts = {k: totals[k] for k in ('density_calls_s', 'confidence_calls_s', 'aggregate_calls_s', 'filter_s', 'forest_s', 'paths_s', 'update_host_s',
                                    'forest_calls_s', 'tree_ends_s') if k in totals}
    totals['largest_part'] = max(parts, key=parts.get)
    return {'what': 'one synthetic group through _lib.SortGraph, round loop of tools/sort_bench.py (profiling on: every call also records HIP events)',
            'box': '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count()), 'contigs': len(case.ctgs), 'shape': shape,
            'links': len(case.links), 'method': 'multiplication', 'cutoff': cutoff, 'rounds': rounds, 'totals': totals, 'counters': stats,
            'note': 'events_ms: HIP-event time of the kernel classes (sort_confidence = top-3 + edges + sisters; sort_emit = row counts, scan, edge list, '
                    'dense matrix) and of the device -> host copy of the 8 * shape^2 byte confidence array; *_call_s: wall time of the whole call from Python, '
                    'allocation, uploads and synchronisation included; forest_s: networkx maximum_spanning_tree(Graph(array)) on the host; update_host_s: '
                    'the map old end -> new end from the paths (stand-in for the name work of update())'}


def reference_run(scripts, case):
    """the reference's unmodified fast_sort on the case, its own functions timed from outside"""
    import types
    S = sc.load_reference_sort(scripts, '_haphic_sort_reference_bench')
    spent, calls = {}, {}

    def timed(name, fn):
        def wrapper(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                spent[name] = spent.get(name, 0.0) + time.perf_counter() - t0
                calls[name] = calls.get(name, 0) + 1
        return wrapper
    inner_d2m = S.dict_to_matrix
    S.dict_to_matrix = lambda d, shape, add_self_loops=False: (inner_d2m(d, shape, True) if add_self_loops
                                                              else timed('dict_to_matrix', inner_d2m)(d, shape))
    for name in ('get_density_graph', 'get_unfiltered_confidence_graph', 'filter_confidence_graph', 'remove_shortest_path', 'update'):
        setattr(S, name, timed(name, getattr(S, name)))
    S.Graph = timed('graph_from_array', S.Graph)          # networkx.Graph(confidence_graph) :570, evaluated before the forest call
    S.nxtree = types.SimpleNamespace(maximum_spanning_tree=timed('forest', S.nxtree.maximum_spanning_tree))
    t0 = time.perf_counter()
    fa_dict, data = sc.group_inputs(S, case)
    prepare_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    S.fast_sort(sc.args_of(case), fa_dict, data, case.name)
    total_s = time.perf_counter() - t0
    return {'what': "HapHiC_sort.fast_sort, unmodified, on a prefix of the same group: the first contigs along the planted chain and the links among them; one core",
            'stored': False, 'box': '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count()), 'contigs': len(case.ctgs),
            'shape': 2 * len(case.ctgs), 'links': len(case.links), 'fast_sort_s': round(total_s, 3), 'get_sub_HT_dict_s (outside fast_sort)': round(prepare_s, 3),
            'seconds_by_function': {k: round(v, 3) for k, v in spent.items()}, 'calls': calls,
            'rest_of_fast_sort_s': round(total_s - sum(spent.values()), 3)}


def forest_bench(sizes, repeats, parent, out):
    """both ways of the forest block on the same groups, interleaved, `repeats` times each (profiling off), then one profiled run of each for the split"""
    res = {'what': 'tools/sort_bench.py --forest-bench: the round loop of this tool on one synthetic chain group per size, whole-loop wall seconds',
           'box': '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count()), 'repeats': repeats, 'sizes': {}}
    device_run(group(200), forest='device')              # warm-up: library, pool, networkx, both forms of the forest
    device_run(group(200))
    for n in sizes:
        case = group(n)
        device_run(case, profile=False, forest='device')                       # every shape of the timed runs
        walls = {'seam_on': [], 'seam_off': []}
        tours = set()
        for _ in range(repeats):
            for name, mode in (('seam_off', 'host'), ('seam_on', 'device')):
                run = device_run(case, profile=False, forest=mode)
                walls[name].append(run['totals']['wall_s'])
                tours.add(tuple((r['shape'], r.get('new_shape')) for r in run['rounds']))
        assert len(tours) == 1, 'the two ways took different rounds'
        rec = {'contigs': n, 'shape': 2 * n}
        for name, w in walls.items():
            rec[name] = {'wall_s': w, 'median_s': sorted(w)[len(w) // 2], 'spread_s': round(max(w) - min(w), 3)}
        if parent and str(n) in parent:
            w = parent[str(n)]
            rec['parent_commit'] = {'wall_s': w, 'median_s': sorted(w)[len(w) // 2], 'spread_s': round(max(w) - min(w), 3)}
        for name, mode in (('seam_off_profiled', 'host'), ('seam_on_profiled', 'device')):
            run = device_run(case, forest=mode)
            rec[name] = {'totals': run['totals'], 'counters': run['counters'],
                         'rounds': [{k: r[k] for k in ('shape', 'edges', 'confidence_call_s', 'filter_s', 'forest_s', 'forest_call_s', 'tree_ends_s', 'paths_s',
                                                      'removed') if k in r} | {'forest_events_ms': round(sum(r['events_ms'].get(k, 0.0) for k in FOREST_KERNELS), 3),
                                                                              'confidence_copy_ms': r['events_ms']['sort_confidence_copy']}
                                    for r in run['rounds']]}
        res['sizes'][str(n)] = rec
        print(json.dumps({k: v for k, v in rec.items() if not k.endswith('_profiled')}), flush=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--forest-bench', action='store_true', help='time the forest block on the host and on the device (profiles/sort_forest_bench.json)')
    ap.add_argument('--sizes', default='3000,10000')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--parent', help='JSON {contigs: [wall seconds]} of the parent commit, measured in the same session')
    ap.add_argument('--contigs', type=int, default=3000)
    ap.add_argument('--prefix', type=int, default=600, help='contigs of the prefix the reference is timed on')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sort_bench.json'))
    ap.add_argument('--reference', default=os.environ.get('HAPHIC_REFERENCE'), help="HapHiC's scripts/ directory: time its fast_sort too")
    ap.add_argument('--reference-only', action='store_true', help='no GPU: the reference record alone (the other records of --out are kept)')
    args = ap.parse_args()
    if args.forest_bench:
        parent = None
        if args.parent:
            with open(args.parent) as f:
                parent = json.load(f)
        out = args.out if args.out != os.path.join(ROOT, 'profiles', 'sort_bench.json') else os.path.join(ROOT, 'profiles', 'sort_forest_bench.json')
        return forest_bench([int(x) for x in args.sizes.split(',')], args.repeats, parent, out)
    res = {}
    for p in (args.out, os.path.join(ROOT, 'profiles', 'sort_bench.json')):
        if os.path.exists(p):
            with open(p) as f:
                res = json.load(f)
            break
    case = group(args.contigs)
    if not args.reference_only:
        device_run(group(200))                           # warm-up: library, pool, networkx
        first = device_run(case)                         # ... and every shape of the timed run
        plain = device_run(case, profile=False)
        res['device'] = device_run(case)
        res['device']['totals']['wall_s_first_run'] = first['totals']['wall_s']
        res['device']['totals']['wall_s_without_events'] = plain['totals']['wall_s']
    if args.reference and os.path.isdir(args.reference):
        res['reference'] = reference_run(args.reference, prefix_of(case, args.prefix))
    elif 'reference' in res:
        res['reference']['stored'] = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({k: (res[k]['totals'] if k == 'device' else res[k]) for k in ('device', 'reference') if k in res}))


if __name__ == '__main__':
    main()
