"""The corpus for the forest block of `haphic sort`'s fast sorting (fast_sort :567-595; haphic_amd/sort.py bind_forest, hhx_sort_graph_forest of
haphic_amd/csrc/hhx_sort.hip): a pure-Python restatement of what the forest call specifies, a host engine with confidence_device / forest /
fetch_confidence on top of tests/sort_cases.py's NumpyEngine, further groups, and the playback over tests/golden/sort_forest.npz (written by
tests/golden/make_golden_sort_forest.py from the reference's own block and networkx).

The fixture has the layout of tests/golden/sort.npz (case / iteration / key) plus, for every iteration whose forest the reference built:
f_cutoff; f_filt_i / f_filt_j / f_filt_v (the filtered confidence graph, upper triangle); f_ref_eu / f_ref_ev (forest.edges() in networkx's order);
f_paths / f_path_off (the reference's paths in its order and direction; absent where it asserted); f_eu / f_ev / f_label / f_pos / f_not_paths (the
canonical answer).  `direct` cases are one round that no fast_sort run reaches (built from edges, equal lengths and sister pairs alone)."""
import os

import numpy as np

from . import sort_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sort_forest.npz')
FOREST_LDS_SHAPE = 2048              # SF_LDS_SHAPE of hhx_sort.hip
LDS_BYTES, LDS_STATIC = 160 * 1024, 4608


def lds_edge_slots(n):
    """the edges the one-workgroup form of hhx_sort_graph_forest holds beside the arrays of n nodes (head of hhx_sort.hip)"""
    cap = 1
    while 12 * 2 * cap + 48 * n + LDS_STATIC <= LDS_BYTES:
        cap *= 2
    return cap


# ------------------------------------------------------------------ restatement
def forest_of_cells(n, u, v, w):
    """The maximum spanning forest of networkx's Kruskal on the graph of the cells (u[k] < v[k], weight w[k] > 0, no pair twice) over nodes 0 .. n - 1
    -> (eu, ev, label, pos, not_paths): edges taken in the order (weight descending, u ascending, v ascending) whenever their ends lie in different
    trees; label = the smallest index of the node's tree; pos = steps from the path's end with the smaller index (-1 everywhere when some node has
    no edge or more than two)."""
    order = np.lexsort((v, u, -np.asarray(w, np.float64)))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    eu, ev, nb = [], [], [[] for _ in range(n)]
    for k in order.tolist():
        a, b = int(u[k]), int(v[k])
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            eu.append(a)
            ev.append(b)
            nb[a].append(b)
            nb[b].append(a)
    label = np.full(n, n, np.int32)
    for x in range(n):
        r = find(x)
        label[r] = min(label[r], x)
    label = label[[find(x) for x in range(n)]]
    not_paths = any(len(x) < 1 or len(x) > 2 for x in nb)
    pos = np.full(n, -1, np.int32)
    if not not_paths:
        ends = [x for x in range(n) if len(nb[x]) == 1]
        other = {}
        for x in ends:                                     # walk every path once, from its smaller end
            if x in other:
                continue
            prev, cur, k = -1, x, 0
            walk = [x]
            while True:
                nxt = [y for y in nb[cur] if y != prev]
                if not nxt:
                    break
                prev, cur = cur, nxt[0]
                walk.append(cur)
            other[x], other[cur] = cur, x
            if cur < x:
                walk.reverse()
            for k, y in enumerate(walk):
                pos[y] = k
    return np.array(eu, np.int32), np.array(ev, np.int32), label.astype(np.int32), pos, bool(not_paths)


class HostForestEngine(sc.NumpyEngine):
    """NumpyEngine plus the three entries bind_forest needs, and the counters of _lib.SortGraph.forest_stats it can know"""
    forest_lds = FOREST_LDS_SHAPE

    def __init__(self, shape, ei, ej, w):
        sc.NumpyEngine.__init__(self, shape, ei, ej, w)
        self._C = None
        self._pairs = None
        self._fstats = dict(lds_forests=0, hbm_forests=0, jump_rounds=0, confidence_copies=0)

    def confidence(self, pair_a, pair_b):
        self._fstats['confidence_copies'] += 1
        return sc.NumpyEngine.confidence(self, pair_a, pair_b)

    def confidence_device(self, pair_a, pair_b):
        self._C, maxs = sc.NumpyEngine.confidence(self, pair_a, pair_b)
        self._pairs = (np.asarray(pair_a, np.int64), np.asarray(pair_b, np.int64))
        return maxs

    def fetch_confidence(self):
        if self._C is None or self._C.shape[0] != self.n:
            raise RuntimeError('SortGraph.fetch_confidence: no confidence graph computed at the current shape')
        self._fstats['confidence_copies'] += 1
        return self._C.copy()

    def forest(self, cutoff):
        if self._C is None or self._C.shape[0] != self.n or cutoff != cutoff:
            raise RuntimeError('SortGraph.forest: no confidence graph computed at the current shape, or no cutoff')
        C, n = self._C, self.n
        live = ~(self.dead[self.ci] | self.dead[self.cj])
        i, j = self.ci[live], self.cj[live]
        low = C[i, j] <= cutoff
        C[i[low], j[low]] = 0
        C[j[low], i[low]] = 0
        a = np.concatenate([i, self._pairs[0]])
        b = np.concatenate([j, self._pairs[1]])
        cell = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
        u, v = cell // n, cell % n
        keep = C[u, v] != 0
        u, v = u[keep], v[keep]
        res = forest_of_cells(n, u, v, C[u, v])
        lds = n <= min(max(self.forest_lds, 0), FOREST_LDS_SHAPE) and u.size <= lds_edge_slots(n)
        self._fstats['lds_forests' if lds else 'hbm_forests'] += 1
        self._fstats['jump_rounds'] = 0 if res[4] else int(np.ceil(np.log2(n)))
        return res

    def forest_stats(self):
        return dict(self._fstats)

    def drop(self, a, b):
        sc.NumpyEngine.drop(self, a, b)
        self._C = None

    def aggregate(self, new_shape, index_map):
        self._C = None
        return sc.NumpyEngine.aggregate(self, new_shape, index_map)


# ------------------------------------------------------------------ further groups
def lone_links_case(name, n, seed, cyclic=False, n_chains=1, cutoff=1.0, weak=(), shuffle=True):
    """n contigs of one length ('sum': every density is the link count over one constant).  The contigs, in a random order and orientation, are cut
    into n_chains runs; neighbours of a run are joined by ONE link of 100 between their facing ends (a link that is alone at both its ends has
    confidence 2: every such edge ties with every other), a cyclic run is closed the same way.  weak: link counts drawn for one further link from the
    facing end of every contig to a random end two runs on — they quantise the confidences (100 / weak) and, above the cutoff, fork the trees."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n) if shuffle else np.arange(n)
    flip = rng.integers(0, 2, n) if shuffle else np.zeros(n, np.int64)
    links = {}
    bounds = np.linspace(0, n, n_chains + 1).astype(int)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        run = order[lo:hi]
        steps = len(run) if cyclic and len(run) > 1 else len(run) - 1
        for p in range(steps):
            x, y = int(run[p]), int(run[(p + 1) % len(run)])
            sc._link(links, x, 'H' if flip[x] else 'T', y, 'T' if flip[y] else 'H', 100)
            if len(weak) and rng.integers(0, 3) == 0:
                z = int(order[rng.integers(0, n)])
                if z not in (x, y):
                    sc._link(links, x, 'H' if flip[x] else 'T', z, 'HT'[rng.integers(0, 2)], int(rng.choice(weak)))
    return sc.Case(name, [(sc._name(k), 500_000) for k in range(n)], links, 'sum', cutoff, 0)


def forest_cases():
    """the groups traced through the reference's fast_sort on top of sort_cases.cases()"""
    out = [lone_links_case('cycle4', 2, 1, cyclic=True, shuffle=False),          # shape 4: both non-sister edges tied, the second is cut
           lone_links_case('cycle_all', 37, 2, cyclic=True),
           lone_links_case('path600', 600, 3)]
    for n in (31, 32, 33, 127, 128, 129, 255, 256, 257):                         # shapes 62 .. 514: chains across the wave and workgroup seams
        out.append(lone_links_case('chain%d' % (2 * n), n, n))
    for k in range(6):
        out.append(lone_links_case('cycles%d' % k, 48 + 5 * k, 100 + k, cyclic=True, n_chains=4 + k))
        out.append(lone_links_case('quant%d' % k, 60 + 7 * k, 200 + k, cyclic=k % 2 == 0, n_chains=3 + k, weak=(10, 20, 25, 50, 100)))
    for k in range(4):
        out.append(lone_links_case('fork%d' % k, 20 + 9 * k, 300 + k, n_chains=2, cutoff=0.5, weak=(60, 75, 90)))
    return out


DIRECT = {
    # shape 4, both links leave c0_T with the same count: confidence 1, filtered at cutoff 1 -> the two sister edges alone, two trees of two nodes
    'direct_sisters_only': dict(shape=4, edges=[(3, 1, 10), (3, 2, 10)], pairs=[(0, 3), (1, 2)], cutoff=1.0),
    # the list edge (0, 3) is a sister pair too: one cell, one edge, at the sister weight
    'direct_twin': dict(shape=6, edges=[(0, 3, 40), (3, 1, 30), (2, 4, 50), (5, 1, 7)], pairs=[(0, 3), (1, 2), (4, 5)], cutoff=1.0),
    # a fourth contig hangs on node 1 and the cutoff is 0.1: every edge stays, node 1 keeps three
    'direct_twin_fork': dict(shape=8, edges=[(0, 3, 40), (3, 1, 30), (2, 4, 50), (6, 1, 7)], pairs=[(0, 3), (1, 2), (4, 5), (6, 7)], cutoff=0.1),
}


def all_case_names():
    return [c.name for c in sc.cases()] + [c.name for c in forest_cases()] + list(DIRECT)


def fast_sort_cases():
    return sc.cases() + forest_cases()


# ------------------------------------------------------------------ fixture and playback
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = sc.Fixture(GOLDEN)
    return _fixture


def forest_rounds(fx, case):
    return [it for it in range(int(fx.get(case, 'n_iter'))) if fx.has(case, 'f_cutoff', it)]


def play_forest(make_engine, fx, case, on_forest):
    """runs an engine through the recorded iterations of a case as sort_cases.play does, with confidence_device in place of confidence; at every
    iteration with a recorded forest: on_forest(it, engine, maxs, engine.forest(cutoff)) -> the engine"""
    eng = None
    shape = int(fx.get(case, 'shape'))
    method = str(fx.get(case, 'method'))
    for it in range(int(fx.get(case, 'n_iter'))):
        if fx.has(case, 'lengths', it):
            if it == 0:
                eng = make_engine(shape, fx.get(case, 'edge_i', it), fx.get(case, 'edge_j', it), fx.get(case, 'edge_w', it).astype(np.int64))
            lengths = fx.get(case, 'lengths', it)
            flagged = eng.density(lengths, method)
            if len(flagged):
                ln = lengths.tolist()
                eng.patch_len(flagged, [np.float32((ln[a] * ln[b]) ** 0.5) for a, b in np.asarray(flagged).tolist()])
        pairs = fx.get(case, 'pairs', it)
        maxs = eng.confidence_device(pairs[:, 0], pairs[:, 1])
        if fx.has(case, 'f_cutoff', it):
            on_forest(it, eng, maxs, eng.forest(float(fx.get(case, 'f_cutoff', it))))
        if int(fx.get(case, 'removed', it)):
            eng.drop(int(pairs[-1, 0]), int(pairs[-1, 1]))
        elif fx.has(case, 'map', it):
            new_shape = int(fx.get(case, 'new_shape', it))
            i, j, _w, over = eng.aggregate(new_shape, fx.get(case, 'map', it))
            if over.size:
                ordinal = np.searchsorted(i.astype(np.int64) * new_shape + j, over)
                eng.patch_cells(over, ordinal, fx.get(case, 'new_w', it)[ordinal])
    return eng


def check_forest(fx, case, it, eng, maxs, got):
    """one forest of an engine against the fixture: MAXS bits, the five results, the filtered array bit for bit"""
    sc.assert_same_bits(np.float64(maxs), fx.get(case, 'maxs', it), (case, it, 'maxs'))
    eu, ev, label, pos, not_paths = got
    assert bool(not_paths) == bool(fx.get(case, 'f_not_paths', it)), (case, it, 'not_paths')
    for name, arr in (('f_eu', eu), ('f_ev', ev), ('f_label', label), ('f_pos', pos)):
        want = fx.get(case, name, it)
        assert arr.dtype == np.int32 and np.array_equal(arr, want), (case, it, name, arr[:8], want[:8])
    C = eng.fetch_confidence()
    assert C.dtype == np.float64 and C.shape == (eng.shape, eng.shape) and np.array_equal(C, C.T), (case, it, 'filtered shape')
    ci, cj = np.nonzero(np.triu(C, 1))
    assert np.array_equal(ci, fx.get(case, 'f_filt_i', it)) and np.array_equal(cj, fx.get(case, 'f_filt_j', it)), (case, it, 'filtered pattern')
    sc.assert_same_bits(C[ci, cj], fx.get(case, 'f_filt_v', it), (case, it, 'filtered values'))
