"""The corpus for `haphic sort`'s fast sorting (haphic_amd/sort.py, haphic_amd/csrc/hhx_sort.hip), a plain numpy restatement of the three kernels'
specifications with the interface of _lib.SortGraph (the host engine: the analogue of tests/oracle_lib.py), and the playback that runs an engine
through the recorded rounds of tests/golden/sort.npz (written by tests/golden/make_golden_sort.py from the reference's own fast_sort).

A case is a group: contigs (name, length), HT_link_dict entries {(ctg_1 + '_H'|'_T', ctg_2 + '_H'|'_T'): links} with ctg_1 < ctg_2 as the
reference's get_sub_HT_dict :117-143 looks them up, and the three arguments fast_sort reads."""
import argparse
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sort.npz')
LDS_SHAPE = 192                      # SG_LDS_SHAPE of hhx_sort.hip: the seam between the LDS and the global re-aggregation
EXACT = 1 << 24                      # float32 sums of non-negative integers are exact up to here

Case = namedtuple('Case', 'name ctgs links method cutoff flank')


# ------------------------------------------------------------------ numpy engine
class NumpyEngine:
    """_lib.SortGraph restated with numpy: what every entry of include/haphic_hip.h's hhx_sort_graph_* section specifies, nothing about how."""
    METHODS = {'sum': 0, 'multiplication': 1, 'geometric_mean': 2}
    lds_shape = LDS_SHAPE

    def __init__(self, shape, ei, ej, w):
        ei, ej, w = np.asarray(ei, np.int64), np.asarray(ej, np.int64), np.asarray(w, np.int64)
        if shape < 4 or shape % 2 or ei.size == 0:
            raise RuntimeError('SortGraph: shape {} / {} edges'.format(shape, ei.size))
        assert ei.min() >= 0 and ej.min() >= 0 and max(ei.max(), ej.max()) < shape and (ei != ej).all() and w.min() >= 0
        self.shape0 = self.n = shape
        self.ea, self.eb, self.ew = ei, ej, w
        self.S = np.zeros((shape, shape), np.float32)
        self.S[ei, ej] = w.astype(np.float32)
        self.S[ej, ei] = w.astype(np.float32)
        self.D = None
        self.ci, self.cj, self.cw = ei, ej, None
        self.dead = np.zeros(shape, bool)
        self._stats = dict(lds_aggregations=0, global_aggregations=0, cells_over=0, pairs_flagged=0)

    @property
    def shape(self):
        return self.n

    def density(self, lengths, method):
        a = np.asarray(lengths, np.float64)
        assert a.size == self.n == self.S.shape[0] and (a > 0).all()
        method = self.METHODS.get(method, method)
        flagged = np.empty((0, 2), np.int32)
        if method == 0:
            L = a[:, None] + a[None, :]
        elif method == 1:
            L = a[:, None] * a[None, :]
        else:
            L = np.sqrt(a[:, None] * a[None, :])
            low = (L.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64) - 0x10000000
            flagged = np.argwhere(np.triu(np.abs(low) <= 2, 1)).astype(np.int32)
        L = L.astype(np.float32)
        np.fill_diagonal(L, 1)
        self.D = self.S / L
        self._stats['pairs_flagged'] = len(flagged)
        return flagged

    def patch_len(self, pairs, L):
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        i, j = pairs[:, 0], pairs[:, 1]
        L = np.asarray(L, np.float32)
        self.D[i, j] = self.S[i, j] / L
        self.D[j, i] = self.S[j, i] / L

    def confidence(self, pair_a, pair_b):
        n = self.n
        D = self.D[:n, :n]
        top = np.sort(D, axis=1)[:, ::-1][:, :3]
        live = ~(self.dead[self.ci] | self.dead[self.cj])
        i, j = self.ci[live], self.cj[live]
        d = D[i, j]
        a0, a1, a2 = top[i, 0], top[i, 1], top[i, 2]
        x0 = np.where(d == a0, a1, a0)
        x1 = np.where((d == a0) | (d == a1), a2, a1)
        b0, b1 = top[j, 0], top[j, 1]
        second = np.where(x0 >= b0, np.maximum(x1, b0), np.maximum(x0, b1))
        with np.errstate(divide='ignore', invalid='ignore'):
            conf = np.where(d == 0, np.float32(0), np.where(second == 0, np.float32(2), d / second)).astype(np.float32)
        C = np.zeros((n, n), np.float64)
        C[i, j] = conf
        C[j, i] = conf
        maxs = np.float64(conf.max()) if conf.size else np.float64(0)
        sister = 2 * maxs if maxs > 1 else 2
        pa, pb = np.asarray(pair_a, np.int64), np.asarray(pair_b, np.int64)
        C[pa, pb] = sister
        C[pb, pa] = sister
        return C, maxs

    def drop(self, a, b):
        if self.n < 6 or {a, b} != {self.n - 1, self.n - 2}:
            raise RuntimeError('SortGraph.drop: ({}, {}) at shape {}'.format(a, b, self.n))
        self.dead[[a, b]] = True
        self.n -= 2

    def aggregate(self, new_shape, index_map):
        m = np.asarray(index_map, np.int64)
        ns = int(new_shape)
        assert m.size == self.shape0 and m.min() >= -1 and m.max() < ns and ns >= 2 and ns % 2 == 0
        i, j = m[self.ea], m[self.eb]
        ok = (i >= 0) & (j >= 0) & (i != j) & ((i ^ 1) != j)
        acc = np.zeros(ns * ns, np.int64)
        np.add.at(acc, np.maximum(i, j)[ok] * ns + np.minimum(i, j)[ok], self.ew[ok])
        cells = np.nonzero(acc)[0]                        # ascending = row-major over (i_1, i_2), i_1 > i_2
        self.ci, self.cj, self.cw = cells // ns, cells % ns, acc[cells].astype(np.float32)
        self.S = np.zeros((ns, ns), np.float32)
        self.S[self.ci, self.cj] = self.cw
        self.S[self.cj, self.ci] = self.cw
        self.D = None
        self.n = ns
        self.dead = np.zeros(self.shape0, bool)
        over = cells[acc[cells] > EXACT]
        lds = ns <= min(max(self.lds_shape, 0), LDS_SHAPE) and int(self.ew.sum()) < 1 << 32
        self._stats['lds_aggregations' if lds else 'global_aggregations'] += 1
        self._stats['cells_over'] = int(over.size)
        return self.ci.astype(np.int32), self.cj.astype(np.int32), self.cw.copy(), over

    def patch_cells(self, cells, ordinal, values):
        cells, values = np.asarray(cells, np.int64), np.asarray(values, np.float32)
        r, c = cells // self.n, cells % self.n
        self.S[r, c] = values
        self.S[c, r] = values
        self.cw[np.asarray(ordinal, np.int64)] = values

    def matrix(self):
        return self.S[:self.n, :self.n].copy()

    def density_graph(self):
        return self.D[:self.n, :self.n].copy()

    def stats(self):
        return dict(self._stats)

    def close(self):
        pass


# ------------------------------------------------------------------ corpus
def _name(k):
    return 'c%04d' % k


def _link(links, x, xe, y, ye, w):
    """links between end xe ('H' | 'T') of contig number x and end ye of contig y, keyed as get_sub_HT_dict :126-131 looks them up"""
    if x == y:
        return
    (x, xe), (y, ye) = sorted([(_name(x), xe), (_name(y), ye)])
    links[(x + '_' + xe, y + '_' + ye)] = links.get((x + '_' + xe, y + '_' + ye), 0) + int(w)


def chain_case(name, n, seed, method='multiplication', cutoff=1.0, flank=0, isolated=0, strong=(40, 400), noise=2.0, lengths=(100_000, 2_000_000)):
    """n contigs planted as a chain in a random order and orientation: strong links between the facing ends of neighbours, weaker ones two and
    three steps away, a sprinkle of noise; the last `isolated` contigs (the shortest) carry no link at all"""
    rng = np.random.default_rng(seed)
    ln = np.sort(rng.integers(lengths[0], lengths[1], n))[::-1]
    linked = n - isolated
    order = rng.permutation(linked)
    flip = rng.integers(0, 2, linked)
    links = {}
    tail = lambda k: 'H' if flip[k] else 'T'             # noqa: E731  (the end that faces the next contig of the chain)
    head = lambda k: 'T' if flip[k] else 'H'             # noqa: E731
    for p in range(linked - 1):
        x, y = int(order[p]), int(order[p + 1])
        _link(links, x, tail(x), y, head(y), rng.integers(strong[0], strong[1]))
        for step, top in ((2, strong[0]), (3, max(strong[0] // 4, 2))):
            if p + step < linked:
                z = int(order[p + step])
                _link(links, x, tail(x), z, head(z), rng.integers(1, top))
    for _ in range(int(noise * linked)):
        x, y = (int(v) for v in rng.integers(0, linked, 2))
        _link(links, x, 'HT'[rng.integers(0, 2)], y, 'HT'[rng.integers(0, 2)], rng.integers(1, 6))
    return Case(name, [(_name(k), int(ln[k])) for k in range(n)], links, method, cutoff, flank)


def pairs_case(name, n_pairs, seed):
    """2 * n_pairs contigs of one length; pair k = (2k, 2k + 1) is joined by one strong link and a weak one leads on to pair k + 1 from the same
    two ends: round 1 links exactly the pairs (the strong link's only rivals are weak: confidence 10; the weak ones stay below 1), so the
    re-aggregation after round 1 has the shape 2 * n_pairs — the way to place a shape on either side of the LDS / global seam"""
    rng = np.random.default_rng(seed)
    links = {}
    for k in range(n_pairs):
        _link(links, 2 * k, 'T', 2 * k + 1, 'H', 100 + int(rng.integers(0, 50)))
        if k + 1 < n_pairs:
            _link(links, 2 * k + 1, 'H', 2 * k + 2, 'T', 10)
    return Case(name, [(_name(k), 500_000) for k in range(2 * n_pairs)], links, 'sum', 1.0, 0)


def ties_case():
    """equal lengths, 'sum': rows whose largest density occurs twice (end c0_T: 50, 50) and three times (end c3_H: 70, 70, 70) -> confidence exactly 1
    for those edges, which only holds if equal values count as often as they occur; c8 has no link at all (an all-zero row; confidence 2 is
    reached by c6_T - c7_H, whose ends see nothing else)"""
    links = {}
    _link(links, 0, 'T', 1, 'H', 50)
    _link(links, 0, 'T', 2, 'H', 50)
    _link(links, 1, 'T', 2, 'T', 20)
    for y in (4, 5, 6):
        _link(links, 3, 'H', y, 'H', 70)
    _link(links, 4, 'T', 5, 'T', 30)
    _link(links, 6, 'T', 7, 'H', 90)
    _link(links, 3, 'T', 0, 'H', 60)
    _link(links, 3, 'T', 1, 'T', 12)
    return Case('ties', [(_name(k), 400_000) for k in range(9)], links, 'sum', 1.0, 0)


def overflow_case():
    """weights near 2^22: round 1 (cutoff 1.5) joins the pairs (2k, 2k + 1) through one link of 2^26 that dwarfs its rivals; the four links between
    the ends of contig 2k + 1 and those of contig 2k + 2, each about 1.5 * 2^22 and alike (confidence about 1, below the cutoff), land in ONE cell
    of round 2 whose sum passes 2^24 with an odd total — where the float32 running sum of the reference rounds"""
    links = {}
    n = 8
    for k in range(0, n, 2):
        _link(links, k, 'T', k + 1, 'H', 1 << 26)
    for k in range(1, n - 1, 2):
        for e, (xe, ye) in enumerate((('T', 'H'), ('T', 'T'), ('H', 'H'), ('H', 'T'))):
            _link(links, k, xe, k + 1, ye, (1 << 22) + (1 << 21) + (1, 1, 1, 3)[e] + 8 * k)     # offsets chosen so that rounding twice shows
    return Case('overflow', [(_name(k), 1_000_000 - 1000 * k) for k in range(n)], links, 'sum', 1.5, 0)


def removal_case():
    """takes the removal branch of fast_sort :549-558 twice in a row, then proceeds: found by a seeded search over small random groups
    (tests/golden/make_golden_sort.py --search-removal) and written out here as data"""
    links = {}
    for (x, xe, y, ye, w) in REMOVAL_LINKS:
        _link(links, x, xe, y, ye, w)
    return Case('removal', [(_name(k), ln) for k, ln in enumerate(REMOVAL_LENGTHS)], links, 'sum', 1.0, 0)


REMOVAL_LENGTHS = (1500000, 1300000, 1200000, 1100000, 1000000, 900000, 700000, 400000)
REMOVAL_LINKS = ((5, 'T', 3, 'H', 10), (2, 'H', 3, 'H', 30), (4, 'H', 1, 'H', 30), (6, 'T', 5, 'H', 20), (3, 'T', 2, 'H', 30), (1, 'H', 3, 'H', 20),
                 (5, 'T', 2, 'H', 20), (5, 'H', 3, 'T', 20), (0, 'H', 6, 'H', 20), (0, 'T', 6, 'H', 10), (5, 'T', 6, 'H', 30), (1, 'H', 4, 'T', 10),
                 (3, 'H', 5, 'T', 10), (5, 'H', 4, 'H', 10), (4, 'T', 2, 'T', 10), (7, 'H', 5, 'T', 10))


def cases():
    out = [
        chain_case('n2', 2, 2), chain_case('n3', 3, 3, method='sum'), chain_case('n4', 4, 4, method='geometric_mean'),
        chain_case('n32', 32, 32), chain_case('n33', 33, 33, method='sum', cutoff=1.5),
        chain_case('n128', 128, 128, method='geometric_mean'), chain_case('n129', 129, 129), chain_case('n130', 130, 130, method='sum', flank=600),
        pairs_case('seam_lds', LDS_SHAPE // 2, 7), pairs_case('seam_global', LDS_SHAPE // 2 + 1, 8),
        chain_case('chain160', 160, 160, flank=800, strong=(60, 120), noise=3.0),
        chain_case('isolated', 12, 12, isolated=1),
        chain_case('flank_geo', 40, 41, method='geometric_mean', cutoff=1.5, flank=500),
        ties_case(), overflow_case(),
    ]
    if REMOVAL_LENGTHS:
        out.append(removal_case())
    return out


def args_of(case):
    return argparse.Namespace(density_cal_method=case.method, confidence_cutoff=case.cutoff, flanking_region=case.flank)


def group_inputs(S, case):
    """(fa_dict, group_specific_data) as run() :912-920 builds them, with the reference's own parse_group order and get_sub_HT_dict"""
    info = sorted(case.ctgs, key=lambda x: x[1], reverse=True)
    ctgs = [c for c, _ in info]
    sub_HT_dict, HT_index_dict = S.get_sub_HT_dict(ctgs, case.links)
    return dict(case.ctgs), (info, ctgs, sub_HT_dict, HT_index_dict)


# ------------------------------------------------------------------ fixture and playback
class Fixture:
    def __init__(self, path=GOLDEN):
        with np.load(path, allow_pickle=False) as z:     # read once: an NpzFile inflates a member again on every access
            self.z = {k: z[k] for k in z.files}
        self.names = [str(s) for s in self.z['cases']]

    def get(self, case, key, it=None):
        return self.z['{}/{}'.format(case, key) if it is None else '{}/{}/{}'.format(case, it, key)]

    def has(self, case, key, it):
        return '{}/{}/{}'.format(case, it, key) in self.z


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


def play(make_engine, fx, case, reference_engine=None):
    """runs one engine through every recorded iteration of a case, chained (the edges one re-aggregation returns are what the next iteration's
    matrix is made of), and holds each array to the fixture bit for bit.  -> (engine, cells above 2^24 per re-aggregation)"""
    eng = None
    over_counts = []
    shape = int(fx.get(case, 'shape'))
    method = str(fx.get(case, 'method'))
    for it in range(int(fx.get(case, 'n_iter'))):
        if fx.has(case, 'lengths', it):
            ei, ej, w = fx.get(case, 'edge_i', it), fx.get(case, 'edge_j', it), fx.get(case, 'edge_w', it)
            if it == 0:
                eng = make_engine(shape, ei, ej, w.astype(np.int64))
            n = eng.shape
            dense = np.zeros((n, n), np.float32)
            dense[ei, ej] = w.astype(np.float32)
            dense[ej, ei] = w.astype(np.float32)
            assert_same_bits(eng.matrix(), dense, (case, it, 'matrix'))
            lengths = fx.get(case, 'lengths', it)
            flagged = eng.density(lengths, method)
            if len(flagged):
                ln = lengths.tolist()
                eng.patch_len(flagged, [np.float32((ln[a] * ln[b]) ** 0.5) for a, b in np.asarray(flagged).tolist()])
            D = eng.density_graph()
            assert_same_bits(D[ei, ej], fx.get(case, 'density', it), (case, it, 'density'))
            assert_same_bits(D[ej, ei], fx.get(case, 'density', it), (case, it, 'density, transposed'))
            assert np.count_nonzero(D) == 2 * np.count_nonzero(fx.get(case, 'density', it)), (case, it, 'density outside the edges')
        pairs = fx.get(case, 'pairs', it)
        C, maxs = eng.confidence(pairs[:, 0], pairs[:, 1])
        assert type(maxs) is np.float64 and C.dtype == np.float64 and C.shape == (eng.shape, eng.shape), (case, it)
        assert_same_bits(np.float64(maxs), fx.get(case, 'maxs', it), (case, it, 'maxs'))
        assert np.array_equal(C, C.T), (case, it, 'confidence symmetry')
        ci, cj = np.nonzero(np.triu(C, 1))
        assert np.array_equal(ci, fx.get(case, 'conf_i', it)) and np.array_equal(cj, fx.get(case, 'conf_j', it)), (case, it, 'confidence pattern')
        assert_same_bits(C[ci, cj], fx.get(case, 'conf_v', it), (case, it, 'confidence'))
        if int(fx.get(case, 'removed', it)):
            eng.drop(int(pairs[-1, 0]), int(pairs[-1, 1]))
        elif fx.has(case, 'map', it):
            new_shape = int(fx.get(case, 'new_shape', it))
            i, j, w, over = eng.aggregate(new_shape, fx.get(case, 'map', it))
            want_i, want_j, want_w = fx.get(case, 'new_i', it), fx.get(case, 'new_j', it), fx.get(case, 'new_w', it)
            assert np.array_equal(i, want_i) and np.array_equal(j, want_j), (case, it, 'aggregated keys')
            assert w.dtype == np.float32
            ordinal = np.searchsorted(i.astype(np.int64) * new_shape + j, over)
            exact = np.ones(w.size, bool)
            exact[ordinal] = False
            assert_same_bits(w[exact], want_w[exact], (case, it, 'aggregated values'))
            if over.size:                                  # the host's part (summing in the reference's order) is pinned by the fast_sort comparison
                eng.patch_cells(over, ordinal, want_w[ordinal])
            over_counts.append(int(over.size))
            assert eng.stats()['cells_over'] == over.size
    return eng, over_counts


# ------------------------------------------------------------------ the reference module and a traced run of its fast_sort
REFERENCE_SCRIPTS = '/root/reference/scripts'


def load_reference_sort(scripts=REFERENCE_SCRIPTS, name='_haphic_sort_reference_private'):
    """HapHiC_sort.py under a private module name: every caller patches (or leaves alone) its own copy"""
    import importlib.util
    import sys
    import types
    for mod, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        try:                                             # HapHiC_sort imports HapHiC_build -> HapHiC_cluster, which imports both; fast sorting uses neither
            __import__(mod)
        except ImportError:
            m = types.ModuleType(mod)
            m.__dict__.update(attrs)
            sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, 'HapHiC_sort.py'))
    module = importlib.util.module_from_spec(spec)
    sys.path.insert(0, scripts)
    try:
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(scripts)
    return module


def run_fast_sort(S, case, log=None):
    """the module's fast_sort on a case -> (output_path_list, the bytes of the .tour file, the debug log lines)"""
    import io
    import logging
    import tempfile
    fa_dict, data = group_inputs(S, case)
    stream = io.StringIO()
    handler = logging.StreamHandler(stream)
    handler.setFormatter(logging.Formatter('%(message)s'))
    level = S.logger.level
    S.logger.addHandler(handler)
    S.logger.setLevel(logging.DEBUG)
    S.logger.propagate = False
    try:
        paths, _one = S.fast_sort(args_of(case), fa_dict, data, case.name)
    finally:
        S.logger.removeHandler(handler)
        S.logger.setLevel(level)
    with tempfile.TemporaryDirectory() as tmp:
        S.output_tour_file(paths, os.path.join(tmp, case.name))
        with open(os.path.join(tmp, case.name + '.tour'), 'rb') as f:
            tour = f.read()
    return paths, tour, stream.getvalue().splitlines()
