"""`haphic sort` (scripts/HapHiC_sort.py), fast sorting on the MI355X library: the dense work of fast_sort :470-615 per group and round.

fast_sort itself, split_new_scaffold, output_tour_file, the ALLHiC optimisation and run() stay the reference's code, and so does the spanning
forest :570-595 unless bind_forest is asked for;
the functions below replace the module globals fast_sort resolves at call time (patch.patch_sort):

    dict_to_matrix :60-88                     round 1: the dict's edges go to the device once (_lib.SortGraph), later rounds: the handle again
    get_density_graph :158-192                lengths per index on the host (float64), length matrix and division on the device
    get_unfiltered_confidence_graph :195-244  per-row top-3 + one thread per edge; one copy of the float64 array networkx reads
    filter_confidence_graph :247-255          vectorised over the edge arrays
    remove_shortest_path :456-467             the last pair popped, its edges dropped, the matrices cut as a view on the device
    update :338-437                           the work on names here, the link re-aggregation as a scatter-add on the device

What the device path does not cover (weights that are not non-negative integers, an empty dict, a shape below 4) is decided once, in round 1:
dict_to_matrix then returns the reference's numpy matrix and every seam hands such a group to the original functions.  The new sub_HT_dict is a
SubHT: a defaultdict that stays arrays until something other than these seams touches it (the pattern of containers.py).

bind_verdict: compare_fast_sort_and_allhic :645-724, which run_haphic_sorting :748 calls per group once fast sorting and ALLHiC have both run.  The
weighted-LIS sums of the rotations :696-721 come from one library call (_lib.sort_verdict_sums); parse_tours, the ratio rule :683-688, the threshold
:712-716 and both log lines stay here, in Python ints and floats.

bind_heads: the front of run() :898-923.  S.pickle becomes a PickleProxy whose load() reads HT_links.pkl into arrays on the device (HTTable) and
get_sub_HT_dict :117-143 extracts each group from them there (HeadsHT, which round 1 of dict_to_matrix takes as arrays).

bind_forest (opt-in): the forest block :567-595.  The confidence array stays on the device (a ConfidenceToken stands for it), one library call
filters it and builds the maximum spanning forest with every node's tree and position along its path (_lib.SortGraph.forest); the host builds the
networkx graph of the chosen edges, asks networkx itself for components, ends and their order, and reads each path off the positions.  Handed back to
the reference's block on the fetched array: a forest that is no set of paths (the reference asserts), an engine without forest(), a group in
host_mode or whose sub_HT_dict is no longer the device's edge list, a token thawed by foreign code, a shape above 65535, a maximum_spanning_tree
call that is not (token, algorithm='kruskal')."""
import threading
from itertools import product

import numpy as np

from . import containers

METHODS = ('sum', 'multiplication', 'geometric_mean')
DEVICE_LOCK = threading.Lock()        # one group on the device at a time; the other threads of run()'s pool are in their ALLHiC child meanwhile
_tls = threading.local()              # .graph: the Graph of the group this thread's fast_sort is working on


DEVICE = None                         # the HIP device of `--device N`: HIP's current device is per thread, and run()'s pool threads start on device 0


def _default_engine(shape, ei, ej, w):
    from . import _lib
    if DEVICE is not None:
        _lib.set_device(DEVICE)
    return _lib.SortGraph(shape, ei, ej, w)


class Graph:
    """What dict_to_matrix / get_density_graph / remove_shortest_path hand to fast_sort in place of a numpy matrix: the device handle of the group
    plus the round-1 edges as host arrays (filter_confidence_graph and the cells update() has to sum in the reference's order need them)."""

    def __init__(self, engine, shape, source, ei, ej, w):
        self.engine = engine
        self.shape0 = shape
        self.source = source                              # the round-1 dict itself: recognised by identity
        self.ei, self.ej, self.w = ei, ej, w
        self.alive = np.ones(ei.size, bool)               # remove_shortest_path in round 1
        self.host_mode = False                            # a SubHT was thawed by foreign code: the rest of the group runs the reference's functions
        self._lookup = None
        self.thaws = 0
        self.forest_rounds = 0                            # bind_forest: rounds whose forest came from the device ...
        self.forest_thaws = 0                             # ... and confidence arrays fetched for the reference's own block

    def note_thawed(self):
        self.thaws += 1

    def links(self, a, b):
        """old_sub_HT_matrix[a, b] (:432) as numpy.float32"""
        if self._lookup is None:
            vals = self.w.astype(np.float32)
            self._lookup = dict(zip(zip(np.minimum(self.ei, self.ej).tolist(), np.maximum(self.ei, self.ej).tolist()), list(vals)))
        return self._lookup.get((a, b) if a < b else (b, a), np.float32(0))

    def dense_round1(self):
        m = np.zeros((self.shape0, self.shape0), np.float32)
        m[self.ei, self.ej] = self.w
        m[self.ej, self.ei] = self.w
        return m

    def close(self):
        close = getattr(self.engine, 'close', None)
        if close is not None:
            close()


class SubHT(containers._Frozen):
    """The sub_HT_dict update() returns: {(i_1, i_2): numpy.float32}, i_1 > i_2, row-major — as three arrays until it is touched."""

    def __init__(self, graph, i, j, w):
        containers._Frozen.__init__(self, int, graph, 'sub_HT')
        self.i, self.j, self.w = i, j, w

    def _n(self):
        return int(self.i.size)

    def _source_items(self):
        return zip(zip(self.i.tolist(), self.j.tolist()), list(self.w))

    def drop_touching(self, a, b):
        keep = ~((self.i == a) | (self.i == b) | (self.j == a) | (self.j == b))
        self.i, self.j, self.w = self.i[keep], self.j[keep], self.w[keep]


def _frozen(d):
    return isinstance(d, SubHT) and d.frozen


def _round1_arrays(dict_, shape):
    """(i, j, w) of a dict the device path covers, else None"""
    n = len(dict_)
    if n == 0 or shape < 4 or shape % 2:
        return None
    try:
        keys = np.array(list(dict_.keys()))
        vals = np.array(list(dict_.values()))
    except (ValueError, TypeError, OverflowError):
        return None
    if keys.shape != (n, 2) or keys.dtype.kind not in 'iu' or vals.shape != (n,) or vals.dtype.kind not in 'iu':
        return None
    i, j = keys[:, 0].astype(np.int64), keys[:, 1].astype(np.int64)
    if i.min() < 0 or j.min() < 0 or i.max() >= shape or j.max() >= shape or (i == j).any() or vals.min() < 0 or int(vals.max()) > 2 ** 53:
        return None
    if np.unique(np.maximum(i, j) * shape + np.minimum(i, j)).size != n:       # (a, b) and (b, a): coo_matrix would add them up
        return None
    return i.astype(np.int32), j.astype(np.int32), vals.astype(np.int64)


def bind(S, engine=None):
    """The mirrors for the imported HapHiC_sort module S -> {name: function}.  engine(shape, ei, ej, w): the SortGraph factory (the device by default)."""
    make_engine = engine or _default_engine
    original = {name: getattr(S, name) for name in ('dict_to_matrix', 'get_density_graph', 'get_unfiltered_confidence_graph', 'filter_confidence_graph',
                                                    'remove_shortest_path', 'update', 'fast_sort')}

    def dict_to_matrix(dict_, shape, add_self_loops=False):
        g = getattr(_tls, 'graph', None)
        if add_self_loops:                                 # the length matrix inside the reference's own get_density_graph
            return original['dict_to_matrix'](dict_, shape, add_self_loops)
        if g is not None and _frozen(dict_) and dict_._session is g and not g.host_mode:
            return g                                       # the link matrix is already on the device (update)
        if g is None and not isinstance(dict_, SubHT):
            arrays = dict_.round1_arrays(shape) if _frozen_heads(dict_) else _round1_arrays(dict_, shape)     # None: the reference's path (a HeadsHT thaws)
            if arrays is not None:
                g = Graph(make_engine(shape, *arrays), shape, dict_, *arrays)
                _tls.graph = g
                return g
            _tls.graph = False                             # decided once: this group is the reference's
        elif g:
            g.host_mode = True
        return original['dict_to_matrix'](dict_, shape)

    def get_density_graph(sub_HT_matrix, shape, index_HT_dict, fa_dict, flank_HT_dict, density_cal_method):
        if not isinstance(sub_HT_matrix, Graph):
            return original['get_density_graph'](sub_HT_matrix, shape, index_HT_dict, fa_dict, flank_HT_dict, density_cal_method)
        g = sub_HT_matrix
        lengths = []
        for k in range(shape):
            HT = index_HT_dict[k]
            lengths.append(flank_HT_dict[HT][1] if HT in flank_HT_dict else S.get_len(HT, fa_dict))
        flagged = g.engine.density(lengths, density_cal_method)
        if len(flagged):                                   # geometric_mean: Python's ** decides the pairs next to a float32 rounding boundary
            g.engine.patch_len(flagged, [np.float32((lengths[a] * lengths[b]) ** 0.5) for a, b in flagged.tolist()])
        return g

    def get_unfiltered_confidence_graph(shape, index_pairs, sub_HT_dict, density_graph):
        if not isinstance(density_graph, Graph):
            return original['get_unfiltered_confidence_graph'](shape, index_pairs, sub_HT_dict, density_graph)
        pairs = np.array(index_pairs, np.int32).reshape(-1, 2)
        confidence_graph, maxs = density_graph.engine.confidence(pairs[:, 0], pairs[:, 1])
        assert confidence_graph.shape == (shape, shape)
        return confidence_graph, maxs

    def _edges_of(sub_HT_dict):
        g = getattr(_tls, 'graph', None)
        if _frozen(sub_HT_dict):
            return sub_HT_dict.i, sub_HT_dict.j
        if g and sub_HT_dict is g.source and not g.host_mode:
            return g.ei[g.alive], g.ej[g.alive]
        return None

    def filter_confidence_graph(confidence_graph, sub_HT_dict, confidence_cutoff):
        edges = _edges_of(sub_HT_dict)
        if edges is None:
            return original['filter_confidence_graph'](confidence_graph, sub_HT_dict, confidence_cutoff)
        i, j = edges
        low = confidence_graph[i, j] <= confidence_cutoff
        confidence_graph[i[low], j[low]] = 0
        confidence_graph[j[low], i[low]] = 0

    def remove_shortest_path(index_pairs, sub_HT_dict, density_graph):
        if not isinstance(density_graph, Graph):
            return original['remove_shortest_path'](index_pairs, sub_HT_dict, density_graph)
        g = density_graph
        a, b = index_pairs.pop(-1)
        if _frozen(sub_HT_dict) or _frozen_heads(sub_HT_dict):
            sub_HT_dict.drop_touching(a, b)
        else:
            for key in [key for key in sub_HT_dict if a in key or b in key]:
                sub_HT_dict.pop(key)
        if sub_HT_dict is g.source:                        # either branch: a frozen HeadsHT of round 1 is g.source too (a SubHT never is)
            g.alive &= ~((g.ei == a) | (g.ei == b) | (g.ej == a) | (g.ej == b))
        g.engine.drop(a, b)                                # the last two rows and columns leave the view; no copy
        return g

    def update(path_list, old_sub_HT_matrix, index_HT_dict, HT_index_dict, flank_HT_dict, fa_dict, known_adjacency, flank):
        if not isinstance(old_sub_HT_matrix, Graph):
            return original['update'](path_list, old_sub_HT_matrix, index_HT_dict, HT_index_dict, flank_HT_dict, fa_dict, known_adjacency, flank)
        g = old_sub_HT_matrix
        if g.host_mode:
            return original['update'](path_list, g.dense_round1(), index_HT_dict, HT_index_dict, flank_HT_dict, fa_dict, known_adjacency, flank)

        def trim(half, order):
            """the part of a scaffold half within `flank` of the junction-far end (get_flank_HT :347-363)"""
            rest = S.get_len(half, fa_dict)
            if rest <= flank:
                return
            m = 0
            for m, HT in enumerate(half[::order]):
                length = S.get_len(HT, fa_dict)
                if rest - length > flank:
                    rest -= length
                else:
                    break
            kept = half if m == 0 else (half[:-m] if order == 1 else half[m:])
            flank_HT_dict[half] = (kept, S.get_len(kept, fa_dict))

        index_pairs, new_index_HT_dict, output_path_list = [], {}, []
        for n, path in enumerate(path_list):
            lo, hi = 2 * n, 2 * n + 1
            index_pairs.append((hi, lo))
            if len(path) == 2:                             # a contig, or a scaffold of an earlier round
                left, right = index_HT_dict[path[0]], index_HT_dict[path[1]]
                output_path_list.append(list(S.format_HTs(left)) + list(S.format_HTs(right)))
            else:                                          # linked in this round: two halves of about the same length
                left, right = S.split_new_scaffold(path, fa_dict, index_HT_dict, known_adjacency)
                output_path_list.append(list(left) + list(right))
                if flank:
                    trim(left, -1)
                    trim(right, 1)
            new_index_HT_dict[lo], new_index_HT_dict[hi] = left, right

        def ends_of(k):
            HT = new_index_HT_dict[k]
            return S.format_HTs(flank_HT_dict[HT][0] if HT in flank_HT_dict else HT)

        new_shape = 2 * len(path_list)
        index_map = np.full(g.shape0, -1, np.int32)
        for k in range(new_shape):
            for ht in ends_of(k):
                index_map[HT_index_dict[ht]] = k
        i, j, w, over = g.engine.aggregate(new_shape, index_map)
        if over.size:                                      # sums past 2^24: numpy.float32 by numpy.float32 in the order of product(HT_1, HT_2) :427-435
            ordinal = np.searchsorted(i.astype(np.int64) * new_shape + j, over)
            values = np.empty(over.size, np.float32)
            for k, cell in enumerate(over.tolist()):
                total = 0
                for ht_1, ht_2 in product(ends_of(cell // new_shape), ends_of(cell % new_shape)):
                    links = g.links(HT_index_dict[ht_1], HT_index_dict[ht_2])
                    if links:
                        total += links
                values[k] = total
            w[ordinal] = values
            g.engine.patch_cells(over, ordinal, values)
        return new_index_HT_dict, SubHT(g, i, j, w), index_pairs, output_path_list

    def fast_sort(args, fa_dict, group_specific_data, prefix):
        with DEVICE_LOCK:
            _tls.graph = None
            try:
                return original['fast_sort'](args, fa_dict, group_specific_data, prefix)
            finally:
                g = getattr(_tls, 'graph', None)
                _tls.graph = None
                if g:
                    g.close()
    fast_sort.__wrapped__ = original['fast_sort']

    return {'dict_to_matrix': dict_to_matrix, 'get_density_graph': get_density_graph, 'get_unfiltered_confidence_graph': get_unfiltered_confidence_graph,
            'filter_confidence_graph': filter_confidence_graph, 'remove_shortest_path': remove_shortest_path, 'update': update, 'fast_sort': fast_sort}


# ------------------------------------------------------------------ the spanning forest and its paths: fast_sort :567-595
FOREST_KEY = 'hhx_forest'             # T.graph[FOREST_KEY] = (label, pos) on the networkx graph the forest mirror returns
FOREST_MAX_SHAPE = 65535              # hhx_sort_graph_forest's limit (its sort key holds u * shape + v in 32 bits)


class ConfidenceToken:
    """What get_unfiltered_confidence_graph hands to fast_sort in place of the float64 array while that array stays on the device.  The forest seams
    recognise it; ANYTHING else done to it (numpy.asarray, indexing, an attribute) thaws it into the array through one fetch_confidence, after
    which the round is the reference's: Graph(token) is networkx's Graph of that array."""

    def __init__(self, graph, shape):
        self.__dict__.update(_graph=graph, _shape=shape, _pending=None, _filtered=False, _array=None)

    def _record(self, sub_HT_dict, cutoff, host_filter):
        self.__dict__['_pending'] = (sub_HT_dict, cutoff, host_filter)

    def _thaw(self):
        d = self.__dict__
        if d['_array'] is None:
            d['_array'] = d['_graph'].engine.fetch_confidence()
            d['_graph'].forest_thaws += 1
            if d['_pending'] is not None and not d['_filtered']:      # the cutoff was recorded, the device call that applies it never ran
                sub_HT_dict, cutoff, host_filter = d['_pending']
                host_filter(d['_array'], sub_HT_dict, cutoff)
            d['_filtered'] = True
        return d['_array']

    def __array__(self, dtype=None, copy=None):
        a = self._thaw()
        return a if dtype is None else a.astype(dtype)

    def __getattr__(self, name):                           # only what the token itself does not have
        if name.startswith('__') and name.endswith('__'):
            raise AttributeError(name)
        return getattr(self._thaw(), name)

    def __getitem__(self, key):
        return self._thaw()[key]

    def __setitem__(self, key, value):
        self._thaw()[key] = value

    def __len__(self):
        return len(self._thaw())

    def __iter__(self):
        return iter(self._thaw())


class _PathsFrom:
    def __init__(self, paths, source):
        self._paths, self._source = paths, source

    def __getitem__(self, target):
        return self._paths.path(self._source, target)

    def keys(self):
        return self._paths.keys()


class ForestPaths:
    """dict(shortest_path(tree))[source][target] for a tree of the forest mirror's T: a mapping whose values are mappings, every path read off `pos`
    when it is asked for — O(path length), where networkx computes all pairs."""

    def __init__(self, tree, pos):
        self._nodes = list(tree)
        self._pos = pos
        self._along = None

    def keys(self):
        return list(self._nodes)

    def __iter__(self):                                    # networkx 3.5: an iterator of (source, {target: path}) pairs; dict() takes either
        return iter(self._nodes)

    def __len__(self):
        return len(self._nodes)

    def __getitem__(self, source):
        return _PathsFrom(self, source)

    def path(self, source, target):
        if self._along is None:
            along = [None] * len(self._nodes)
            for v in self._nodes:
                along[self._pos[v]] = v
            self._along = along
        a, b = self._pos[source], self._pos[target]
        return self._along[a:b + 1] if a <= b else self._along[b:a + 1][::-1]


class NxTreeProxy:
    """What S.nxtree is re-bound to: networkx.tree, except maximum_spanning_tree(token, algorithm='kruskal')."""

    def __init__(self, module, forest):
        self._module, self._forest = module, forest

    def __getattr__(self, name):
        return getattr(self._module, name)

    def maximum_spanning_tree(self, G, *args, **kwargs):
        return self._forest(G, args, kwargs)


def bind_forest(S):
    """The forest block of fast_sort :567-595 on the device, for a module S that bind()'s mirrors are already bound to -> {name: object} for the
    globals fast_sort resolves at call time: get_unfiltered_confidence_graph (answers a ConfidenceToken and MAXS: no copy of the array),
    filter_confidence_graph (records the cutoff), Graph (passes the token on), nxtree (NxTreeProxy: one engine.forest(cutoff) call, then the real
    networkx graph T — nodes 0 .. shape - 1, then the chosen edges in Kruskal's order — which networkx's own connected_components / subgraph /
    degree answer on as they do on the reference's forest, so that the direction of every path is the reference's) and shortest_path (ForestPaths
    for a subgraph of such a T).  connected_components stays networkx's.

    A round goes to the reference's block, on the array fetched from the device, when: the forest is no set of paths (not_paths: the reference then
    fails its assert :586 as before); the engine has no forest(); the group is in host_mode or its sub_HT_dict is no longer the arrays the device
    holds; the token was thawed by foreign code; the shape exceeds 65535; maximum_spanning_tree is called with anything but algorithm='kruskal'."""
    prev_conf, prev_filter = getattr(S, 'get_unfiltered_confidence_graph', None), getattr(S, 'filter_confidence_graph', None)
    nx_graph, nx_tree, nx_shortest = getattr(S, 'Graph', None), getattr(S, 'nxtree', None), getattr(S, 'shortest_path', None)

    def _ours(sub_HT_dict, g):
        return _frozen(sub_HT_dict) or (sub_HT_dict is g.source and not g.host_mode)      # the edges bind()'s filter_confidence_graph works on

    def get_unfiltered_confidence_graph(shape, index_pairs, sub_HT_dict, density_graph):
        g = density_graph
        if (not isinstance(g, Graph) or g.host_mode or not hasattr(g.engine, 'forest') or shape > FOREST_MAX_SHAPE or not _ours(sub_HT_dict, g)):
            return prev_conf(shape, index_pairs, sub_HT_dict, density_graph)
        pairs = np.array(index_pairs, np.int32).reshape(-1, 2)
        maxs = g.engine.confidence_device(pairs[:, 0], pairs[:, 1])
        return ConfidenceToken(g, shape), maxs

    def filter_confidence_graph(confidence_graph, sub_HT_dict, confidence_cutoff):
        if not isinstance(confidence_graph, ConfidenceToken):
            return prev_filter(confidence_graph, sub_HT_dict, confidence_cutoff)
        d = confidence_graph.__dict__
        if d['_array'] is not None or not _ours(sub_HT_dict, d['_graph']):
            return prev_filter(confidence_graph._thaw(), sub_HT_dict, confidence_cutoff)
        confidence_graph._record(sub_HT_dict, confidence_cutoff, prev_filter)

    def graph(data=None, **attr):
        if isinstance(data, ConfidenceToken):
            return data if data.__dict__['_array'] is None else nx_graph(data.__dict__['_array'], **attr)
        return nx_graph(data, **attr)

    def forest(G, args, kwargs):
        if not isinstance(G, ConfidenceToken):
            return nx_tree.maximum_spanning_tree(G, *args, **kwargs)
        d = G.__dict__
        if d['_array'] is None and d['_pending'] is not None and not args and kwargs == {'algorithm': 'kruskal'}:
            g = d['_graph']
            eu, ev, label, pos, not_paths = g.engine.forest(d['_pending'][1])
            d['_filtered'] = True
            if not not_paths:
                g.forest_rounds += 1
                T = nx_graph()                             # networkx.Graph, as the module imported it
                T.add_nodes_from(range(d['_shape']))
                T.add_edges_from(zip(eu.tolist(), ev.tolist()))
                T.graph[FOREST_KEY] = (label.tolist(), pos.tolist())
                return T
        return nx_tree.maximum_spanning_tree(nx_graph(G._thaw()), *args, **kwargs)

    def shortest_path(G, *args, **kwargs):
        held = getattr(G, 'graph', None)
        held = held.get(FOREST_KEY) if isinstance(held, dict) else None
        if held is None or args or kwargs:
            return nx_shortest(G, *args, **kwargs)
        return ForestPaths(G, held[1])

    return {'get_unfiltered_confidence_graph': get_unfiltered_confidence_graph, 'filter_confidence_graph': filter_confidence_graph, 'Graph': graph,
            'nxtree': NxTreeProxy(nx_tree, forest), 'shortest_path': shortest_path}


# ------------------------------------------------------------------ fast sorting or ALLHiC: compare_fast_sort_and_allhic :645-724
class VerdictUnsupported(RuntimeError):
    """raised by a verdict engine for a group it does not serve: the mirror hands the call to the reference's function"""


def _default_verdict_engine(value, lengths, r0, r1):
    from . import _lib
    if DEVICE is not None:
        _lib.set_device(DEVICE)
    try:
        return _lib.sort_verdict_sums(value, lengths, r0, r1)
    except _lib.SortVerdictUnsupported as e:
        raise VerdictUnsupported(str(e))


def bind_verdict(S, engine=None):
    """The mirror of compare_fast_sort_and_allhic for the imported HapHiC_sort module S.  engine(value, lengths, r0, r1) -> the sums s[r0 .. r1) of
    include/haphic_hip.h's hhx_sort_verdict_sums (the device by default); it may raise VerdictUnsupported.

    Handed to the original function, which then raises or answers as it always did (and parses the tours again, so `Parsing tour files...` is logged
    once more): fewer than two contigs (:723 raises), a length that is not a non-negative int or lengths summing to 2^62 and more, an ALLHiC tour that
    is no permutation of the fast-sort tour (.index :699 raises, or longer), an engine that raises VerdictUnsupported."""
    sums_of = engine or _default_verdict_engine
    original = S.compare_fast_sort_and_allhic

    def compare_fast_sort_and_allhic(prefix, fa_dict):
        fast = list(S.parse_tours(['{}.tour.sav'.format(prefix)], fa_dict)[0].values())[0]
        n = len(fast)
        lengths = [fa_dict[ctg] for ctg, _ori in fast]
        if n < 2 or any(type(x) is not int or x < 0 for x in lengths):
            return original(prefix, fa_dict)
        group_len = sum(lengths)
        if group_len >= 1 << 62:
            return original(prefix, fa_dict)
        ratio = group_len / max(lengths)
        if ratio > 50:
            S.logger.info('{}: choose allhic optimization (group length / longest contig = {})'.format(prefix, ratio))
            return False
        allhic = list(S.parse_tours(['{}.tour'.format(prefix)], fa_dict)[0].values())[0]
        where = {ctg: (j, ori) for j, (ctg, ori) in enumerate(allhic)}
        if len(allhic) != n or any(ctg not in where for ctg, _ori in fast):
            return original(prefix, fa_dict)
        value = [where[ctg][0] + 1 if ori == where[ctg][1] else -where[ctg][0] - 1 for ctg, ori in fast]
        try:
            with DEVICE_LOCK:                                  # called from the threads of run()'s pool
                sums = [int(x) for x in sums_of(value, lengths, 0, 1)]
            if sums[0] / group_len < 0.9 and n > 2:            # rotation 0 settles it when the tours agree (the reference's early exit :714)
                with DEVICE_LOCK:
                    sums += [int(x) for x in sums_of(value, lengths, 1, n - 1)]
        except VerdictUnsupported:
            return original(prefix, fa_dict)
        for max_sum in sums:
            if max_sum / group_len >= 0.9:
                S.logger.info('{}: choose allhic optimization (LIS length / group length = {})'.format(prefix, max_sum / group_len))
                return False
        # :723 prints the ratio of the last rotation looked at, whatever its wording says
        S.logger.info('{}: choose fast sorting (maximum LIS length / group length = {})'.format(prefix, sums[-1] / group_len))
        return True
    compare_fast_sort_and_allhic.__wrapped__ = original
    return compare_fast_sort_and_allhic


# ------------------------------------------------------------------ each group's H/T links from HT_links.pkl: run() :898-923, get_sub_HT_dict :117-143
class _HeadsSession:
    """what the containers below need of a session; the table's one also owns the open file (engine: _lib.LinkPickle or a stand-in)"""

    def __init__(self, engine=None):
        self.engine = engine
        self.thaws = 0

    def note_thawed(self):
        self.thaws += 1
        engine, self.engine = self.engine, None
        if engine is not None:
            engine.close()                                 # the dict holds every key now


class HTTable(containers._Frozen):
    """HT_link_dict of run() :899-901 while it is the arrays hhx_pickle_open left in the memory of the device: {(name, name): links}.  The
    get_sub_HT_dict mirror works on the open handle; ANY other access thaws it into the defaultdict(int) pickle.load builds from the file, key by
    key in the file's order.  When the table goes away (`del HT_link_dict; gc.collect()` :922-923) a finalizer closes the handle."""

    def __init__(self, engine):
        import weakref
        containers._Frozen.__init__(self, int, _HeadsSession(engine), 'HT_links')
        self._ids = None
        self._finalizer = weakref.finalize(self, engine.close)

    def _n(self):
        return int(self._session.engine.n_keys)

    def name_ids(self):
        """{name: id}, from one fetch of the names alone"""
        if self._ids is None:
            names = self._session.engine.names()
            self._ids = dict(zip(names, range(len(names))))
        return self._ids

    def _source_items(self):
        from . import reassign
        arrays = self._session.engine.arrays()
        if arrays is None:
            raise RuntimeError('HT_links: the table on the device cannot be turned into a dict (a name that is not UTF-8, or integers beyond 2^53 beside floats)')
        return containers.LinkTable(reassign.PickleSession(*arrays), 'full')._source_items()


class HeadsHT(containers._Frozen):
    """The sub_HT_dict of get_sub_HT_dict :117-143: {(index, index): links} in the reference's insertion order — three arrays (int32, int32, int64)
    until something other than the seams touches it; then the defaultdict(int) of Python ints the reference builds."""

    def __init__(self, i, j, w):
        containers._Frozen.__init__(self, int, _HeadsSession(), 'sub_HT_heads')
        self.i, self.j, self.w = i, j, w

    def _n(self):
        return int(self.i.size)

    def _source_items(self):
        return zip(zip(self.i.tolist(), self.j.tolist()), self.w.tolist())

    def drop_touching(self, a, b):
        keep = ~((self.i == a) | (self.i == b) | (self.j == a) | (self.j == b))
        self.i, self.j, self.w = self.i[keep], self.j[keep], self.w[keep]

    def round1_arrays(self, shape):
        """what _round1_arrays answers for the thawed dict, from the arrays"""
        n = self.i.size
        if n == 0 or shape < 4 or shape % 2 or int(self.w.min()) < 0 or int(self.w.max()) > 2 ** 53:
            return None
        if int(self.i.max()) >= shape or int(self.j.max()) >= shape:
            return None
        return self.i, self.j, self.w


def _frozen_heads(d):
    return isinstance(d, HeadsHT) and d.frozen


class PickleProxy:
    """What S.pickle is re-bound to: the pickle module, except that load(f) of a real file open for reading at its start goes through the device
    reader and answers an HTTable; a file the reader refuses, and every other call, is pickle's own."""

    def __init__(self, module, open_engine):
        self._module, self._open = module, open_engine
        self.tables = []                                   # the session of every table made here: .engine (None once closed by a thaw), .thaws

    def __getattr__(self, name):                           # only what the proxy itself does not have
        return getattr(self._module, name)

    def load(self, file, *args, **kwargs):
        import os
        path = getattr(file, 'name', None)
        try:
            ours = (not args and not kwargs and isinstance(path, (str, bytes)) and os.path.isfile(path) and 'b' in getattr(file, 'mode', '')
                    and file.tell() == 0)
        except (OSError, ValueError):
            ours = False
        engine = self._open(path) if ours else None
        if engine is None:
            return self._module.load(file, *args, **kwargs)
        file.seek(0, 2)                                    # as after pickle.load: the file has been read
        table = HTTable(engine)
        self.tables.append(table._session)
        return table


def _default_heads_engine(path):
    from . import _lib
    if DEVICE is not None:
        _lib.set_device(DEVICE)
    return _lib.LinkPickle.open(path)


def bind_heads(S, engine=None):
    """-> (the pickle proxy, the mirror of get_sub_HT_dict :117-143) for the imported HapHiC_sort module S.  engine(path): a stand-in for
    _lib.LinkPickle.open (the tests' host reader): an object with n_keys, n_names, any_float, names(), arrays(), group_heads(n, slot, rank) and
    close(), or None for a file it does not answer.  proxy.tables lists the session of every table the proxy made (engine None after a thaw;
    thaws counts the thaws).

    get_sub_HT_dict(ctgs, HT_link_dict) for a frozen HTTable: HT_index_dict is the real dict, by its closed form; sub_HT_dict is a HeadsHT over the
    arrays of one hhx_pickle_group_heads call (the host does 2 n dict look-ups for the slots and one sort of the names).  Fewer than two contigs:
    the two empty results, no device call.  Handed to the reference's function — on the thawed table when it was one of ours: a plain dict, a
    table that was thawed, a contig listed twice or one that is no str, a table with float values, 2 n beyond int32."""
    import pickle
    from collections import defaultdict
    original = getattr(S, 'get_sub_HT_dict', None)
    proxy = PickleProxy(pickle, engine or _default_heads_engine)

    def get_sub_HT_dict(ctgs, HT_link_dict):
        if not (isinstance(HT_link_dict, HTTable) and HT_link_dict.frozen):
            return original(ctgs, HT_link_dict)
        n = len(ctgs)
        if n < 2:
            return defaultdict(int), dict()
        eng = HT_link_dict._session.engine
        if eng.any_float or 2 * n > 2 ** 31 - 1 or any(type(c) is not str for c in ctgs) or len(set(ctgs)) != n:
            return original(ctgs, HT_link_dict)
        ids = HT_link_dict.name_ids()
        slot = np.full(eng.n_names, -1, np.int32)
        for pos, ctg in enumerate(ctgs):
            for suffix, tail in enumerate(('_H', '_T')):
                k = ids.get(ctg + tail)
                if k is not None:
                    slot[k] = 2 * pos + suffix
        rank = np.empty(n, np.int32)
        rank[sorted(range(n), key=ctgs.__getitem__)] = np.arange(n, dtype=np.int32)
        ei, ej, w = eng.group_heads(n, slot, rank)
        lo, hi = sorted(ctgs[:2])
        HT_index_dict = {lo + '_H': 0, hi + '_H': 1, hi + '_T': 2, lo + '_T': 3}
        for k in range(2, n):
            HT_index_dict[ctgs[k] + '_H'] = 2 * k
            HT_index_dict[ctgs[k] + '_T'] = 2 * k + 1
        return HeadsHT(ei, ej, w), HT_index_dict
    get_sub_HT_dict.__wrapped__ = original
    return proxy, get_sub_HT_dict
