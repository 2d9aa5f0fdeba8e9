"""remove_allelic_HiC_links() :474-692 on the device tables (--remove_allelic_links, BASELINE.json configs[3]).

The reference walks ctg_coord_dict and full_link_dict key by key; with the array-backed containers of the S5 mirrors
(containers.py) that walk first thaws three tables into Python dicts.  Here everything that touches every key runs on the
device (haphic_amd/csrc/hhx_allelic.hip):

    stage 1   cal_concordance_ratio :419-428 of every eligible key as integer modal counts (hhx_ingest_concordance);
              the ratio is formed here, in float64, by the same two divisions as :428
    stage 2   the links between non-maximum matches :621-667 (hhx_allelic_nonmax through nonmax_keys_device): the candidate keys times their
              allele groups, the unique group pairs, their matrices, linear_sum_assignment and the mismatch verdict
    verdict   update_link_dicts :488-509 for both stages at once, and the isolated fragments :678-692 (hhx_ingest_drop_links)

and the allele groups between stage 1 and 2 stay host code (networkx cliques on the few allelic keys, split_cliques / get_weakest_edge
restated from :511-550).  Stage 2 must pick scipy's assignment among equal optima: the device solver restates scipy's method step by step, and
lsap_small() below is the same in Python, its oracle.  nonmax_keys() is the host form of stage 2 — numpy on ARRAYS plus one
scipy.optimize.linear_sum_assignment call per unique pair of allele groups that more than one key connects (a pair connected by a single
key has one non-zero cell in its matrix, which every optimal assignment contains).  It is the specification of the device form and serves when
the engine is not the library's own Ingest (and has no nonmax_keys method of its own), when HAPHIC_ALLELIC_STAGE2=host, and when an allele group
has more than 8 contigs; STATS['stage2_engine'] says which form ran.

The array path is taken only when the containers are still frozen on one live session and the run is the plain one; every
other call goes to the reference's own function (`_original`, bound by patch.patch_reference(H, allelic=True)), which thaws as before:
  * full_link_dict, flank_link_dict and ctg_coord_dict are frozen and share one IngestSession; flank_link_dict is not empty
    and filtered_frags is given (and names only fragments of the table);
  * --remove_concentrated_links is off (the reference forces it off, :2783) and args.ul is not set;
  * the logger is not at DEBUG (the per-key debug lines :582-599, :672, :690 are the original's business);
  * every contig is at least nwindows bp long (else the window width is 0 and the reference raises);
  * the engine has concordance_counts / drop_links and serves the call (max_read_pairs within its cap);
  * no `assert` of :652-659 would fail (then the original raises it).
"""
import logging
import os
import time

import numpy as np

from . import _lib as _hip
from . import cluster

logger = cluster.logger

STATS = {}     # of the last array-path call (measurement only): seconds per step, candidates, unique group pairs, assignment problems solved and their seconds


def _edges_graph(inter_i, inter_j, inter_cnt):
    """the Graph that `Graph(dict_to_matrix(inter_allele_dict, allelic_ctg_set)[0])` :603-606 builds, without the dense matrix:
    nodes = matrix indices (first-seen order over the keys, i before j: dict_to_matrix :337-349), every edge entered from both of
    its ends in row-major order of the matrix with its float32 weight, as networkx reads an ndarray.  Returns (graph, node -> contig id)."""
    from networkx import Graph
    both = np.stack([inter_i, inter_j], axis=1).ravel()
    seen, first = np.unique(both, return_index=True)
    index_ctg = seen[np.argsort(first, kind='stable')]
    index_of = np.zeros(int(both.max()) + 1 if len(both) else 1, np.int64)
    index_of[index_ctg] = np.arange(len(index_ctg))
    a, b = index_of[inter_i], index_of[inter_j]
    w = np.asarray(inter_cnt, np.float32)                      # coo_matrix(..., dtype=float32) :371
    rows, cols, vals = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    order = np.lexsort((cols, rows))
    graph = Graph()
    graph.add_nodes_from(range(len(index_ctg)))
    graph.add_weighted_edges_from(zip(rows[order].tolist(), cols[order].tolist(), vals[order].astype(float).tolist()))
    return graph, index_ctg


def _get_weakest_edge(graph):                                  # :511-523
    weakest_edge = (None, None, np.inf)
    for node1, node2, data in graph.edges(data=True):
        if node1 == node2:
            continue
        if data['weight'] < weakest_edge[-1]:
            weakest_edge = (node1, node2, data['weight'])
    assert weakest_edge[0] is not None
    return weakest_edge


def _split_cliques(graph, cliques, ploidy, cached_cliques):    # :525-550
    from networkx import Graph, find_cliques
    new_cliques = set()
    for clique in cliques:
        clique = tuple(clique)
        if len(clique) > ploidy:
            if clique not in cached_cliques:
                subgraph = graph.subgraph(clique)
                node1, node2, _ = _get_weakest_edge(subgraph)
                subgraph = Graph(subgraph)                     # unfreeze
                subgraph.remove_edge(node1, node2)
                sub_cliques = find_cliques(subgraph)
                cached_cliques.add(clique)
                new_cliques |= _split_cliques(subgraph, sub_cliques, ploidy, cached_cliques)
        else:
            new_cliques.add(tuple(clique))
    return new_cliques


def allele_groups(inter_i, inter_j, inter_cnt, names, ploidy):
    """:601-619 — the allele groups of the inter-allele keys (contig ids into `names`, counts, in full_link_dict order) as a list of
    sorted name tuples, without duplicates.  ploidy 2: the keys themselves; above that the cliques of the allele graph, split at
    their weakest edge until none has more than `ploidy` members (needs networkx)."""
    if ploidy > 2:
        from networkx import find_cliques
        if not len(inter_i):
            return []
        graph, index_ctg = _edges_graph(inter_i, inter_j, inter_cnt)
        groups = _split_cliques(graph, find_cliques(graph), ploidy, set())
        return list({tuple(sorted(names[index_ctg[i]] for i in group)) for group in groups})
    return list({(names[a], names[b]) for a, b in zip(np.asarray(inter_i).tolist(), np.asarray(inter_j).tolist())})


def _segments(lengths):
    """(owner, offset inside the owner) of every slot of consecutive segments with these lengths"""
    lengths = np.asarray(lengths, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    owner = np.repeat(np.arange(len(lengths)), lengths)
    return owner, np.arange(int(ptr[-1])) - ptr[owner], ptr


def nonmax_keys(si, sj, scnt, groups, names, ctg_rank, stats=None):
    """:621-667 on arrays.  (si, sj, scnt): the keys of full_link_dict after stage 1, in dict order; groups: allele_groups().  Returns the
    boolean mask of the keys that are not part of the maximum matching of some pair of allele groups they connect, or None when an
    `assert` of :652-659 would fail somewhere (the caller lets the reference raise it)."""
    from scipy.optimize import linear_sum_assignment
    stats = {} if stats is None else stats
    n_ctg = len(names)
    out = np.zeros(len(si), bool)
    stats.update(candidates=0, group_pairs=0, assignments=0, assignment_s=0.0)
    if not len(groups) or not len(si):
        return out
    cid = {n: k for k, n in enumerate(names)}
    groups = sorted(groups)                                    # position = rank under tuple comparison: tuple(sorted([group_1, group_2])) :644
    glen = np.fromiter(map(len, groups), np.int64, len(groups))
    gmem = np.fromiter((cid[c] for g in groups for c in g), np.int64, int(glen.sum()))
    gown, gpos, gptr = _segments(glen)
    nG = len(groups)
    # position of contig c inside group g (or -1): sorted (g, c) cells
    cell = gown * n_ctg + gmem
    cell_order = np.argsort(cell, kind='stable')
    cell_sorted, cell_pos = cell[cell_order], gpos[cell_order]

    def pos_in(g, c):
        want = g * n_ctg + c
        at = np.minimum(np.searchsorted(cell_sorted, want), len(cell_sorted) - 1)
        return np.where(cell_sorted[at] == want, cell_pos[at], -1)
    # the groups of every contig (ctg_allele_group_dict :624-627)
    by_ctg = np.argsort(gmem, kind='stable')
    cg_grp = gown[by_ctg]
    cg_deg = np.bincount(gmem, minlength=n_ctg)
    cg_ptr = np.concatenate([[0], np.cumsum(cg_deg)])
    si, sj = np.asarray(si, np.int64), np.asarray(sj, np.int64)
    cand = np.flatnonzero((cg_deg[si] > 0) & (cg_deg[sj] > 0))                       # :639
    stats['candidates'] = int(len(cand))
    if not len(cand):
        return out
    c1, c2 = si[cand], sj[cand]
    d1, d2 = cg_deg[c1], cg_deg[c2]
    own, off, _ = _segments(d1 * d2)                           # one slot per (key, group_1, group_2) :642-643
    g1 = cg_grp[cg_ptr[c1[own]] + off // d2[own]]
    g2 = cg_grp[cg_ptr[c2[own]] + off % d2[own]]
    ga, gb = np.minimum(g1, g2), np.maximum(g1, g2)            # group_pair :644
    k1, k2 = c1[own], c2[own]
    p1a = pos_in(ga, k1)
    first = p1a >= 0                                           # :652 ctg_1 in group_pair[0]
    index_1 = np.where(first, p1a, pos_in(ga, k2))
    index_2 = np.where(first, pos_in(gb, k2), pos_in(gb, k1))
    if (index_1 < 0).any() or (index_2 < 0).any():             # :653 / :657 would raise
        return None
    # the unique group pairs and their degree x degree matrices (:552-568).  Every non-zero cell of such a matrix is a surviving key between the two
    # groups, and every such key is one of the candidates and lists this very pair among its combinations: the matrices are filled by scattering
    # the candidates' counts (in both roles where a contig sits in both groups), not by looking every cell up
    pair, inv = np.unique(ga * nG + gb, return_inverse=True)
    pa, pb = pair // nG, pair % nG
    stats['group_pairs'] = int(len(pair))
    degree = np.maximum(glen[pa], glen[pb])
    mat_ptr = np.concatenate([[0], np.cumsum(degree * degree)])
    flat = np.zeros(int(mat_ptr[-1]), np.int64)
    links = np.asarray(scnt, np.int64)[cand][own]
    deg = degree[inv]
    r1, c1_ = p1a, pos_in(gb, k2)                              # ctg_1 as a row of group_pair[0], ctg_2 as a column of group_pair[1]
    ok = (r1 >= 0) & (c1_ >= 0)
    flat[mat_ptr[inv[ok]] + r1[ok] * deg[ok] + c1_[ok]] = links[ok]
    r2, c2_ = pos_in(ga, k2), pos_in(gb, k1)                   # ... and the other way round
    ok = (r2 >= 0) & (c2_ >= 0)
    flat[mat_ptr[inv[ok]] + r2[ok] * deg[ok] + c2_[ok]] = links[ok]
    # A matrix with a single non-zero cell needs no solver: every optimal assignment contains that cell (any other sums to 0), and the
    # cell is the only key that asks.  The rest go through scipy one by one, for its tie-breaking (:568)
    cells = np.add.reduceat((flat != 0).astype(np.int64), mat_ptr[:-1])
    solve = np.flatnonzero(cells > 1)
    stats['assignments'] = int(len(solve))
    sol_ptr = np.zeros(len(pair) + 1, np.int64)
    sol_ptr[solve + 1] = degree[solve]
    sol_ptr = np.cumsum(sol_ptr)
    solution = np.empty(int(sol_ptr[-1]), np.int64)
    t0 = time.perf_counter()
    neg = -flat
    for u, d, at, to in zip(solve.tolist(), degree[solve].tolist(), mat_ptr[solve].tolist(), sol_ptr[solve].tolist()):
        solution[to:to + d] = linear_sum_assignment(neg[at:at + d * d].reshape(d, d))[1]
    stats['assignment_s'] = time.perf_counter() - t0
    asked = cells[inv] > 1
    mismatch = np.zeros(len(inv), bool)
    mismatch[asked] = solution[sol_ptr[inv[asked]] + index_1[asked]] != index_2[asked]      # :661
    out[cand[np.unique(own[mismatch])]] = True
    return out


def lsap_small(cost):
    """scipy.optimize.linear_sum_assignment(cost)[1] of a square integer matrix, restated step by step from scipy 1.15's solver (the shortest
    augmenting path method with dual variables, Crouse's variant of Jonker-Volgenant), in Python integers: the CPU oracle of the device
    solver (csrc/hhx_allelic.hip lsap_solve) and the documentation of the order and tie rule that make the result scipy's among equal optima —
      * the unvisited columns are scanned in the order of `remaining`, which starts as [d-1 .. 0] and loses a visited column by moving its last
        element into that slot;
      * a column as cheap as the cheapest so far replaces it only when it is unassigned.
    Every quantity is a sum or difference of the costs, which scipy's doubles hold exactly below 2^53."""
    cost = [[int(x) for x in row] for row in np.asarray(cost).tolist()]
    d = len(cost)
    inf = None                                                   # +inf of shortestPathCosts: compared, never added to
    u, v = [0] * d, [0] * d
    col4row, row4col, path = [-1] * d, [-1] * d, [-1] * d
    for cur in range(d):
        remaining = list(range(d - 1, -1, -1))
        shortest = [inf] * d
        SR, SC = [False] * d, [False] * d
        min_val, i, sink = 0, cur, -1
        while sink == -1:
            index, lowest = -1, inf
            SR[i] = True
            for it, j in enumerate(remaining):
                r = min_val + cost[i][j] - u[i] - v[j]
                if shortest[j] is inf or r < shortest[j]:
                    path[j] = i
                    shortest[j] = r
                if lowest is inf or shortest[j] < lowest or (shortest[j] == lowest and row4col[j] == -1):
                    lowest = shortest[j]
                    index = it
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            remaining[index] = remaining[-1]
            remaining.pop()
        u[cur] += min_val
        for k in range(d):
            if SR[k] and k != cur:
                u[k] += min_val - shortest[col4row[k]]
        for j in range(d):
            if SC[j]:
                v[j] -= min_val - shortest[j]
        j = sink
        while True:                                              # flip the path back from the sink
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return np.asarray(col4row, np.int64)


def nonmax_keys_device(si, sj, scnt, groups, names, ctg_rank, stats=None):
    """nonmax_keys on the device (hhx_allelic_nonmax): the same arguments, the same mask (or None), the same `stats`; NotImplemented when the
    library does not serve the call (an allele group of more than 8 contigs).  The host part is the group table alone."""
    stats = {} if stats is None else stats
    stats.update(candidates=0, group_pairs=0, assignments=0, assignment_s=0.0)
    cid = {n: k for k, n in enumerate(names)}
    groups = sorted(groups)                                    # position = rank under tuple comparison :644
    glen = np.fromiter(map(len, groups), np.int64, len(groups))
    gmem = np.fromiter((cid[c] for g in groups for c in g), np.int32, int(glen.sum()))
    gptr = np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)
    got = _hip.allelic_nonmax(si, sj, scnt, len(names), gptr, gmem)
    if got is None or got is NotImplemented:
        return got
    mask, counters = got
    stats.update(candidates=int(counters[0]), group_pairs=int(counters[1]), assignments=int(counters[2]))
    return mask.astype(bool)


STAGE2_DEFAULT = 'device'      # what the real engine takes when HAPHIC_ALLELIC_STAGE2 (host / device) does not say


def _stage2(engine):
    """(the function that serves stage 2 with this engine, 'device' / 'host'): a stand-in engine's own nonmax_keys, the device form with the real
    engine unless the environment says host, else the host form"""
    own = getattr(engine, 'nonmax_keys', None)
    if own is not None:
        return own, 'device'
    if isinstance(engine, _hip.Ingest) and os.environ.get('HAPHIC_ALLELIC_STAGE2', STAGE2_DEFAULT) != 'host':
        return nonmax_keys_device, 'device'
    return nonmax_keys, 'host'


def _array_path(fa_dict, ctg_coord_dict, full_link_dict, args, flank_link_dict, filtered_frags, ctg_pair_to_frag, log, engine):
    """the session when the call can run on the arrays, else None"""
    frozen = cluster._frozen
    if not (frozen(full_link_dict, 'full') and frozen(flank_link_dict, 'flank') and frozen(ctg_coord_dict, 'crd')):
        return None
    session = full_link_dict._session
    if flank_link_dict._session is not session or ctg_coord_dict._session is not session or getattr(session, 'ing', None) is None:
        return None
    if filtered_frags is None or not len(flank_link_dict):
        return None
    if getattr(args, 'remove_concentrated_links', False) or getattr(args, 'ul', None) or log.isEnabledFor(logging.DEBUG):
        return None
    if bool(ctg_pair_to_frag) != bool(getattr(session, 'bins', False)):
        return None
    if len(session.table.ctg_len) and int(session.table.ctg_len.min()) < int(args.nwindows):
        return None
    engine = session.ing if engine is None else engine
    if not (hasattr(engine, 'concordance_counts') and hasattr(engine, 'drop_links')):
        return None
    return session


def remove_allelic_HiC_links(fa_dict, ctg_coord_dict, full_link_dict, args, flank_link_dict=None, filtered_frags=None,
                             ctg_pair_to_frag=None, logger=logger, _original=None, _engine=None):
    """remove_allelic_HiC_links() :474-692 (see the module docstring).  Returns remaining_frags, a set of fragment names built in the
    order :680-683 meets them."""
    def original():
        if _original is None:
            raise ValueError('remove_allelic_HiC_links: this call is the reference function\'s (see haphic_amd/allelic.py) and none was bound')
        return _original(fa_dict, ctg_coord_dict, full_link_dict, args, flank_link_dict, filtered_frags, ctg_pair_to_frag, logger)

    session = _array_path(fa_dict, ctg_coord_dict, full_link_dict, args, flank_link_dict, filtered_frags, ctg_pair_to_frag, logger, _engine)
    if session is None:
        return original()
    t_start = time.perf_counter()
    engine = session.ing if _engine is None else _engine
    table = session.table
    frag_names, names = table.frag_names, table.ctg_names
    in_set = np.fromiter(map(filtered_frags.__contains__, frag_names), np.uint8, len(frag_names))
    if int(in_set.sum()) != len(filtered_frags):               # a name that is no fragment of the table
        return original()
    ploidy, min_read_pairs, max_read_pairs = int(args.remove_allelic_links), int(args.min_read_pairs), int(args.max_read_pairs)
    # ---- 1) the keys whose read pairs sit on one diagonal (:578-599)
    counts = engine.concordance_counts(max_read_pairs, int(args.nwindows), min_read_pairs)
    if counts is None:
        return original()
    t_counts = time.perf_counter()
    m, diag, anti = counts
    fi, fj, cnt, _ = full_link_dict.arrays()
    eligible = (cnt >= max_read_pairs) | (m >= min_read_pairs)                       # the collapsed entries :581 | :589
    ratio = np.zeros(len(m), np.float64)
    ratio[eligible] = np.maximum(diag[eligible] / m[eligible], anti[eligible] / m[eligible])   # :428
    allelic = eligible & (ratio > args.concordance_ratio_cutoff)
    # ---- the allele groups (:601-619) from inter_allele_dict, the small dict of the allelic keys
    inter = np.flatnonzero(allelic)
    groups = allele_groups(fi[inter], fj[inter], cnt[inter], names, ploidy)
    t_groups = time.perf_counter()
    # ---- 2) links between non-max matches (:621-667), among the keys that are left
    stats = {}
    left = np.flatnonzero(~allelic)
    stage2, stage2_engine = _stage2(engine)
    nonmax = stage2(fi[left], fj[left], cnt[left], groups, names, table.ctg_rank, stats)
    if nonmax is NotImplemented:                               # not served there (an allele group beyond the solver's size)
        stage2_engine = 'host'
        nonmax = nonmax_keys(fi[left], fj[left], cnt[left], groups, names, table.ctg_rank, stats)
    if nonmax is None:
        return original()
    t_nonmax = time.perf_counter()
    logger.info("Removing Hi-C links between alleic contig pairs...")                # :476 (nothing was changed before this point)
    full_drop = allelic.copy()
    full_drop[left[nonmax]] = True
    dropped = engine.drop_links(full_drop, in_set)
    if dropped is None:
        return original()
    session.links_dropped()
    _n_full, _n_flank, _flank_dropped, remaining = dropped
    # ---- isolated fragments (:678-692)
    kept = np.flatnonzero(remaining)
    first_row = getattr(engine, 'first_row', None)
    if first_row is not None:
        kept = kept[np.argsort(first_row[kept], kind='stable')]
    remaining_frags = set()
    for f in kept.tolist():
        remaining_frags.add(frag_names[f])
    logger.info('Removing isolated fragments after filtering out allelic Hi-C links...')
    logger.info('{} fragments removed, {} fragments kept'.format(len(filtered_frags) - len(remaining_frags), len(remaining_frags)))
    t_end = time.perf_counter()
    STATS.clear()
    STATS.update(stats, stage2_engine=stage2_engine, keys=int(len(m)), stage1_keys=int(allelic.sum()), allele_groups=len(groups), stage2_keys=int(nonmax.sum()),
                 concordance_s=t_counts - t_start, groups_s=t_groups - t_counts, stage2_s=t_nonmax - t_groups, drop_s=t_end - t_nonmax,
                 total_s=t_end - t_start)
    return remaining_frags
