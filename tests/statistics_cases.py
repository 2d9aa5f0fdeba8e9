"""Cases and CPU engines for output_statistics :2279-2478 on the device tables (haphic_amd/statistics.py, csrc/hhx_groupstats.hip).

  * Case: contigs (names, lengths, RE sites = fa_dict), the keys of full_link_dict in dict order with their counts, and one list of clusters per
    inflation.  Every key is (i, j) with i < j and the names sort like the ids, so that an ingest handle orients the keys the same way.
  * dict_group_stats: the semantics restated per key with real dicts, as the reference's parse_link_dict :2252-2268 and :2361-2384 do it.
  * group_stats: a numpy engine with the signature of haphic_amd._lib.group_stats — the CPU stand-in of the library.
  * plain_sum / neumaier_sum: the two summations as pure-Python loops."""
import math

import numpy as np


# ------------------------------------------------------------------ the two summations
def plain_sum(xs):
    total = 0.0
    for x in xs:
        total += x
    return total


def neumaier_sum(xs):
    """sum() of CPython >= 3.12 on floats (Neumaier's variant of Kahan-Babuska), with its last step"""
    total, c = 0.0, 0.0
    for x in xs:
        t = total + x
        if abs(total) >= abs(x):
            c += (total - t) + x
        else:
            c += (x - t) + total
        total = t
    if c and math.isfinite(c):
        total += c
    return total


SUMS = {0: plain_sum, 1: neumaier_sum}


# ------------------------------------------------------------------ (i) the semantics with real dicts
def dict_group_stats(frag_i, frag_j, links, group, n_groups, group_re, ctg_re, sum_mode=0):
    group = np.asarray(group)
    n_sets, n_ctg = group.shape
    out = (np.zeros((n_sets, n_ctg), np.int32), np.zeros((n_sets, n_ctg), np.int64), np.full((n_sets, n_ctg), -1, np.int32), np.zeros((n_sets, n_ctg)))
    off = np.concatenate(([0], np.cumsum(n_groups))).tolist()
    keys = list(zip(np.asarray(frag_i).tolist(), np.asarray(frag_j).tolist(), np.asarray(links).tolist()))
    cre = np.asarray(ctg_re).tolist()
    for s in range(n_sets):
        grp = group[s].tolist()
        gre = np.asarray(group_re)[off[s]:off[s + 1]].tolist()
        cells = {}
        for a, b, v in keys:
            for ctg, g in ((a, grp[b]), (b, grp[a])):
                if g != -1:
                    inner = cells.setdefault(ctg, {})
                    inner[g] = inner.get(g, 0) + v
        for ctg, inner in cells.items():
            ranked = sorted(inner.items(), key=lambda x: x[1], reverse=True)
            dens = [v / gre[g] if g == grp[ctg] else v / (gre[g] + cre[ctg] - 1) for g, v in ranked[1:]]
            out[0][s, ctg], out[1][s, ctg], out[2][s, ctg], out[3][s, ctg] = len(ranked), ranked[0][1], ranked[0][0], SUMS[sum_mode](dens)
    return out


# ------------------------------------------------------------------ (ii) the numpy engine
def group_stats(frag_i, frag_j, links, group, n_groups, group_re, ctg_re, sum_mode=0):
    """(n_cells, max_links, max_group, other_sum), each [n_sets, n_ctg]: include/haphic_hip.h, hhx_group_stats"""
    if sum_mode not in (0, 1):
        return None
    fi, fj, lk = np.asarray(frag_i, np.int64), np.asarray(frag_j, np.int64), np.asarray(links, np.int64)
    group = np.asarray(group, np.int64)
    n_sets, n_ctg = group.shape
    cre = np.asarray(ctg_re, np.int64)
    off = np.concatenate(([0], np.cumsum(n_groups))).astype(np.int64)
    ctg = np.stack([fi, fj], axis=1).ravel()
    val = np.repeat(lk, 2)
    pos = np.arange(2 * len(fi), dtype=np.int64)
    out = (np.zeros((n_sets, n_ctg), np.int32), np.zeros((n_sets, n_ctg), np.int64), np.full((n_sets, n_ctg), -1, np.int32), np.zeros((n_sets, n_ctg)))
    for s in range(n_sets):
        grp = group[s]
        gre = np.asarray(group_re, np.int64)[off[s]:off[s + 1]]
        G = max(int(n_groups[s]), 1)
        other = np.stack([grp[fj], grp[fi]], axis=1).ravel()
        keep = other >= 0
        if not keep.any():
            continue
        cell, inverse = np.unique(ctg[keep] * G + other[keep], return_inverse=True)
        sums = np.zeros(len(cell), np.int64)
        np.add.at(sums, inverse, val[keep])
        first = np.full(len(cell), np.iinfo(np.int64).max, np.int64)
        np.minimum.at(first, inverse, pos[keep])
        c_ctg, c_grp = cell // G, cell % G
        order = np.lexsort((first, -sums, c_ctg))                  # by contig, then links descending, then first contribution
        c_ctg, c_grp, sums = c_ctg[order], c_grp[order], sums[order]
        head = np.flatnonzero(np.diff(c_ctg, prepend=-1))
        n_cells = np.diff(np.append(head, len(c_ctg)))
        rows = c_ctg[head]
        out[0][s, rows], out[1][s, rows], out[2][s, rows] = n_cells, sums[head], c_grp[head]
        den = np.where(c_grp == grp[c_ctg], gre[c_grp], gre[c_grp] + cre[c_ctg] - 1)
        q = sums / den
        rank = np.arange(len(c_ctg)) - np.repeat(head, n_cells)
        total, comp = np.zeros(n_ctg), np.zeros(n_ctg)
        for r in range(1, int(n_cells.max())):                     # one addition per contig at a time: the order of the reference's sum()
            at = np.flatnonzero(rank == r)
            ctgs, x = c_ctg[at], q[at]
            t = total[ctgs] + x
            if sum_mode == 1:
                big = np.abs(total[ctgs]) >= np.abs(x)
                comp[ctgs] += np.where(big, (total[ctgs] - t) + x, (x - t) + total[ctgs])
            total[ctgs] = t
        if sum_mode == 1:
            add = (comp != 0) & np.isfinite(comp)
            total[add] += comp[add]
        out[3][s] = total
    return out


# ------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, lengths, re_sites, fi, fj, cnt, sets, handle=True):
        """sets: [(inflation label, [[contig ids of cluster 0], ...]), ...]; handle: the counts are small enough to be pushed as read pairs"""
        self.name = name
        self.lengths, self.re_sites = np.asarray(lengths, np.int64), np.asarray(re_sites, np.int64)
        self.fi, self.fj, self.cnt = np.asarray(fi, np.int32), np.asarray(fj, np.int32), np.asarray(cnt, np.int64)
        assert (self.fi < self.fj).all() and len(set(zip(self.fi.tolist(), self.fj.tolist()))) == len(self.fi)
        self.sets = [(str(label), [list(map(int, c)) for c in clusters]) for label, clusters in sets]
        self.names = ['ctg%06d' % k for k in range(len(self.lengths))]
        self.handle = handle

    @property
    def n_ctg(self):
        return len(self.lengths)

    def fa_dict(self):
        return {n: ['', int(length), int(re)] for n, length, re in zip(self.names, self.lengths, self.re_sites)}

    def link_dict(self):
        return {(self.names[a], self.names[b]): int(c) for a, b, c in zip(self.fi.tolist(), self.fj.tolist(), self.cnt.tolist())}

    def result_clusters_list(self):
        return [(label, [([self.names[c] for c in cluster], None) for cluster in clusters]) for label, clusters in self.sets]

    def engine_args(self):
        """(group [n_sets, n_ctg], n_groups, group_re, ctg_re) the way the mirror forms them"""
        group = np.full((len(self.sets), self.n_ctg), -1, np.int32)
        n_groups, group_re = [], []
        for s, (_label, clusters) in enumerate(self.sets):
            n_groups.append(len(clusters))
            for n, cluster in enumerate(clusters):
                group[s, cluster] = n
                group_re.append(1 + int((self.re_sites[cluster] - 1).sum()))
        return group, np.array(n_groups, np.int32), np.array(group_re, np.int64), self.re_sites


def _partition(rng, n_ctg, n_groups, ungrouped=0.15):
    """clusters of a random assignment; some contigs stay ungrouped; no cluster is empty"""
    g = rng.integers(0, n_groups, n_ctg)
    g[rng.random(n_ctg) < ungrouped] = -1
    g[rng.permutation(n_ctg)[:n_groups]] = np.arange(n_groups)
    return [np.flatnonzero(g == k).tolist() for k in range(n_groups)]


def _random_keys(rng, n_ctg, n_keys):
    pairs = set()
    while len(pairs) < n_keys:
        a, b = rng.integers(0, n_ctg, 2).tolist()
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    pairs = sorted(pairs)
    order = rng.permutation(len(pairs))
    return np.array([pairs[k][0] for k in order]), np.array([pairs[k][1] for k in order])


def traps():
    """hand-built: ties, both denominators, ungrouped partners, contigs without keys, a single group"""
    #  0,1: group A (RE 3, 5)   2,3: group B (RE 7, 2)   4: group C (RE 11)   5,6: ungrouped   7: in no key   8: only ungrouped partners
    re_sites = [3, 5, 7, 2, 11, 4, 6, 9, 13, 2]
    keys = [(5, 6, 4),            # both ungrouped: contributes nothing
            (2, 5, 5), (0, 5, 5),  # contig 5 ties B (first) and A at 5 links: B wins, group_RE differ
            (0, 6, 9), (3, 6, 9), (4, 6, 9),   # contig 6: three-way tie A, B, C in that order
            (0, 1, 7),            # inside A: the own-group denominator for both
            (0, 2, 3), (1, 3, 2), (1, 2, 1),   # A <-> B
            (2, 4, 6), (0, 4, 6),  # contig 4 ties B (first) and A
            (6, 8, 2), (5, 8, 1),  # contig 8: only ungrouped partners -> not in the dict; contributes nothing to 5 and 6 either
            (3, 9, 8), (1, 9, 8), (4, 9, 8)]   # contig 9 (grouped with C in the second set): ties in another order
    fi, fj, cnt = zip(*keys)
    sets = [('1.1', [[0, 1], [2, 3], [4]]),
            ('1.2', [[2, 3], [4, 9], [0, 1]]),      # the same groups under other ids, contig 9 in a group of its own kind
            ('1.3', [[0, 1, 2, 3, 4, 9]])]          # len(group_RE_dict) == 1
    return Case('traps', [1000 * (k + 1) for k in range(10)], re_sites, fi, fj, cnt, sets)


def exact(sentinel_first):
    """a computed ratio of exactly 1000000.0 beside the int sentinel 1000000: (15625 / 16384) / ((1 / 2**20) / (2 - 1)).  X contigs (RE 1, ungrouped)
    link group A (one contig, RE 16384) with 15625 and group B (one contig, RE 2**20) with 1; S contigs link A only -> the sentinel."""
    A, B = 0, 1
    order = ['S', 'X', 'S', 'X'] if sentinel_first else ['X', 'S', 'X', 'S']
    re_sites = [16384, 2 ** 20] + [1] * len(order) + [5]
    keys = []
    for k, kind in enumerate(order):
        c = 2 + k
        keys.append((A, c, 15625 if kind == 'X' else 3 + k))
        if kind == 'X':
            keys.append((B, c, 1))
    fi, fj, cnt = zip(*keys)
    clusters = [[A], [B]]
    return Case('exact_s' if sentinel_first else 'exact_x', [500 + 100 * k for k in range(len(re_sites))], re_sites, fi, fj, cnt,
                [('2.0', clusters), ('2.1', [[B], [A]]), ('2.2', [[A, B]])])


def big():
    """sums above 2^32 (counts up to 2^40): arrays only, nobody pushes that many read pairs"""
    rng = np.random.default_rng(40)
    n = 24
    fi, fj = _random_keys(rng, n, 120)
    cnt = rng.integers(1, 2 ** 40, len(fi))
    cnt[:10] = 2 ** 40
    return Case('big', rng.integers(1000, 10 ** 6, n), rng.integers(1, 5000, n), fi, fj, cnt,
                [(str(x), _partition(rng, n, g)) for x, g in (('1.5', 3), ('2.5', 6), ('3.5', 2))], handle=False)


def ties():
    """small counts over groups of very different group_RE: most contigs have tied cells"""
    rng = np.random.default_rng(7)
    n = 80
    fi, fj = _random_keys(rng, n, 600)
    cnt = rng.integers(1, 3, len(fi))
    re_sites = rng.integers(1, 2000, n)
    return Case('ties', rng.integers(1000, 10 ** 6, n), re_sites, fi, fj, cnt, [(str(x), _partition(rng, n, g)) for x, g in (('1.1', 12), ('1.6', 25), ('2.4', 5))])


def magnitude():
    """quotients of one contig spanning many orders of magnitude (RE sites from 1 to 10^12): the order of the additions shows in the double"""
    rng = np.random.default_rng(11)
    n = 90
    fi, fj = _random_keys(rng, n, 1500)
    cnt = rng.integers(1, 60, len(fi))
    re_sites = (10.0 ** rng.uniform(0, 12, n)).astype(np.int64) + 1
    return Case('magnitude', rng.integers(1000, 10 ** 6, n), re_sites, fi, fj, cnt,
                [(str(x), _partition(rng, n, g, ungrouped=0.05)) for x, g in (('1.2', 30), ('1.8', 45), ('3.0', 18))])


def fixture_cases():
    return [traps(), exact(False), exact(True), big(), ties(), magnitude()]


def tied_rows(case, s):
    """contigs of set s whose two best cells tie in links while their groups differ in group_RE"""
    group, n_groups, group_re, _cre = case.engine_args()
    off = np.concatenate(([0], np.cumsum(n_groups)))
    gre = group_re[off[s]:off[s + 1]]
    cells = {}
    for a, b, v in zip(case.fi.tolist(), case.fj.tolist(), case.cnt.tolist()):
        for ctg, g in ((a, group[s, b]), (b, group[s, a])):
            if g != -1:
                cells.setdefault(ctg, {}).setdefault(int(g), 0)
                cells[ctg][int(g)] += v
    rows = []
    for ctg, inner in cells.items():
        ranked = sorted(inner.items(), key=lambda x: x[1], reverse=True)
        if len(ranked) > 1 and ranked[0][1] == ranked[1][1] and gre[ranked[0][0]] != gre[ranked[1][0]]:
            rows.append(ctg)
    return rows


# ------------------------------------------------------------------ shapes for the kernel tests (no fixture: the numpy engine is the reference)
def star(row_len, n_groups, seed, extra=0):
    """contig 0 linked to row_len others spread over n_groups groups (+ `extra` random keys among the others)"""
    rng = np.random.default_rng(seed)
    n = row_len + 1 + (1 if row_len == 0 else 0)
    fi, fj = np.zeros(row_len, np.int64), rng.permutation(np.arange(1, row_len + 1))
    if extra:
        ei, ej = _random_keys(rng, n - 1, extra)
        keep = np.ones(len(ei), bool)
        fi, fj = np.concatenate((fi, ei[keep] + 1)), np.concatenate((fj, ej[keep] + 1))
        lo, hi = np.minimum(fi, fj), np.maximum(fi, fj)
        _u, idx = np.unique(lo * n + hi, return_index=True)
        idx.sort()
        fi, fj = lo[idx], hi[idx]
    cnt = rng.integers(1, 50, len(fi))
    g = max(n_groups, 1)
    group = rng.integers(0, g, n).astype(np.int32)
    group[rng.random(n) < 0.1] = -1
    if row_len >= g:
        group[1:g + 1] = np.arange(g)                              # every group occurs among the hub's partners
    group_re = rng.integers(1, 10 ** 6, g)
    ctg_re = rng.integers(1, 1000, n)
    return fi.astype(np.int32), fj.astype(np.int32), cnt, group[None, :], np.array([g], np.int32), group_re, ctg_re


def random_case(n_ctg, n_keys, set_groups, seed, max_count=200):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n_ctg, n_keys), rng.integers(0, n_ctg, n_keys)
    ok = a != b
    lo, hi = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
    _u, idx = np.unique(lo * n_ctg + hi, return_index=True)
    idx.sort()
    swap = rng.random(len(idx)) < 0.5                              # arrays in dict order: both orientations of a key occur
    fi, fj = np.where(swap, hi[idx], lo[idx]), np.where(swap, lo[idx], hi[idx])
    cnt = rng.integers(1, max_count, len(fi))
    group = np.stack([rng.integers(-1, g, n_ctg) for g in set_groups]).astype(np.int32)
    group_re = np.concatenate([rng.integers(1, 10 ** 7, g) for g in set_groups])
    return fi.astype(np.int32), fj.astype(np.int32), cnt, group, np.array(set_groups, np.int32), group_re, rng.integers(1, 5000, n_ctg)
