"""The numpy engine of the rescue / reassignment rounds (HapHiC_reassign.py run_reassignment :266-427) and of the group-pair sums of the
agglomerative step :494-508: a stand-in for haphic_amd._lib.Reassign with the same interface (include/haphic_hip.h, hhx_reassign_*), so that
the seams of haphic_amd/reassign.py run without a GPU (`patch_reassign(R, rounds=True, engine=NumpyReassign)`).  It is a plain sequential walk
over dense [contigs x groups] tables; tests/test_reassign_rounds_cpu.py pins it against the reference's own function
(tests/golden/reassign_rounds.npz), the GPU tests lean on it where the fixture has no case (2 100 groups).

Also the reader of the fixture (load_cases) and what the tests share to drive a whole job from its arrays (run_job)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'reassign_rounds.npz')

NONE = np.iinfo(np.int64).max                # stamp of a cell that never existed
# verdict codes (counts[] of a round: consistent, rescued, reassigned, not rescued); the not-rescued reasons are told apart for the fixture's
# coverage checks only
CONSISTENT, RESCUED, REASSIGNED, NR_RE, NR_LINKS, NR_AMBIGUOUS, NR_DENSITY, NR_RATIO = range(8)
COUNT_OF = (0, 1, 2, 3, 3, 3, 3, 3)


def python_sum(values, sum_mode):
    """sum() of a list of floats as CPython <= 3.11 (sum_mode 0) or >= 3.12 (1, Neumaier's compensation) computes it"""
    total = 0.0
    if sum_mode == 0:
        for x in values:
            total += x
        return total
    c = 0.0
    for x in values:
        t = total + x
        if abs(total) >= abs(x):
            c += (total - t) + x
        else:
            c += (x - t) + total
        total = t
    if c and math.isfinite(c):
        total += c
    return total


class NumpyReassign:
    def __init__(self, frag_i, frag_j, links, n_ctg, group, n_groups):
        self.fi, self.fj = np.asarray(frag_i, np.int64), np.asarray(frag_j, np.int64)
        self.links = np.asarray(links, np.int64)
        self.n_ctg, self.n_groups = int(n_ctg), int(n_groups)
        group = np.asarray(group, np.int64)
        self.sum = np.zeros((self.n_ctg, self.n_groups), np.int64)
        self.stamp = np.full((self.n_ctg, self.n_groups), NONE, np.int64)
        self.adj = [[] for _ in range(self.n_ctg)]
        for k, (a, b, v) in enumerate(zip(self.fi.tolist(), self.fj.tolist(), self.links.tolist())):
            for side, (x, y) in enumerate(((a, b), (b, a))):
                g = group[y]
                if g >= 0:
                    self.sum[x, g] += v
                    self.stamp[x, g] = min(self.stamp[x, g], 2 * k + side)
                self.adj[x].append((y, v))
        self.moves = 0
        self.rounds = 0
        self.events = set()                 # what the fixture's generator asserts the cases contain
        self.fell_to_zero = set()
        self.last_verdicts = None
        self.mode_sensitive = 0             # judgements whose list of other densities adds up differently under the two sum modes

    def cells(self):
        """(sums, first) as hhx_group_link_sums returns them: first == -1 where there is no cell"""
        return self.sum.copy(), np.where(self.stamp == NONE, -1, self.stamp)

    def judge(self, c, group, group_re, ctg_re, flags, min_links, min_link_density, min_density_ratio, ambiguous_cutoff, is_rescue_round, gfa,
              sum_mode):
        """-> (verdict, target group) of contig c against the state as it is"""
        row = self.sum[c]
        nz = np.flatnonzero(row)
        if not (flags[c] & 1) or nz.size == 0:
            return NR_RE, -1
        order = nz[np.lexsort((self.stamp[c, nz], -row[nz]))]
        max_group, max_links = int(order[0]), int(row[order[0]])
        second = int(row[order[1]]) if order.size > 1 else 0
        if order.size > 1 and second == max_links and (is_rescue_round or second / max_links < ambiguous_cutoff):
            self.events.add('tie_by_move' if max(self.stamp[c, order[0]], self.stamp[c, order[1]]) >= 2 * len(self.links) else 'tie_by_first')
        own = int(group[c])

        def density(g):
            return int(row[g]) / (int(group_re[g]) if g == own else int(group_re[g]) + int(ctg_re[c]) - 1)
        if max_links < min_links:
            return NR_LINKS, -1
        if not is_rescue_round and second / max_links >= ambiguous_cutoff:
            return NR_AMBIGUOUS, -1
        max_density = density(max_group)
        if max_density < min_link_density:
            return NR_DENSITY, -1
        quotients = [density(int(g)) for g in order[1:]]
        other = python_sum(quotients, sum_mode)
        if python_sum(quotients, 0) != python_sum(quotients, 1):
            self.mode_sensitive += 1
        if other:
            avg = other / (order.size - 1) if gfa else other / (self.n_groups - 1)
        else:
            avg = 1000000000
        ratio_ok = max_density / avg >= min_density_ratio
        if own < 0:
            return (RESCUED, max_group) if ratio_ok else (NR_RATIO, -1)
        if row[own] == max_links:
            return CONSISTENT, -1
        if not is_rescue_round and (flags[c] & 2) and ratio_ok:
            return REASSIGNED, max_group
        if not is_rescue_round and not (flags[c] & 2) and ratio_ok:
            self.events.add('too_long_to_move')
        return CONSISTENT, -1

    def round(self, group, group_re, ctg_re, order, flags, dismissed, min_links, min_link_density, min_density_ratio, ambiguous_cutoff,
              is_rescue_round, gfa, sum_mode):
        """one call of run_reassignment: group [n_ctg] (-1 = 'ungrouped') and group_re [n_groups] are changed in place -> counts[4]"""
        if sum_mode not in (0, 1):
            return None
        if dismissed is not None:
            d = np.flatnonzero(dismissed)
            group[np.isin(group, d)] = -1
            self.sum[:, d] = 0
        args = (min_links, min_link_density, min_density_ratio, ambiguous_cutoff, bool(is_rescue_round), bool(gfa), sum_mode)
        counts = np.zeros(4, np.int64)
        verdicts = np.zeros(len(order), np.int32)
        for n, c in enumerate(np.asarray(order).tolist()):
            verdict, target = self.judge(c, group, group_re, ctg_re, flags, *args)
            verdicts[n] = verdict
            counts[COUNT_OF[verdict]] += 1
            if target < 0:
                continue
            former = int(group[c])
            group[c] = target
            stamp = 2 * len(self.links) + self.moves
            self.moves += 1
            for y, v in self.adj[c]:
                if former >= 0:
                    self.sum[y, former] -= v
                    if self.sum[y, former] == 0:
                        self.fell_to_zero.add((y, former))
                if self.sum[y, target] == 0 and (y, target) in self.fell_to_zero:
                    self.events.add('zero_and_back')
                self.sum[y, target] += v
                if self.stamp[y, target] == NONE:
                    self.stamp[y, target] = stamp
            if former >= 0:
                group_re[former] -= ctg_re[c] - 1
            group_re[target] += ctg_re[c] - 1
        self.last_verdicts = verdicts
        self.rounds += 1
        return counts

    def pair_sums(self, member, group_of_ctg, n_groups):
        """:496-508: (sums, first) [n_groups, n_groups], cell (smaller, larger) group id; first = dict position of the first key, -1 = none"""
        member, g = np.asarray(member, bool), np.asarray(group_of_ctg, np.int64)
        sums = np.zeros((n_groups, n_groups), np.int64)
        first = np.full((n_groups, n_groups), NONE, np.int64)
        ga, gb = g[self.fi], g[self.fj]
        ok = member[self.fi] & member[self.fj] & (ga >= 0) & (gb >= 0) & (ga != gb)
        lo, hi = np.minimum(ga, gb)[ok], np.maximum(ga, gb)[ok]
        np.add.at(sums, (lo, hi), self.links[ok])
        np.minimum.at(first, (lo, hi), np.flatnonzero(ok))
        return sums, np.where(first == NONE, -1, first)

    def close(self):
        pass


def build_case(seed, n_groups, max_links, p_in, p_out, ungrouped):
    """a synthetic job of 300 contigs and about 5 000 keys with a planted grouping: (fi, fj, links, group, ctg_re, ctg_len)"""
    rng = np.random.default_rng(seed)
    n_ctg, n_keys = 300, 5000
    true = rng.integers(0, n_groups, n_ctg)
    iu, ju = np.triu_indices(n_ctg, 1)
    keep = rng.random(iu.size) < np.where(true[iu] == true[ju], p_in, p_out)
    iu, ju = iu[keep], ju[keep]
    pick = rng.permutation(iu.size)[:n_keys]
    fi, fj = iu[pick].astype(np.int32), ju[pick].astype(np.int32)
    links = np.where(true[fi] == true[fj], rng.integers(1, max_links + 1, fi.size), rng.integers(1, max(2, max_links // 3) + 1, fi.size)).astype(np.int64)
    group = true.copy()
    u = rng.random(n_ctg)
    group[u < ungrouped] = -1
    wrong = (u >= ungrouped) & (u < ungrouped + 0.2)
    group[wrong] = rng.integers(0, n_groups, int(wrong.sum()))
    group[n_ctg - 6:] = -1                                               # a few contigs that no key may name: not in any group either
    lonely = np.isin(fi, np.arange(n_ctg - 3, n_ctg)) | np.isin(fj, np.arange(n_ctg - 3, n_ctg))
    fi, fj, links = fi[~lonely], fj[~lonely], links[~lonely]
    sparse = np.arange(n_ctg - 20, n_ctg - 6)                           # contigs with one key or two: too few links to pass min_links
    hit = np.isin(fi, sparse) | np.isin(fj, sparse)
    drop = hit & (rng.random(fi.size) < 0.93)
    fi, fj, links = fi[~drop], fj[~drop], links[~drop]
    ctg_re = rng.integers(8, 400, n_ctg).astype(np.int64)
    ctg_len = (ctg_re * rng.integers(300, 500, n_ctg)).astype(np.int64)
    return fi, fj, links, group.astype(np.int32), ctg_re, ctg_len


def load_cases():
    """{name: {field: array}} of tests/golden/reassign_rounds.npz"""
    z = np.load(FIXTURE)
    cases = {}
    for key in z.files:
        name, field = key.split('/', 1)
        cases.setdefault(name, {})[field] = z[key]
    return cases


def case_flags(case):
    """the two flag bits the host computes: RE filter passed (RE_site_dict[ctg] - 1 >= min_RE_sites), short enough to be reassigned"""
    return (((case['ctg_re'] - 1 >= int(case['min_RE_sites'])).astype(np.uint8))
            | ((case['ctg_len'] <= float(case['max_ctg_len']) * 1000).astype(np.uint8) << 1))


def case_dismissed(case, group):
    """:304-316 on arrays: the mask of the groups a round above 1 dismisses (None: nothing to do)"""
    min_group_len = float(case['min_group_len'])
    if not min_group_len:
        return None
    n_groups = len(case['group_re0'])
    length = np.zeros(n_groups, np.int64)
    np.add.at(length, group[group >= 0], case['ctg_len'][group >= 0])
    present = np.zeros(n_groups, bool)
    present[group[group >= 0]] = True
    return (present & (length / 1000000 < min_group_len)).astype(np.uint8)


def run_job(case, engine, sum_mode=0, on_round=None):
    """the round loop of run() :865-880 on the arrays of a fixture case through `engine` (a NumpyReassign or a _lib.Reassign built from the case);
    -> [(nround, group, group_re, counts)] per call, to compare with the fixture's records"""
    group, group_re = case['group0'].astype(np.int32), case['group_re0'].astype(np.int64)
    flags = case_flags(case)
    out = []
    for nround in case['nrounds'].tolist():
        dismissed = case_dismissed(case, group) if nround > 1 else None
        counts = engine.round(group, group_re, case['ctg_re'], case['order'], flags, dismissed, float(case['min_links']),
                              float(case['min_link_density']), float(case['min_density_ratio']), float(case['ambiguous_cutoff']), nround == 0,
                              bool(case['gfa']), sum_mode)
        out.append((nround, group.copy(), group_re.copy(), np.asarray(counts).copy()))
        if on_round:
            on_round(nround)
    return out


# ------------------------------------------------------------------ a fixture case as the dicts run() :845-896 works on
def case_dicts(case):
    """the reference's containers for a case, built as tests/golden/make_golden_reassign_rounds.py builds them"""
    n_ctg, n_groups = len(case['group0']), len(case['group_re0'])
    names = ['c%03d' % k for k in range(n_ctg)]
    gnames = ['g%d' % g for g in range(n_groups)]
    group, ctg_re, ctg_len = case['group0'], case['ctg_re'], case['ctg_len']
    d = dict(names=names, gnames=gnames)
    d['full_link_dict'] = {(names[i], names[j]): int(v) for i, j, v in zip(case['fi'].tolist(), case['fj'].tolist(), case['links'].tolist())}
    d['fa_dict'] = {names[k]: [None, int(ctg_len[k]), int(ctg_re[k])] for k in range(n_ctg)}
    d['RE_site_dict'] = {names[k]: int(ctg_re[k]) for k in range(n_ctg)}
    d['sorted_ctg_list'] = [(names[k], int(ctg_len[k])) for k in case['order'].tolist()]
    d['ctg_group_dict'] = {names[k]: gnames[group[k]] for k in np.argsort(group, kind='stable').tolist() if group[k] >= 0}
    d['group_RE_dict'] = {g: int(v) for g, v in zip(gnames, case['group_re0'].tolist())}
    d['grouped_ctgs'] = set(d['ctg_group_dict'])
    for c in d['fa_dict']:                                              # add_ungrouped_ctgs :202-214
        d['ctg_group_dict'].setdefault(c, 'ungrouped')
    d['params'] = dict(gfa='x' if bool(case['gfa']) else None, max_ctg_len=float(case['max_ctg_len']), min_RE_sites=int(case['min_RE_sites']),
                       min_links=int(case['min_links']), min_link_density=float(case['min_link_density']),
                       min_density_ratio=float(case['min_density_ratio']), ambiguous_cutoff=float(case['ambiguous_cutoff']),
                       min_group_len=float(case['min_group_len']))
    return d


def call_round(R, d, tables, nround, whitelist=(), **override):
    """one call of R.run_reassignment on the dicts of case_dicts() as run() :866-869 spells it"""
    p = dict(d['params'], **override)
    return R.run_reassignment(d['sorted_ctg_list'], tables[0], d['ctg_group_dict'], d['full_link_dict'], tables[1], d['fa_dict'], d['RE_site_dict'],
                              p['gfa'], d['group_RE_dict'], p['max_ctg_len'], p['min_RE_sites'], p['min_links'], p['min_link_density'],
                              p['min_density_ratio'], p['ambiguous_cutoff'], p['min_group_len'], set(whitelist), nround)


def drive_rounds(R, d, after_call=None):
    """run() :855-880 through the names R holds: parse_link_dict, up to five rounds with the convergence test, the rescue round"""
    tables = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'], normalize_by_nlinks=False)
    last_round = None
    for n in range(5):
        call_round(R, d, tables, n + 1)
        if after_call:
            after_call(n + 1)
        if n > 0 and last_round == d['ctg_group_dict']:
            break
        last_round = d['ctg_group_dict'].copy()
    call_round(R, d, tables, 0)
    if after_call:
        after_call(0)
    return tables


def dense_dict_to_matrix(link_dict, frag_set, dense_matrix=True, add_self_loops=False):
    """HapHiC_cluster.dict_to_matrix :310-373 in its dense form, for a stand-in module (every member of frag_set is taken to have a link:
    the order of the others is the interpreter's set order)"""
    index = {}
    for a, b in link_dict:
        if a in frag_set and b in frag_set:
            index.setdefault(a, len(index))
            index.setdefault(b, len(index))
    assert len(index) == len(frag_set)
    m = np.zeros((len(frag_set), len(frag_set)), np.float32)
    for (a, b), v in link_dict.items():
        if a in index and b in index:
            m[index[a], index[b]] += np.float32(v)
            m[index[b], index[a]] += np.float32(v)
    return m, index


def compensation_quotients():
    """a list of positive quotients of integers whose plain and compensated sums differ"""
    rng = np.random.default_rng(5)
    return [int(a) / int(b) for a, b in zip(rng.integers(1, 10 ** 6, 400), rng.integers(1, 10 ** 4, 400))]


def check_pair_sums(case, sums, first):
    """(sums, first) of pair_sums on the case's agglomerative inputs against what the reference wrote, and against the keys counted one by one"""
    p = case['agg_pairs']
    lo, hi = np.minimum(p[:, 0], p[:, 1]), np.maximum(p[:, 0], p[:, 1])
    assert (sums[lo, hi] == p[:, 2]).all() and (first[lo, hi] == p[:, 3]).all()
    assert int((first >= 0).sum()) == len(p) and int(sums.sum()) == int(p[:, 2].sum())
    assert (np.diff(p[:, 3]) > 0).all()                                  # the fixture lists the pairs in dict order
    member, g = case['agg_member'].astype(bool), case['agg_group']
    counted = masked = 0
    for a, b, v in zip(case['fi'].tolist(), case['fj'].tolist(), case['links'].tolist()):
        if member[a] and member[b] and g[a] >= 0 and g[b] >= 0 and g[a] != g[b]:
            counted += v
        else:
            masked += 1
    assert counted == int(sums.sum()) and masked > 0
