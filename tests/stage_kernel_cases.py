"""Deterministic inputs for the four small stage kernels — RE-site counting (a5, csrc/hhx_resites.hip), link weights (a6) and
group link sums (f3, csrc/hhx_weights.hip), rank sums (f1, csrc/hhx_filter.hip) — placed on the seams, strides and limits of the
kernels, each with a plain reference of the operation the reference program performs: Python `bytes.count`, Python integers and
numpy float64, `np.add.at` / `np.minimum.at`, a dense stable argsort.  Neither the library nor the C oracle is used here;
tests/test_stage_kernel_cases_cpu.py ties the references to the oracle and asserts that every case reaches the path it is built
for, tests/test_gpu_stage_kernels.py runs the kernels on them.  Every builder is seeded and cached: a case is built once per process."""
import functools
from itertools import combinations

import numpy as np

RS_BLOCK, RS_MAX_SITES, RS_MAX_LEN = 4096, 64, 32         # csrc/hhx_resites.hip
GRID_CAP = 256 * 16                                       # blocks of the grid-stride kernels of hhx_resites.hip / hhx_weights.hip
THREADS_CAP = GRID_CAP * 256                              # ... and their threads: 1,048,576
RK_MAX_TOP = 64                                           # csrc/hhx_filter.hip


def sites_of(RE):
    from haphic_amd import cluster                        # host-only: parse_RE_sites' N expansion
    return cluster._sites_of(RE)


def has_border(site):
    """a proper prefix of the site equals a suffix: the site can overlap itself (hhx_resites.hip sends it to the greedy kernel)"""
    return any(site[:b] == site[len(site) - b:] for b in range(1, len(site)))


def count_re(seq, off, length, sites):
    """count_RE_sites :75-84 on the slice of every segment: sum of the non-overlapping bytes.count of every site"""
    out = np.zeros(len(off), np.int64)
    for k, (a, l) in enumerate(zip(np.asarray(off).tolist(), np.asarray(length).tolist())):
        piece = seq[a:a + l]
        out[k] = sum(piece.count(site) for site in sites)
    return out


class ReCase:
    def __init__(self, name, seq, RE, seg_off, seg_len, plants=()):
        self.name, self.seq, self.RE = name, seq, RE
        self.sites = sites_of(RE)
        self.seg_off, self.seg_len = np.asarray(seg_off, np.int64), np.asarray(seg_len, np.int64)
        self.plants = list(plants)                        # (seam, start) of every planted site
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = count_re(self.seq, self.seg_off, self.seg_len, self.sites)
            self._want.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------- a5: seams
SEAM_SITES = ('GATC', 'GANTC', 'AAGCTT', 'GCGC', 'AAAA')
SEAM_EXTRA_SITES = ('C',)               # a site of one byte: the only length at which a query point can be seq_len itself
SEAM_BLOCKS = 5
SEAM_LEN = SEAM_BLOCKS * RS_BLOCK + 17


def _seam_case(site, shift, cut):
    """b'T' everywhere; at every seam s = 4096 k the site (N expanded, another expansion per seam) is planted at s - L + shift.
    cut: the sequence ends on the last seam."""
    L = len(site)
    forms = [x for x in sites_of(site)]
    seq = bytearray(b'T' * SEAM_LEN)
    plants = []
    for k in range(1, SEAM_BLOCKS + 1):
        s = k * RS_BLOCK
        start = s - L + shift
        seq[start:start + L] = forms[(k + shift) % len(forms)]
        plants.append((s, start))
    seq = bytes(seq[:SEAM_BLOCKS * RS_BLOCK] if cut else seq)
    n = len(seq)
    segs = set()
    for k in range(1, SEAM_BLOCKS + 1):
        s = k * RS_BLOCK
        for end in range(s - L, s + L + 1):
            for off in [0] + list(range(s - L, s + 2)):
                if off <= end <= n:
                    segs.add((off, end - off))
    segs = sorted(segs)
    segs += [(0, n), (n, 0), (n - 3, 3), (RS_BLOCK - 1, L - 1)]           # whole, empty at the end, tail, shorter than the site
    if cut:
        segs += [(n - L - j, L + j) for j in range(3)] + [(n - RS_BLOCK, RS_BLOCK)]      # ending at seq_len == 5 * 4096
    off, length = zip(*segs)
    return ReCase('seams-%s-shift%d%s' % (site, shift, '-cut' if cut else ''), seq, site, off, length, plants)


@functools.lru_cache(maxsize=None)
def re_seams():
    return tuple(_seam_case(site, shift, cut) for site in SEAM_SITES + SEAM_EXTRA_SITES for shift in range(len(site) + 1) for cut in (False, True))


# ---------------------------------------------------------------------------------------------------------------- a5: many sites
MANY_RES = ('GANNNNTC', 'GATC,GANTC,AAGCTT,GCGC,A', 'GATC,GATC')


def _random_acgt(rng, n):
    return np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=None)
def re_many_sites():
    rng = np.random.default_rng(501)
    n = 40_000
    seq = bytearray(_random_acgt(rng, n))
    seq[12_286:12_286 + 24] = b'GATCGATC' * 3             # the bordered expansion of GANNNNTC, overlapping itself, over a seam
    seq = bytes(seq)
    off = rng.integers(0, n, 300)
    length = np.minimum(rng.integers(0, 6000, 300), n - off)
    off[:3], length[:3] = (0, 12_000, n), (n, 1_000, 0)
    return tuple(ReCase('many_sites-' + RE, seq, RE, off, length) for RE in MANY_RES)


# ---------------------------------------------------------------------------------------------------------------- a5: strides
STRIDE_SEQ_LEN = (GRID_CAP + 1) * RS_BLOCK + 5            # 4098 blocks: k_block_counts makes a second lap
STRIDE_TAIL = GRID_CAP * RS_BLOCK                         # first byte of the blocks counted on that lap


@functools.lru_cache(maxsize=None)
def _stride_seq():
    return _random_acgt(np.random.default_rng(502), STRIDE_SEQ_LEN)


@functools.lru_cache(maxsize=None)
def re_strides():
    seq = _stride_seq()
    n = len(seq)
    rng = np.random.default_rng(503)
    # (a) border free: 1 + 8200 segments = 16,402 query points > 16,384 (one lap of k_segment_counts); 200 of them lie in the blocks
    #     whose counts k_block_counts writes on its second lap
    la = rng.integers(0, 201, 8200)
    oa = rng.integers(0, n - 200, 8200)
    oa[-200:] = rng.integers(STRIDE_TAIL, n - 200, 200)
    a = ReCase('strides-GATC', seq, 'GATC', np.concatenate([[0], oa]), np.concatenate([[n], la]))
    # (b) 64 bordered sites x 16,385 segments = 1,048,640 (segment, site) pairs > 1,048,576 threads of k_greedy_counts
    lb = rng.integers(0, 65, THREADS_CAP // 64 + 1)
    ob = rng.integers(0, n - 64, lb.size)
    b = ReCase('strides-ANNNA', seq, 'ANNNA', ob, lb)
    return a, b


def re_cases():
    return re_seams() + re_many_sites() + re_strides()


def re_refusals():
    """(name, seq, seg_off, seg_len, sites): each must be refused with a RuntimeError before any device work"""
    seq = b'GATC' * 25
    return (('site_of_33_bytes', seq, [0], [100], [b'GATC', b'A' * (RS_MAX_LEN + 1)]),
            ('empty_site', seq, [0], [100], [b'GATC', b'']),
            ('segment_past_the_end', seq, [0, 98], [100, 3], [b'GATC']),
            ('negative_offset', seq, [-1], [4], [b'GATC']))


# ---------------------------------------------------------------------------------------------------------------- a6: link weights
class WeightCase:
    """mode 0: per_frag = link totals; 1: per_frag = lengths, param = 2 * flank in bp; 2: tag = haplotype, param = phasing weight.
    want: the float64 values of the reference's dict rewrite; n_zero: the entries it deletes (mode 2)"""

    def __init__(self, name, fi, fj, value, mode, n_frag, per_frag=None, tag=None, param=0.0):
        self.name, self.mode, self.n_frag, self.param = name, mode, n_frag, float(param)
        self.fi, self.fj = np.asarray(fi, np.int32), np.asarray(fj, np.int32)
        self.value = np.asarray(value, np.float64)
        self.per_frag = None if per_frag is None else np.asarray(per_frag, np.int64)
        self.tag = None if tag is None else np.asarray(tag, np.int32)
        for a in (self.fi, self.fj, self.value):
            a.setflags(write=False)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = weights_reference(self)
            self._want[0].setflags(write=False)
        return self._want[0]

    @property
    def n_zero(self):
        self.want
        return self._want[1]

    def __repr__(self):
        return self.name


def weights_reference(c):
    """normalize_by_nlinks :718-724, normalize_by_length :727-738, reduce_inter_hap_HiC_links :695-707 on arrays in dict order"""
    v = c.value
    if c.mode == 0:                                       # value / (links[i] * links[j]) ** 0.5, the product in Python integers
        la, lb = c.per_frag[c.fi].tolist(), c.per_frag[c.fj].tolist()
        root = np.array([float(int(a) * int(b)) ** 0.5 for a, b in zip(la, lb)], np.float64)
        return v / root, 0
    if c.mode == 1:                                       # value / ((fl_i / 1e6) * (fl_j / 1e6)), fl = min(len, 2 * flank)
        fa = np.minimum(c.per_frag[c.fi], int(c.param)).astype(np.float64)
        fb = np.minimum(c.per_frag[c.fj], int(c.param)).astype(np.float64)
        return v / ((fa / 1000000.0) * (fb / 1000000.0)), 0
    diff = c.tag[c.fi] != c.tag[c.fj]                     # value -= value * weight between haplotypes; zeros are deleted
    out = v.copy()
    out[diff] = v[diff] - v[diff] * np.float64(c.param)
    return out, int(((out == 0.0) & diff).sum())


@functools.lru_cache(maxsize=None)
def weights_stride():
    rng = np.random.default_rng(601)
    n, n_frag = THREADS_CAP + 333, 5000
    fi = rng.integers(0, n_frag, n)
    fj = rng.integers(0, n_frag, n)
    cnt = rng.integers(1, 2000, n).astype(np.float64)
    links = rng.integers(1, 3_000_000, n_frag)
    length = rng.integers(1_000, 3_000_000, n_frag)       # about a third below 2 * flank = 1 Mbp
    hap = rng.integers(0, 4, n_frag)
    return (WeightCase('stride-nlinks', fi, fj, cnt, 0, n_frag, per_frag=links),
            WeightCase('stride-length', fi, fj, cnt, 1, n_frag, per_frag=length, param=1_000_000),
            WeightCase('stride-hap-1.0', fi, fj, cnt, 2, n_frag, tag=hap, param=1.0),
            WeightCase('stride-hap-0.5', fi, fj, cnt, 2, n_frag, tag=hap, param=0.5),
            WeightCase('stride-hap-0.3', fi, fj, cnt, 2, n_frag, tag=hap, param=0.3))


@functools.lru_cache(maxsize=None)
def weights_wide_totals():
    """link totals in [2^31, 2^40]: the product of two passes 2^63 for most keys, where int64 wraps and Python's integers do not"""
    rng = np.random.default_rng(602)
    n, n_frag = 4096, 300
    links = rng.integers(2 ** 31, 2 ** 40, n_frag, endpoint=True)
    links[:4] = (2 ** 31, 2 ** 40, 2 ** 32 - 1, 2 ** 32 + 1)
    return (WeightCase('wide_totals', rng.integers(0, n_frag, n), rng.integers(0, n_frag, n), rng.integers(1, 10 ** 6, n).astype(np.float64),
                       0, n_frag, per_frag=links),)


ZERO_LENGTHS = (1, 63, 64, 65, 255, 257, 100_003)


def zeros_expected(n):
    """keys of weights_zeros(n) that join two haplotypes: all but those with k % 3 == 1"""
    return n - (n + 1) // 3


@functools.lru_cache(maxsize=None)
def weights_zeros():
    out = []
    n_frag = 60
    for n in ZERO_LENGTHS:
        rng = np.random.default_rng(610 + n)
        k = np.arange(n)
        fi = rng.integers(0, n_frag, n)
        delta = np.where(k % 3 == 1, 0, 1 + rng.integers(0, 2, n))        # haplotype = fragment % 3: delta 0 keeps it, 1 / 2 change it
        fj = (fi + delta + 3 * rng.integers(1, 19, n)) % n_frag
        value = np.where(rng.random(n) < 0.5, rng.integers(1, 500, n), rng.random(n) * 37.0)
        out.append(WeightCase('zeros-%d' % n, fi, fj, value, 2, n_frag, tag=np.arange(n_frag) % 3, param=1.0))
    return tuple(out)


def weight_cases():
    return weights_stride() + weights_wide_totals() + weights_zeros()


# ---------------------------------------------------------------------------------------------------------------- f3: group link sums
class GroupCase:
    def __init__(self, name, fi, fj, links, group, n_groups):
        self.name, self.n_groups = name, n_groups
        self.fi, self.fj = np.asarray(fi, np.int32), np.asarray(fj, np.int32)
        self.links, self.group = np.asarray(links, np.int64), np.asarray(group, np.int32)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = group_reference(self.fi, self.fj, self.links, self.group, self.n_groups)
            for a in self._want:
                a.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


def group_reference(fi, fj, links, group, n_groups):
    """parse_link_dict :217-263: sums[i][group[j]] += links, sums[j][group[i]] += links; first = the smallest dict position
    2 k (first side) / 2 k + 1 (second side) that reached a cell, -1 where none did"""
    n_ctg = len(group)
    fi, fj = fi.astype(np.int64), fj.astype(np.int64)
    sums = np.zeros(n_ctg * n_groups, np.int64)
    first = np.full(n_ctg * n_groups, np.iinfo(np.int64).max, np.int64)
    pos = np.arange(len(fi), dtype=np.int64)
    for side, (row, g) in enumerate(((fi, group[fj]), (fj, group[fi]))):
        ok = g >= 0
        cell = row[ok] * n_groups + g[ok]
        np.add.at(sums, cell, links[ok])
        np.minimum.at(first, cell, 2 * pos[ok] + side)
    first[first == np.iinfo(np.int64).max] = -1
    return sums.reshape(n_ctg, n_groups), first.reshape(n_ctg, n_groups)


@functools.lru_cache(maxsize=None)
def group_stride():
    rng = np.random.default_rng(701)
    n, n_ctg, n_groups = THREADS_CAP + 77, 3000, 7
    group = rng.integers(0, n_groups, n_ctg)
    group[rng.permutation(n_ctg)[:n_ctg // 5]] = -1
    return (GroupCase('stride', rng.integers(0, n_ctg, n), rng.integers(0, n_ctg, n), rng.integers(1, 1000, n), group, n_groups),)


@functools.lru_cache(maxsize=None)
def group_one_cell():
    rng = np.random.default_rng(702)
    n = 200_000
    return (GroupCase('one_cell', np.zeros(n, np.int32), np.ones(n, np.int32), rng.integers(2 ** 30, 2 ** 31, n), [0, 0], 1),)


@functools.lru_cache(maxsize=None)
def group_edges():
    rng = np.random.default_rng(703)
    n_ctg = 40
    fi, fj, links = rng.integers(0, n_ctg, 500), rng.integers(0, n_ctg, 500), rng.integers(1, 50, 500)
    group = rng.integers(-1, 3, n_ctg)
    selfish = GroupCase('self_key', np.concatenate([[7, 3], fi, [7]]), np.concatenate([[7, 9], fj, [7]]), np.concatenate([[11, 5], links, [13]]),
                        np.where(np.arange(n_ctg) == 7, 2, group), 3)
    return (GroupCase('no_keys', [], [], [], group, 3),
            GroupCase('one_group', fi, fj, links, np.minimum(group, 0), 1),
            GroupCase('all_ungrouped', fi, fj, links, np.full(n_ctg, -1), 3),
            selfish)


def group_cases():
    return group_stride() + group_one_cell() + group_edges()


# ---------------------------------------------------------------------------------------------------------------- f1: rank sums
class RankCase:
    def __init__(self, name, csr, topN, same_as=None):
        self.name, self.topN = name, topN
        self.csr = tuple(np.ascontiguousarray(a, t) for a, t in zip(csr, (np.int32, np.int32, np.float32)))
        self.n = len(self.csr[0]) - 1
        self.same_as = same_as                            # a matrix that must give the same result (explicit zeros removed)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = rank_reference(self.csr, self.topN)
            self._want.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


def rank_reference(csr, topN):
    """filter_fragments :866-892 on the dense matrix: every row sorted by links descending (stable: ties by index), the topN first
    of a row, and the sum over their pairs of the smaller of the two positions in each other's list"""
    ip, ix, dx = csr
    n = len(ip) - 1
    dense = np.zeros((n, n), np.float32)
    for r in range(n):
        dense[r, ix[ip[r]:ip[r + 1]]] = dx[ip[r]:ip[r + 1]]
    ranked = [np.argsort(-dense[r], kind='stable').tolist() for r in range(n)]
    out = np.zeros(n, np.int64)
    for f in range(n):
        out[f] = sum(min(ranked[a].index(b), ranked[b].index(a)) for a, b in combinations(ranked[f][:topN], 2))
    return out


def csr_from_keys(n, a, b, v):
    """the symmetric link matrix without self loops of the keys (a[k], b[k]) -> v[k], rows sorted by column"""
    rows, cols, vals = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([v, v]).astype(np.float32)
    order = np.lexsort((cols, rows))
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr).astype(np.int32), cols[order].astype(np.int32), vals[order]


def _random_keys(rng, n, per_row):
    """about per_row entries in every row: n * per_row / 2 distinct unordered pairs"""
    a, b = rng.integers(0, n, n * per_row // 2), rng.integers(0, n, n * per_row // 2)
    key = np.unique(np.minimum(a, b)[a != b] * n + np.maximum(a, b)[a != b])
    return key // n, key % n


@functools.lru_cache(maxsize=None)
def rank_topn():
    rng = np.random.default_rng(801)
    n = 300
    a, b = _random_keys(rng, n, 12)
    csr = csr_from_keys(n, a, b, rng.integers(1, 6, a.size))
    return tuple(RankCase('topn-%d' % t, csr, t) for t in (0, 1, 2, 10, 63, 64))


@functools.lru_cache(maxsize=None)
def rank_fractional():
    """what --normalize_by_nlinks leaves in the matrix: float32(count / sqrt(total_i * total_j))"""
    rng = np.random.default_rng(802)
    n = 400
    a, b = _random_keys(rng, n, 12)
    cnt = rng.integers(1, 400, a.size)
    tot = np.zeros(n, np.int64)
    np.add.at(tot, a, cnt)
    np.add.at(tot, b, cnt)
    csr = csr_from_keys(n, a, b, (cnt / np.sqrt((tot[a] * tot[b]).astype(np.float64))).astype(np.float32))
    return tuple(RankCase('fractional-%d' % t, csr, t) for t in (10, 64))


def _hub_keys():
    rng = np.random.default_rng(803)
    n = 600
    a, b = [], []
    for h in range(4):                                    # rows 0..3: linked to every other fragment
        a += [h] * (n - 1 - h)
        b += list(range(h + 1, n))
    for r in range(4, n):                                 # every other row: the four hubs and a few links of its own
        for c in rng.integers(4, n, rng.integers(1, 4)).tolist():
            if c != r:
                a.append(min(r, c))
                b.append(max(r, c))
    key = np.unique(np.array(a) * n + np.array(b))
    return n, key // n, key % n, rng


@functools.lru_cache(maxsize=None)
def rank_hub():
    n, a, b, rng = _hub_keys()
    return (RankCase('hub', csr_from_keys(n, a, b, rng.integers(1, 4, a.size)), 10),)


@functools.lru_cache(maxsize=None)
def rank_explicit_zeros():
    n, a, b, rng = _hub_keys()
    v = rng.integers(1, 4, a.size)
    zero = rng.random(a.size) < 0.1
    v[zero] = 0
    removed = RankCase('explicit_zeros-removed', csr_from_keys(n, a[~zero], b[~zero], v[~zero]), 10)
    return (RankCase('explicit_zeros', csr_from_keys(n, a, b, v), 10, same_as=removed),)


@functools.lru_cache(maxsize=None)
def rank_dense_small():
    rng = np.random.default_rng(804)
    out = []
    for n in (63, 64, 65, 129):
        a, b = np.triu_indices(n, 1)
        out.append(RankCase('dense_small-%d' % n, csr_from_keys(n, a, b, rng.integers(1, 5, a.size)), RK_MAX_TOP))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rank_tiny():
    rng = np.random.default_rng(805)
    out = [RankCase('tiny-1', csr_from_keys(1, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)), 10),
           RankCase('tiny-2', csr_from_keys(2, np.array([0]), np.array([1]), np.array([2.0])), 10)]
    a, b = _random_keys(rng, 7, 3)
    out.append(RankCase('tiny-7', csr_from_keys(7, a, b, rng.integers(1, 4, a.size)), 10))
    out.append(RankCase('empty-50', csr_from_keys(50, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)), 10))
    return tuple(out)


def rank_cases():
    return rank_topn() + rank_fractional() + rank_hub() + rank_explicit_zeros() + rank_dense_small() + rank_tiny()


# case groups by name, built on first use (the GPU tests are parametrised over the names alone)
RE_GROUPS = {'seams': re_seams, 'many_sites': re_many_sites, 'strides': re_strides}
WEIGHT_GROUPS = {'stride': weights_stride, 'wide_totals': weights_wide_totals, 'zeros': weights_zeros}
GROUP_GROUPS = {'stride': group_stride, 'one_cell': group_one_cell, 'edges': group_edges}
RANK_GROUPS = {'topn': rank_topn, 'fractional': rank_fractional, 'hub': rank_hub, 'dense_small': rank_dense_small,
               'explicit_zeros': rank_explicit_zeros, 'tiny': rank_tiny}
