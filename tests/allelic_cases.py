"""Cases and stand-ins for --remove_allelic_links on the device tables (haphic_amd/allelic.py, csrc/hhx_allelic.hip).

  cases()         small polyploid assemblies with allelic contacts, built with numpy only: what tests/golden/make_golden_allelic.py runs the
                  reference on (tests/golden/allelic.npz) and what the CPU and GPU tests run the mirror on
  Ingest          tests/oracle_lib.Ingest (the C oracle's ingest) plus the two engine methods of _lib.Ingest, restated in numpy from the
                  header's words: the stand-in of the CPU tests and the reference of the GPU tests
  library()       tests/oracle_lib with that Ingest: what `_lib` is bound to without a GPU
Test infrastructure only — the product has no such path."""
import types

import numpy as np

from haphic_amd import synth
from tests import oracle_lib

CAP = 4096                 # max_read_pairs the library serves (include/haphic_hip.h)


# ------------------------------------------------------------------ the engine
def modal_counts(crd_ptr, crd, ctg_len, full_i, full_j, nwindows, threshold):
    """(m, diag, anti) of cal_concordance_ratio :419-428 from flat coordinate lists [x0, y0, x1, y1, ...] per key (crd_ptr in values);
    keys with m < threshold get 0 / 0.  None when an evaluated key has window width 0."""
    m = (np.diff(crd_ptr) // 2).astype(np.int64)
    width = np.minimum(ctg_len[full_i], ctg_len[full_j]) // nwindows
    evaluated = m >= threshold
    if (evaluated & (width <= 0) & (m > 0)).any():
        return None
    key = np.repeat(np.arange(len(m)), m)
    x, y = crd[0::2].astype(np.int64), crd[1::2].astype(np.int64)
    w = np.maximum(width[key], 1)
    out = []
    for v in ((y - x) // w, (y + x) // w):                       # numpy's // floors, as Python's does
        order = np.lexsort((v, key))
        k, v = key[order], v[order]
        start = np.flatnonzero(np.r_[True, (k[1:] != k[:-1]) | (v[1:] != v[:-1])]) if len(k) else np.zeros(0, np.int64)
        run = np.diff(np.r_[start, len(k)])
        best = np.zeros(len(m), np.int64)
        np.maximum.at(best, k[start], run)
        out.append(np.where(evaluated, best, 0).astype(np.int32))
    return m.astype(np.int32), out[0], out[1]


class Ingest(oracle_lib.Ingest):
    UNSUPPORTED = 2
    first_row = None
    _dropped = False

    def fetch(self, max_read_pairs=0, want=None):
        if not self._dropped:
            return super().fetch(max_read_pairs, want)
        if max_read_pairs:
            raise RuntimeError('keys left the link tables (drop_links): the kept read pairs no longer match them')
        return self.out if want is None else {k: self.out[k] for k in want}

    def fetch_pairs(self, max_read_pairs, full_cnt):
        if self._dropped:
            raise RuntimeError('keys left the link tables (drop_links): the kept read pairs no longer match them')
        return super().fetch_pairs(max_read_pairs, full_cnt)

    def concordance_counts(self, max_read_pairs, nwindows, min_read_pairs=0):
        if max_read_pairs > CAP:
            return None
        pairs, self.pairs = self.pairs, True
        try:
            o = self.fetch(int(max_read_pairs))
        finally:
            self.pairs = pairs
        return modal_counts(o['crd_ptr'], o['crd'], self.t.ctg_len, o['full_i'], o['full_j'], int(nwindows), min(int(min_read_pairs), int(max_read_pairs)))

    def drop_links(self, full_drop, in_set):
        o = self.out if self.out is not None else self.fetch()
        full_drop, in_set = np.asarray(full_drop).astype(bool), np.asarray(in_set).astype(bool)
        assert full_drop.shape == (self.n_full,) and in_set.shape == (self.n_frag,)
        n_ctg = self.t.n_ctg
        gone_keys = o['full_i'][full_drop].astype(np.int64) * n_ctg + o['full_j'][full_drop]
        fi, fj = o['flank_i'].astype(np.int64), o['flank_j'].astype(np.int64)
        ci, cj = fi, fj
        if self.bins:                                                # fragment -> contig, the pair sorted by contig name (:1731)
            ci = np.searchsorted(self.t.ctg_frag0, fi, side='right') - 1
            cj = np.searchsorted(self.t.ctg_frag0, fj, side='right') - 1
            swap = self.t.ctg_rank[ci] > self.t.ctg_rank[cj]
            ci, cj = np.where(swap, cj, ci), np.where(swap, ci, cj)
        gone = np.isin(ci * n_ctg + cj, gone_keys) & (ci != cj) & in_set[fi] & in_set[fj]
        stay = ~gone
        inside = stay & in_set[fi] & in_set[fj]
        remaining = np.zeros(self.n_frag, np.uint8)
        first_row = np.full(self.n_frag, -1, np.int64)
        rows = np.flatnonzero(inside)
        seen = np.stack([fi[rows], fj[rows]], 1).ravel()
        at = np.stack([2 * rows, 2 * rows + 1], 1).ravel()
        frag, first = np.unique(seen, return_index=True)
        remaining[frag] = 1
        first_row[frag] = at[first]
        weights = self.fetch_flank_values()
        self.out = dict(o, full_i=o['full_i'][~full_drop], full_j=o['full_j'][~full_drop], full_cnt=o['full_cnt'][~full_drop],
                        ht_cnt=o['ht_cnt'][~full_drop], flank_i=o['flank_i'][stay], flank_j=o['flank_j'][stay], flank_cnt=o['flank_cnt'][stay])
        for k in ('clm_ptr', 'clm', 'crd_ptr', 'crd'):
            self.out.pop(k, None)
        if self.weights is not None:
            self.weights = weights[stay]
        self.n_full, self.n_flank = len(self.out['full_i']), len(self.out['flank_i'])
        self._dropped = True
        self.first_row = first_row
        return self.n_full, self.n_flank, gone.astype(np.uint8), remaining


def library():
    lib = types.ModuleType('allelic_oracle_lib')
    lib.__dict__.update({k: v for k, v in vars(oracle_lib).items() if not k.startswith('__')})
    lib.Ingest = Ingest
    return lib


# ------------------------------------------------------------------ the cases
def sample_pairs(genome, npairs, seed, cis=0.9, min_dist=1000):
    """synth.sample_pairs with numpy's generator (the fixture is tied to it, not to torch's): cis power-law pairs inside a chromosome"""
    rng = np.random.default_rng(seed)
    L, n = genome.chr_len, int(npairs)
    gstart = genome.chrom.astype(np.int64) * L + genome.start
    c1 = rng.integers(0, genome.nchrs, n)
    x1 = np.clip((rng.random(n) * L).astype(np.int64), 0, L - 1)
    is_cis = rng.random(n) < cis
    d = (min_dist * np.power(L / min_dist, rng.random(n))).astype(np.int64)
    sign = rng.integers(0, 2, n) * 2 - 1
    x2 = x1 + sign * d
    x2 = np.where((x2 < 0) | (x2 >= L), x1 - sign * d, x2)
    xr = np.clip((rng.random(n) * L).astype(np.int64), 0, L - 1)
    x2 = np.where((x2 < 0) | (x2 >= L), xr, x2)
    c2 = np.where(is_cis, c1, rng.integers(0, genome.nchrs, n))
    x2 = np.where(is_cis, x2, xr)

    def locate(c, x):
        gpos = c * L + x
        cid = np.searchsorted(gstart, gpos, side='right') - 1
        off = gpos - gstart[cid]
        return cid.astype(np.int32), np.where(genome.rev[cid], genome.length[cid] - 1 - off, off).astype(np.int32)
    return locate(c1, x1) + locate(c2, x2)


class Case:
    """one --remove_allelic_links job: the assembly, its fragments, the read pairs and the options"""

    def __init__(self, name, ploidy, nchrs, chr_len, mean_len, npairs, seed, bin_size=0, normalize=False, max_read_pairs=40, min_read_pairs=20,
                 cutoff=0.2, allelic=0.1, drop_frags=0.0):
        self.name, self.ploidy, self.bin_size, self.normalize = name, ploidy, bin_size, normalize
        base = synth.make_genome(nchrs, chr_len, mean_len, cv=0.3, min_len=8000, seed=seed)
        g = synth.make_polyploid(base, ploidy)
        id1, p1, id2, p2 = sample_pairs(g, npairs, seed + 1)
        id1, p1, id2, p2 = synth.add_allelic_pairs(g, base.n, ploidy, id1, p1, id2, p2, allelic, seed + 2)
        self.names, self.length = list(g.names), g.length.astype(np.int64)
        self.re_sites = g.re_sites
        # contigs of two bins and more are split (stat_fragments :188-296 decides this from N50 in a real run; any split is a valid input)
        self.split = [n for n, ln in zip(self.names, self.length) if bin_size and ln >= 2 * bin_size]
        if not self.split:
            keep = id1 != id2                                    # run() feeds the inter-contig generator then (:2865)
            id1, p1, id2, p2 = id1[keep], p1[keep], id2[keep], p2[keep]
        self.id1, self.pos1, self.id2, self.pos2 = id1, p1, id2, p2
        self.frag_len = {}
        split = set(self.split)
        for n, ln in zip(self.names, self.length.tolist()):
            if n in split:
                nb = -(-ln // bin_size)
                for k in range(nb):
                    self.frag_len['{}_bin{}'.format(n, k + 1)] = bin_size if k + 1 < nb else ln - (nb - 1) * bin_size
            else:
                self.frag_len[n] = ln
        self.frag_names = list(self.frag_len)
        rng = np.random.default_rng(seed + 3)
        self.filtered = [f for f in self.frag_names if rng.random() >= drop_frags]      # filtered_frags (filter_fragments :741)
        self.max_read_pairs, self.min_read_pairs, self.cutoff = max_read_pairs, min_read_pairs, cutoff
        self.checksum = int(id1.astype(np.int64).sum() + p1.astype(np.int64).sum() + id2.astype(np.int64).sum() + p2.astype(np.int64).sum())

    def fa_dict(self):
        return {n: [None, int(ln), int(r)] for n, ln, r in zip(self.names, self.length, self.re_sites)}

    def args(self):
        a = types.SimpleNamespace(flank=500, remove_allelic_links=self.ploidy, remove_concentrated_links=False, max_read_pairs=self.max_read_pairs,
                                  min_read_pairs=self.min_read_pairs, concordance_ratio_cutoff=self.cutoff, nwindows=50, ul=None,
                                  normalize_by_nlinks=self.normalize, skip_clustering=True)
        return a

    def alignments(self):
        nm = self.names
        return ((nm[a], nm[b], int(x), int(y)) for a, x, b, y in zip(self.id1.tolist(), self.pos1.tolist(), self.id2.tolist(), self.pos2.tolist()))

    def parse(self, mod):
        """parse_alignments* of `mod` (the reference module or haphic_amd.cluster): (full, flank, frag_link, coord, ctg_pair_to_frag or None)"""
        fa, args = self.fa_dict(), self.args()
        if self.split:
            full, flank, _ht, _clm, frag_link, coord, c2f = mod.parse_alignments(self.alignments(), fa, args, self.bin_size, dict(self.frag_len),
                                                                                  set(self.frag_names), set(self.split), 'int32', 'int32')
            return full, flank, frag_link, coord, c2f
        full, flank, _ht, _clm, frag_link, coord = mod.parse_alignments_for_ctgs(self.alignments(), fa, args, dict(self.frag_len), set(self.frag_names),
                                                                                 'int32', 'int32')
        return full, flank, frag_link, coord, None


def cases():
    return [
        Case('p2', 2, 2, 1_500_000, 40_000, 40_000, 7100),
        Case('p4', 4, 2, 1_000_000, 40_000, 60_000, 7200),
        Case('p4_bins', 4, 1, 1_600_000, 80_000, 60_000, 7300, bin_size=35_000, drop_frags=0.12),
        Case('p4_norm', 4, 1, 1_200_000, 40_000, 40_000, 7400, normalize=True, drop_frags=0.05),
    ]


def run_mirror(case, cluster, allelic, groups=None, engine=None):
    """the mirror on a case: parse_alignments* (whatever `_lib` cluster is bound to), normalize_by_nlinks where the case asks, then
    allelic.remove_allelic_HiC_links.  groups: frozen allele groups to use instead of allele_groups().  Returns a dict of what the fixture freezes."""
    full, flank, frag_link, coord, c2f = case.parse(cluster)
    if case.normalize:
        cluster.normalize_by_nlinks(flank, frag_link)
    pre_full, pre_flank = full.arrays()[:2], flank.arrays()[:2]
    session = full._session
    seen = {}
    real_groups = allelic.allele_groups

    def spy(inter_i, inter_j, inter_cnt, names, ploidy):
        seen['stage1'] = (np.array(inter_i), np.array(inter_j))
        return list(groups) if groups is not None else real_groups(inter_i, inter_j, inter_cnt, names, ploidy)
    allelic.allele_groups = spy
    try:
        remaining = allelic.remove_allelic_HiC_links(case.fa_dict(), coord, full, case.args(), flank, set(case.filtered), c2f, _engine=engine)
    finally:
        allelic.allele_groups = real_groups
    return dict(session=session, full=full, flank=flank, remaining=remaining, pre_full=pre_full, pre_flank=pre_flank, stage1=seen.get('stage1'))


def removed_mask(pre_i, pre_j, post_i, post_j, n):
    """which keys of the dict before (pre) are missing afterwards (post), in dict order"""
    return ~np.isin(pre_i.astype(np.int64) * n + pre_j, post_i.astype(np.int64) * n + post_j)
