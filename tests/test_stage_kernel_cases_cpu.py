"""The cases of tests/stage_kernel_cases.py are themselves checked here, without a GPU: every plain reference equals the C oracle
(oracle.count_re_sites, oracle.rank_sums always; oracle.group_link_sums, a Python loop, on the small cases and on a 20,000-key prefix
of the large ones; oracle.link_weights except where its int64 product wraps, which is asserted to happen), and every case still
reaches the kernel path it was built for — a generator that quietly stops doing so fails here, not on the GPU.

What a user sees for --topN 65 is pinned at the end: hhx_rank_sums holds its top list in LDS (RK_MAX_TOP = 64) and refuses more;
cluster.filter_fragments passes --topN through unchanged, so the run ends with the library's own
"hhx_rank_sums: topN must be in [0, 64]" as a RuntimeError, the link matrix freed — no silent wrong result.  The reference itself has
no such limit (INTEGRATION.md lists it among the narrower ones)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import stage_kernel_cases as skc


# ---------------------------------------------------------------------------------------------------------------- a5
def test_re_references_equal_the_oracle():
    for c in skc.re_cases():
        assert np.array_equal(c.want, orc.count_re_sites(c.seq, c.seg_off, c.seg_len, c.sites)), c
        assert (c.seg_off >= 0).all() and (c.seg_len >= 0).all() and (c.seg_off + c.seg_len <= len(c.seq)).all(), c


def test_re_seams_reach_the_seams():
    cases = skc.re_seams()
    assert len(cases) == 2 * sum(len(s) + 1 for s in skc.SEAM_SITES + skc.SEAM_EXTRA_SITES)
    assert [skc.has_border(s.encode()) for s in skc.SEAM_SITES] == [False, False, False, True, True]
    for site in skc.SEAM_SITES:
        L = len(site)
        mine = [c for c in cases if c.RE == site and not c.name.endswith('-cut')]
        assert len(mine) == L + 1 and all(len(c.seq) == 5 * 4096 + 17 for c in mine)
        assert sorted(start - s for c in mine for s, start in c.plants if s == 4096) == list(range(-L, 1))      # starts s - L .. s
        for k in range(1, 6):
            s, hit = 4096 * k, 0
            for c in mine:
                (start,) = [p for seam, p in c.plants if seam == s]
                assert c.seq[start:start + L] in c.sites
                if s - L + 1 <= start <= s - 1:           # the match starts in one block and ends in the next
                    covers = (c.seg_off <= start) & (c.seg_off + c.seg_len >= start + L) & (c.seg_off > 0)
                    assert covers.any() and (c.want[covers] > 0).all()
                    hit += 1
            assert hit == L - 1, (site, s)
        for c in mine:
            assert ((c.seg_off + c.seg_len - L + 1) % 4096 == 0).any() and ((c.seg_off % 4096 == 0) & (c.seg_off > 0)).any(), c
            assert int(c.want[(c.seg_off == 0) & (c.seg_len == len(c.seq))][0]) == 5                            # one plant per seam, nothing else
            assert (c.seg_len < L).any() and ((c.seg_off == len(c.seq)) & (c.seg_len == 0)).any()
    for c in cases:
        if c.name.endswith('-cut'):
            assert len(c.seq) == 5 * 4096 and ((c.seg_off + c.seg_len == len(c.seq)) & (c.seg_len >= len(c.sites[0]))).sum() >= 4, c
    # a query point x == seq_len on the last seam needs a site of one byte
    one = [c for c in cases if c.RE in skc.SEAM_EXTRA_SITES and c.name.endswith('-cut')]
    assert one and all(((c.seg_off + c.seg_len - 1 + 1 == len(c.seq)) & (c.seg_len > 0)).any() for c in one)


def test_re_many_sites_fill_more_than_one_site_set():
    sites = skc.sites_of('GANNNNTC')
    assert len(sites) == 256 and len(set(sites)) == 256 and all(len(s) == 8 for s in sites)
    bordered = [s for s in sites if skc.has_border(s)]
    assert bordered == [b'GATCGATC'] and len(sites) - len(bordered) > skc.RS_MAX_SITES
    a, b, c = skc.re_many_sites()
    assert len(a.seq) == 40_000 and len(a.seg_off) == 300 and a.seq is b.seq is c.seq
    assert a.seq[12_286:12_310] == b'GATCGATC' * 3 and a.want[1] >= 3            # the bordered site, greedy: 3, not the 5 overlapping starts
    free = [s for s in b.sites if not skc.has_border(s)]
    assert sorted({len(s) for s in free}) == [1, 4, 5, 6] and [s for s in b.sites if skc.has_border(s)] == [b'GCGC']
    assert c.sites == [b'GATC', b'GATC'] and c.want.sum() > 0 and (c.want % 2 == 0).all()          # a duplicate counts twice
    for x in (a, b, c):
        assert (x.want > 0).sum() > 200 and (x.seg_len == 0).any(), x


def test_re_strides_pass_one_lap_of_every_grid():
    a, b = skc.re_strides()
    assert len(a.seq) == 4097 * 4096 + 5 and a.seq is b.seq
    assert len(a.seq) // 4096 + 1 > skc.GRID_CAP                                  # k_block_counts: blocks per lap
    assert 2 * len(a.seg_off) > 4 * skc.GRID_CAP == 16384                         # k_segment_counts: one wave per query point
    assert len(b.seg_off) * 64 > skc.THREADS_CAP == 1048576                       # k_greedy_counts: one thread per (segment, site)
    assert len(a.sites) == 1 and not skc.has_border(a.sites[0])
    assert len(b.sites) == 64 and all(skc.has_border(s) for s in b.sites)
    tail = a.seg_off >= 4096 * 4096
    assert tail.sum() >= 200 and (a.want[tail] > 0).sum() >= 20                        # counts that rest on the second lap's blocks
    assert a.want[0] == a.seq.count(b'GATC') > 60_000
    late = np.arange(len(b.seg_off)) >= skc.THREADS_CAP // 64                     # the segment of the second lap
    assert late.sum() == 1 and b.seg_len[late][0] >= 5 and (b.want > 0).mean() > 0.3
    assert a.seg_len[1:].max() == 200 and a.seg_len.min() == 0 and b.seg_len.max() == 64 and b.seg_len.min() == 0


def test_re_refusals_are_out_of_domain():
    for name, seq, off, length, sites in skc.re_refusals():
        bad_site = any(len(s) == 0 or len(s) > skc.RS_MAX_LEN for s in sites)
        bad_seg = any(a < 0 or l < 0 or a + l > len(seq) for a, l in zip(off, length))
        assert bad_site != bad_seg, name                                          # exactly one reason each


# ---------------------------------------------------------------------------------------------------------------- a6
def test_weight_references_equal_the_oracle():
    for c in skc.weight_cases():
        if c.name == 'wide_totals':
            continue
        got = orc.link_weights(c.fi, c.fj, c.value, c.mode, per_frag=c.per_frag, tag=c.tag, param=c.param)
        assert np.array_equal(got, c.want), c
        assert np.isfinite(c.want).all() and (c.want >= 0).all()


def test_weight_cases_reach_their_paths():
    stride = skc.weights_stride()
    assert [c.mode for c in stride] == [0, 1, 2, 2, 2] and [c.param for c in stride[2:]] == [1.0, 0.5, 0.3]
    assert all(len(c.value) == 1048576 + 333 > skc.THREADS_CAP and c.n_frag == 5000 for c in stride)
    below = stride[1].per_frag < stride[1].param
    assert 0.2 < below.mean() < 0.5                                               # both sides of min(len, 2 * flank)
    differ = int((stride[2].tag[stride[2].fi] != stride[2].tag[stride[2].fj]).sum())
    assert stride[2].n_zero == differ > 0 and stride[3].n_zero == stride[4].n_zero == 0
    assert np.array_equal(stride[3].want != stride[3].value, stride[2].want == 0)
    # wide totals: the oracle's int64 product wraps, Python's does not
    (w,) = skc.weights_wide_totals()
    assert len(w.value) == 4096 and w.per_frag.min() == 2 ** 31 and w.per_frag.max() == 2 ** 40
    exact = [int(a) * int(b) for a, b in zip(w.per_frag[w.fi].tolist(), w.per_frag[w.fj].tolist())]
    with np.errstate(all='ignore'):
        wrapped = (w.per_frag[w.fi] * w.per_frag[w.fj]).tolist()
        theirs = np.asarray(orc.link_weights(w.fi, w.fj, w.value, 0, per_frag=w.per_frag))
    wraps = np.array([x != y for x, y in zip(exact, wrapped)])
    assert wraps.sum() > 1000 and sum(x >= 2 ** 63 for x in exact) == wraps.sum()
    assert (theirs[wraps] != w.want[wraps]).all() and np.array_equal(theirs[~wraps].real, w.want[~wraps])       # the case bites
    assert np.isfinite(w.want).all() and (w.want > 0).all()
    # zeros
    zeros = skc.weights_zeros()
    assert tuple(len(c.value) for c in zeros) == skc.ZERO_LENGTHS == (1, 63, 64, 65, 255, 257, 100_003)
    for c in zeros:
        n = len(c.value)
        assert c.n_zero == skc.zeros_expected(n) == int((c.tag[c.fi] != c.tag[c.fj]).sum()) > 0, c
        assert n < 63 or (c.n_zero % 64 and c.n_zero % 256), c
        assert (c.value > 0).all() and (c.fi != c.fj).all() and int((c.want == 0).sum()) == c.n_zero


# ---------------------------------------------------------------------------------------------------------------- f3
def test_group_references_equal_the_oracle():
    for c in skc.group_cases():
        k = min(len(c.fi), 20_000)
        want = c.want if k == len(c.fi) else skc.group_reference(c.fi[:k], c.fj[:k], c.links[:k], c.group, c.n_groups)
        sums, first = orc.group_link_sums(c.fi[:k], c.fj[:k], c.links[:k], c.group, c.n_groups)
        assert np.array_equal(sums, want[0]) and np.array_equal(first, want[1]), c


def test_group_cases_reach_their_paths():
    (s,) = skc.group_stride()
    assert len(s.fi) == 1048576 + 77 > skc.THREADS_CAP and len(s.group) == 3000 and s.n_groups == 7
    assert (s.group < 0).sum() == 600 and sorted(set(s.group.tolist())) == list(range(-1, 7))
    assert (s.want[1] >= 2 * skc.THREADS_CAP).sum() == 0 and (s.want[1] >= 0).all()       # every cell is reached early: ...
    late = np.arange(len(s.fi)) >= skc.THREADS_CAP
    assert (s.group[s.fj[late]] >= 0).sum() > 40                                          # ... the second lap shows in the sums
    (o,) = skc.group_one_cell()
    assert len(o.fi) == 200_000 and o.want[0].shape == (2, 1)
    assert o.want[0][0, 0] == o.want[0][1, 0] == int(o.links.sum()) > 2 ** 33 and o.links.min() >= 2 ** 30 and o.links.max() < 2 ** 31
    assert o.want[1].tolist() == [[0], [1]]
    edges = {c.name: c for c in skc.group_edges()}
    assert set(edges) == {'no_keys', 'one_group', 'all_ungrouped', 'self_key'}
    e = edges['no_keys']
    assert len(e.fi) == 0 and e.want[0].size == 120 and not e.want[0].any() and (e.want[1] == -1).all()
    assert edges['one_group'].n_groups == 1 and edges['one_group'].want[0].any() and (edges['one_group'].group < 0).any()
    assert not edges['all_ungrouped'].want[0].any() and (edges['all_ungrouped'].want[1] == -1).all()
    e = edges['self_key']
    assert (e.fi[0], e.fj[0], e.fi[-1], e.fj[-1]) == (7, 7, 7, 7) and e.group[7] == 2
    assert e.want[1][7, 2] == 0 and e.want[0][7, 2] >= 2 * (11 + 13)                       # a self key adds twice; its first side comes first


# ---------------------------------------------------------------------------------------------------------------- f1
def test_rank_references_equal_the_oracle():
    for c in skc.rank_cases():
        assert np.array_equal(c.want, orc.rank_sums(c.csr, c.topN)), c
        if c.same_as is not None:
            assert np.array_equal(c.want, c.same_as.want), c
            assert np.array_equal(c.same_as.want, orc.rank_sums(c.same_as.csr, c.same_as.topN)), c


def _rows(c):
    return np.diff(c.csr[0])


def test_rank_cases_reach_their_paths():
    topn = skc.rank_topn()
    assert [c.topN for c in topn] == [0, 1, 2, 10, 63, 64] and all(c.n == 300 for c in topn) and 10 < _rows(topn[0]).mean() < 13
    assert not topn[0].want.any() and not topn[1].want.any() and topn[2].want.any()
    assert (_rows(topn[0]) < 63).all()                                            # every list of 63 / 64 is padded with unlinked fragments
    frac = skc.rank_fractional()
    assert [c.topN for c in frac] == [10, 64] and frac[0].n == 400
    ip, ix, dx = frac[0].csr
    assert dx.dtype == np.float32 and (dx != np.round(dx)).all() and (dx > 0).all()
    tied = sum(int(e - b - len(set(dx[b:e].tolist()))) for b, e in zip(ip[:-1], ip[1:]))
    assert tied < 0.01 * len(dx)
    (hub,) = skc.rank_hub()
    assert hub.n == 600 and _rows(hub)[:4].tolist() == [599] * 4 and 599 > 9 * 64          # over nine strides of a wavefront
    assert _rows(hub)[4:].max() < 20 and _rows(hub)[4:].min() >= 5 and len(set(hub.csr[2].tolist())) == 3
    (z,) = skc.rank_explicit_zeros()
    stored_zero = z.csr[2] == 0
    assert 0.07 < stored_zero.mean() < 0.13 and z.same_as.csr[2].all() and len(z.same_as.csr[2]) == int((~stored_zero).sum())
    assert stored_zero[:z.csr[0][4]].any() and stored_zero[z.csr[0][4]:].any()    # in hub rows and in short rows
    dense = skc.rank_dense_small()
    assert [c.n for c in dense] == [63, 64, 65, 129] and all(c.topN == 64 == skc.RK_MAX_TOP for c in dense)
    assert all((_rows(c) == c.n - 1).all() for c in dense)
    tiny = skc.rank_tiny()
    assert [(c.n, c.topN, len(c.csr[1])) for c in tiny][:2] == [(1, 10, 0), (2, 10, 2)] and [c.n for c in tiny] == [1, 2, 7, 50]
    assert len(tiny[3].csr[1]) == 0 and tiny[3].want.tolist() == [sum(min(a, b) for a in range(10) for b in range(a + 1, 10))] * 50


def test_symmetric_rank_matrices():
    import scipy.sparse as sp
    for c in skc.rank_cases():
        ip, ix, dx = c.csr
        m = sp.csr_matrix((dx, ix, ip), shape=(c.n, c.n))
        assert (m != m.T).nnz == 0 and not m.diagonal().any(), c
        rows = np.repeat(np.arange(c.n), np.diff(ip))
        assert (np.diff(ix)[np.diff(rows) == 0] > 0).all(), c                     # sorted by column, no duplicates


# ---------------------------------------------------------------------------------------------------------------- --topN 65
def test_topn_65_ends_with_the_library_message(monkeypatch):
    from haphic_amd import cluster, _lib
    from tests.conftest import load_golden
    from tests.test_oracle_golden import _filter_inputs
    names, Nx_set, RE_site_dict, frag_link, flank = _filter_inputs(load_golden('filter.npz'))
    seen = {'freed': 0}

    class Matrix:
        def free(self):
            seen['freed'] += 1

    def rank_sums(m, topN):
        """the argument check of hhx_rank_sums (csrc/hhx_filter.hip), which returns before any launch"""
        seen['topN'] = topN
        if topN < 0 or topN > skc.RK_MAX_TOP:
            raise RuntimeError('libhaphic_hip: hhx_rank_sums: topN must be in [0, %d]' % skc.RK_MAX_TOP)
        return np.zeros(len(names), np.int64)

    monkeypatch.setattr(cluster, 'dict_to_matrix', lambda *a, **k: (Matrix(), {n: i for i, n in enumerate(names)}))
    monkeypatch.setattr(_lib, 'rank_sums', rank_sums)
    cluster.logger.setLevel('WARNING')
    with pytest.raises(RuntimeError, match=r'topN must be in \[0, 64\]'):
        cluster.filter_fragments(set(Nx_set), RE_site_dict, 5, frag_link, '0.2X', '1.9X', 65, '1.5X', 0, flank, {}, '1.5X', None)
    assert seen == {'freed': 1, 'topN': 65}                                       # passed through unchanged, the matrix released
    cluster.filter_fragments(set(Nx_set), RE_site_dict, 5, frag_link, '0.2X', '1.9X', 64, '1.5X', 0, flank, {}, '1.5X', None)
    assert seen == {'freed': 2, 'topN': 64}
