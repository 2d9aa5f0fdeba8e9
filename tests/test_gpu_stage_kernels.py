"""The four small stage kernels between the ingest and the clustering, each against the plain reference of
tests/stage_kernel_cases.py (bytes.count, Python integers / numpy float64, np.add.at / np.minimum.at, a dense stable argsort —
tied to the C oracle and to the paths below by tests/test_stage_kernel_cases_cpu.py), at the seams, strides and limits of the kernels.

hhx_count_re_sites (csrc/hhx_resites.hip; RS_BLOCK = 4096, RS_MAX_SITES = 64, RS_MAX_LEN = 32) — counts equal
  seams        b'T' * (5 * 4096 + 17) with GATC / GANTC / AAGCTT (border free: k_block_counts + k_segment_counts) and GCGC / AAAA
               (bordered: k_greedy_counts) planted at every start s - L .. s around each seam s = 4096 k, one sequence per (site, shift):
               a match that starts in one block and ends in the next; segments whose end point lies on every byte of s - L .. s + L and
               whose start is 0 or s - L .. s + 1, so both query points of k_segment_counts fall on x % 4096 == 0 (no partial recount,
               block_prefix[b] alone) and one byte to either side; the whole sequence, an empty segment at seq_len, the last three
               bytes, a segment shorter than the site; the same sequences cut to 5 * 4096 bytes with segments that end at seq_len, and
               a one-byte site, the only length whose query point is seq_len itself (block_prefix[n_blocks - 1], nothing recounted)
  many_sites   GANNNNTC: 256 sites of length 8, 255 border free -> four SiteSets of one length (64 + 64 + 64 + 63), GATCGATC alone to
               the greedy kernel, planted three times back to back across a seam; GATC,GANTC,AAGCTT,GCGC,A: four border-free lengths
               (one of a single byte) and one bordered site in one call; GATC,GATC: the duplicate counts twice
  strides      4097 * 4096 + 5 bytes: 4098 blocks, the second lap of k_block_counts (> 4096 blocks), with segments inside those blocks;
               16,402 query points, the second lap of k_segment_counts (> 16,384); 64 bordered sites x 16,385 segments, the second lap
               of k_greedy_counts (> 1,048,576 threads)
  refusals     a site of 33 bytes, an empty site, a segment past the end, a negative offset: RuntimeError from the argument check,
               before any launch; no segment at all and an empty sequence with empty segments: empty / zero counts

hhx_link_weights (csrc/hhx_weights.hip) — modes 1 and 2 and n_zero bit equal; mode 0 by the rule of
tests/test_gpu_pipeline.py::test_link_weights_a6 (rtol 4.5e-16, fewer than 1 % of the values not bit equal)
  stride       1,048,576 + 333 keys: the second lap of the grid-stride loop, all three modes, mode 2 with weights 1.0 / 0.5 / 0.3
  wide_totals  link totals in [2^31, 2^40]: the products pass 2^63, where an int64 product wraps (the oracle's does) and Python's
               integers do not — the case the mode-0 comment of the kernel is written for
  zeros        mode 2, weight 1.0 at 1, 63, 64, 65, 255, 257 and 100,003 keys: n_zero (wave sum + one atomic per wave) with a known
               count that is no multiple of a wave or a block; each also through the device-resident route (on_device = 1, raw device
               pointers), which must give the host route's bits

hhx_group_link_sums (csrc/hhx_weights.hip) — sums and first positions equal
  stride       1,048,576 + 77 keys, 3000 contigs, 7 groups, a fifth of the contigs ungrouped: the second lap
  one_cell     200,000 keys (0, 1) in one group: two cells take 200,000 atomics each, the sums pass 2^32, 2^33 and 2^47 (a 32-bit slip
               would show), first is 0 and 1
  edges        no key at all (zeros, first == -1 everywhere), n_groups == 1, every contig ungrouped, self keys (c, c)

hhx_rank_sums (csrc/hhx_filter.hip; RK_MAX_TOP = 64) on DeviceCSR.from_arrays — rank sums equal
  topn         n = 300, about 12 links per row, topN 0, 1, 2, 10, 63, 64 (the full LDS list; every list padded with unlinked
               fragments); 65 and -1 are refused
  fractional   float32(count / sqrt(total_i * total_j)), what --normalize_by_nlinks leaves: next to no ties, topN 10 and 64
  hub          n = 600, rows 0..3 of 599 entries (over nine strides of a wavefront in the selection and in rank_in_row), the others short,
               three distinct values: heavy ties, broken by index
  dense_small  n = 63, 64, 65, 129 with every off-diagonal entry stored, topN 64: at 63 and 64 the list takes every fragment, the row's own
               last; rows of 62, 63 (a wavefront less one), 64 (exactly one) and 128 (two strides) entries
  explicit_zeros  the hub pattern with a tenth of the values stored as 0.0: equals the matrix without them (rank_in_row: "x itself may be
               stored with 0"; the selection and the padding skip them)
  tiny         n = 1, 2, 7 below topN = 10; 50 fragments without a link
  Out of reach: the grid-stride lap of k_rank_sums needs n > 32,768 rows, where the dense reference takes 8.6 GB; negative stored
  values, which the kernel's own comment excludes and nothing upstream produces.

--topN 65: cluster.filter_fragments passes topN through, so the user sees the library's "hhx_rank_sums: topN must be in [0, 64]" as a
RuntimeError (after the link matrix was built, which is then freed) — a refusal, not a wrong result; pinned below on the device and in
tests/test_stage_kernel_cases_cpu.py on the host."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import stage_kernel_cases as skc


# ---------------------------------------------------------------------------------------------------------------- a5
@pytest.mark.parametrize('group', list(skc.RE_GROUPS))
def test_count_re_sites(group):
    from haphic_amd import _lib
    for c in skc.RE_GROUPS[group]():
        got = _lib.count_re_sites(c.seq, c.seg_off, c.seg_len, c.sites)
        bad = np.flatnonzero(got != c.want)
        assert bad.size == 0, (c, bad[:5], c.seg_off[bad[:5]], c.seg_len[bad[:5]], got[bad[:5]], c.want[bad[:5]])


def test_count_re_sites_refusals():
    from haphic_amd import _lib
    for name, seq, off, length, sites in skc.re_refusals():
        with pytest.raises(RuntimeError, match='hhx_count_re_sites'):
            _lib.count_re_sites(seq, off, length, sites)
    none = _lib.count_re_sites(b'GATC' * 25, [], [], [b'GATC'])
    assert none.shape == (0,) and none.dtype == np.int64
    assert _lib.count_re_sites(b'', [0, 0], [0, 0], [b'GATC', b'AAAA', b'A']).tolist() == [0, 0]
    assert _lib.count_re_sites(b'GATC' * 25, [0, 3], [100, 7], [b'GATC']).tolist() == [25, 1]          # the handle still works


# ---------------------------------------------------------------------------------------------------------------- a6
def _check_weights(c, v, nz):
    if c.mode == 0:
        differ = float((v != c.want).mean())
        with np.errstate(invalid='ignore'):
            print('%s: %.4f %% of the values not bit equal, largest relative error %.3g' % (c, 100 * differ, float(np.abs(v / c.want - 1).max())))
        np.testing.assert_allclose(v, c.want, rtol=4.5e-16, atol=0, err_msg=str(c))
        assert differ < 0.01, c
    else:
        assert np.array_equal(v, c.want), c
    assert nz == c.n_zero, c


@pytest.mark.parametrize('group', list(skc.WEIGHT_GROUPS))
def test_link_weights(group):
    import torch
    from haphic_amd import _lib
    for c in skc.WEIGHT_GROUPS[group]():
        v = c.value.copy()
        nz = _lib.link_weights(c.fi, c.fj, v, c.mode, c.n_frag, per_frag=c.per_frag, tag=c.tag, param=c.param)
        _check_weights(c, v, nz)
        if group == 'zeros':                              # the device-resident route: the same kernel on arrays that stay on the device
            di, dj, dv = (torch.from_numpy(a.copy()).cuda() for a in (c.fi, c.fj, c.value))
            torch.cuda.synchronize()
            nz2 = _lib.link_weights(None, None, None, c.mode, c.n_frag, tag=c.tag, param=c.param,
                                    device_ptrs=(len(c.value), di.data_ptr(), dj.data_ptr(), dv.data_ptr()))
            assert nz2 == nz and np.array_equal(dv.cpu().numpy(), v), c
            assert np.array_equal(di.cpu().numpy(), c.fi) and np.array_equal(dj.cpu().numpy(), c.fj), c


# ---------------------------------------------------------------------------------------------------------------- f3
@pytest.mark.parametrize('group', list(skc.GROUP_GROUPS))
def test_group_link_sums(group):
    from haphic_amd import _lib
    for c in skc.GROUP_GROUPS[group]():
        sums, first = _lib.group_link_sums(c.fi, c.fj, c.links, c.group, c.n_groups)
        assert sums.shape == first.shape == (len(c.group), c.n_groups), c
        assert np.array_equal(sums, c.want[0]), (c, np.argwhere(sums != c.want[0])[:5])
        assert np.array_equal(first, c.want[1]), (c, np.argwhere(first != c.want[1])[:5])


# ---------------------------------------------------------------------------------------------------------------- f1
@pytest.mark.parametrize('group', list(skc.RANK_GROUPS))
def test_rank_sums(group):
    from haphic_amd import _lib
    for c in skc.RANK_GROUPS[group]():
        m = _lib.DeviceCSR.from_arrays(*c.csr)
        got = _lib.rank_sums(m, c.topN)
        assert got.shape == (c.n,) and np.array_equal(got, c.want), (c, np.flatnonzero(got != c.want)[:8])
        if c.same_as is not None:
            m2 = _lib.DeviceCSR.from_arrays(*c.same_as.csr)
            assert np.array_equal(_lib.rank_sums(m2, c.same_as.topN), got), c
            m2.free()
        if group == 'topn' and c.topN == skc.RK_MAX_TOP:
            for bad in (skc.RK_MAX_TOP + 1, -1):
                with pytest.raises(RuntimeError, match=r'hhx_rank_sums: topN must be in \[0, 64\]'):
                    _lib.rank_sums(m, bad)
            assert np.array_equal(_lib.rank_sums(m, c.topN), c.want)              # the refusal left nothing behind
        m.free()


def test_filter_fragments_refuses_topn_65():
    """what the user of --topN 65 sees today: the library's message, raised out of cluster.filter_fragments"""
    from haphic_amd import cluster
    from tests.conftest import load_golden
    from tests.test_oracle_golden import _filter_inputs
    names, Nx_set, RE_site_dict, frag_link, flank = _filter_inputs(load_golden('filter.npz'))
    cluster.logger.setLevel('WARNING')
    with pytest.raises(RuntimeError, match=r'hhx_rank_sums: topN must be in \[0, 64\]'):
        cluster.filter_fragments(set(Nx_set), RE_site_dict, 5, frag_link, '0.2X', '1.9X', 65, '1.5X', 0, flank, {}, '1.5X', None)
    kept = cluster.filter_fragments(set(Nx_set), RE_site_dict, 5, frag_link, '0.2X', '1.9X', 64, '1.5X', 0, flank, {}, '1.5X', None)
    assert kept and kept <= Nx_set
