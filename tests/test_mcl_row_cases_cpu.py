"""The numpy model of tests/mcl_row_cases.py against the oracle on every case of the module: bit for bit at inflation 2 and for the
convergence statistic, pattern + bound at inflations 1.5 and 3.0; the exactness proofs and the margins that the GPU comparisons
(tests/test_gpu_mcl_row_kernels.py) rest on; the closed form of the block-ones matrix.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import mcl_row_cases as rc


def same(x, y):
    return len(x) == len(y) and all(np.array_equal(np.asarray(u), np.asarray(v)) and np.asarray(u).dtype.kind == np.asarray(v).dtype.kind
                                    for u, v in zip(x, y))


@pytest.fixture(scope='module')
def mats():
    return dict(edge=rc.edge_matrix()[0], prune=rc.edge_matrix_prune()[0], counts=rc.edge_matrix_counts(), tall=rc.tall_matrix(),
                empty=rc.empty_matrix())


def test_edge_matrix_holds_what_it_says():
    (p, j, x), names = rc.edge_matrix()
    lens = np.diff(p)
    assert len(names) == len(lens) and lens[0] == 0 and lens[-1] == 0
    assert set(rc.EDGE_LENGTHS) <= set(lens.tolist()) and np.sum(lens == 0) >= 4
    assert sum(n.startswith('tie') for n in names) == 45 + 3
    s = rc.row_sums(p, x)
    assert np.all(s[lens > 0] == 1.0), 'every unit row is stochastic'
    q = rc.normalize(p, rc.inflate(x, 2.0))
    t = names.index('tie 0,1')
    row = q[p[t]:p[t + 1]]
    assert abs(row.max() - 0.447) < 1e-3 and abs(row.min() - 5.3e-4) < 1e-5
    for thr, kept in ((0.5, 1), (2.0 ** -6, 2), (1e-4, 200)):
        op, oj, _ = rc.prune(p, j, q, thr)
        assert op[t + 1] - op[t] == kept
        assert oj[op[t]] == j[p[t]]                                # the first of the two maxima
    t = names.index('tie 199,0,100')
    op, oj, _ = rc.prune(p, j, q, 0.5)
    assert op[t + 1] - op[t] == 1 and oj[op[t]] == j[p[t]]
    for n, kept in ((64, 64), (128, 1)):
        t = names.index('%d equal' % n)
        for r in rc.INFLATIONS:
            qr = rc.normalize(p, rc.inflate(x, r))
            assert np.all(qr[p[t]:p[t + 1]] == np.float32(1.0 / n))
            op = rc.prune(p, j, qr, 2.0 ** -6)[0]
            assert op[t + 1] - op[t] == kept
    for name, thr, kept in (('2 equal', 0.5, 2), ('32 equal', 0.5, 1), ('32 equal', 2.0 ** -6, 32), ('short tie 1,3', 0.5, 1)):
        t = names.index(name)                                      # the rows of the thread-per-row class of the fused expansion
        assert lens[t] <= 32
        op, oj, _ = rc.prune(p, j, q, thr)
        assert op[t + 1] - op[t] == kept and (kept > 1 or oj[op[t]] == j[p[t]:p[t + 1]][1 if name.startswith('short') else 0])
    (pp, pj, px), pnames = rc.edge_matrix_prune()
    t = pnames.index('threshold neighbours')
    op, oj, ox = rc.prune(pp, pj, px, 2.0 ** -6)
    assert np.array_equal(oj[op[t]:op[t + 1]], pj[pp[t]:pp[t + 1]][[0, 2, 3]])
    t = pnames.index('all zero')
    assert op[t + 1] - op[t] == 1 and oj[op[t]] == pj[pp[t]] and ox[op[t]] == 0.0
    tall = rc.tall_matrix()
    assert len(tall[0]) - 1 == 2 * 32768 + 5 and np.diff(tall[0]).min() == 1 and np.diff(tall[0]).max() == 3


@pytest.mark.parametrize('name', ['edge', 'prune', 'tall', 'empty'])
def test_exact_sums_where_bits_are_compared(mats, name):
    assert rc.exact_everywhere(mats[name]), name
    if name == 'edge':
        p, j, x = mats['counts']
        assert rc.exact_sums(p, x)


def test_exact_sums_tells_inexact_rows():
    p = np.array([0, 3], np.int32)
    assert rc.exact_sums(p, np.array([1.0, 2.0 ** -30, 2.0 ** -52], np.float32))
    assert not rc.exact_sums(p, np.array([1.0, 1.0, 2.0 ** -53], np.float32))
    assert not rc.exact_sums(p, np.array([2.0 ** 60, 1.0, 1.0], np.float32))
    assert rc.exact_sums(np.array([0, 0, 0], np.int32), np.zeros(0, np.float32))


@pytest.mark.parametrize('name', ['edge', 'tall'])
@pytest.mark.parametrize('infl', [1.5, 3.0])
def test_margins_of_the_bounded_comparisons(mats, name, infl):
    p, j, x = mats[name]
    near, gap = rc.margins(p, rc.normalize(p, rc.inflate(x, infl)))
    print('%s at %.1f: nearest value to a threshold %.3g relative, smallest gap of the two largest values %.3g' % (name, infl, near, gap))
    assert near > rc.MARGIN and gap > rc.MARGIN


def test_normalize_against_the_oracle(mats):
    for name in ('counts', 'edge', 'tall', 'empty'):
        p, j, x = mats[name]
        got = rc.normalize(p, x)
        assert got.dtype == np.float32 and np.array_equal(got, orc.normalize_l1(p, x)), name


@pytest.mark.parametrize('infl', rc.INFLATIONS)
def test_inflate_prune_against_the_oracle(mats, infl):
    worst = 0.0
    for name in ('edge', 'tall', 'empty'):
        p, j, x = mats[name]
        v = rc.inflate(x, infl)
        ov = orc.power(x, infl)
        q = rc.normalize(p, v)
        oq = orc.normalize_l1(p, ov)
        if infl == 2.0:
            assert np.array_equal(v, ov) and np.array_equal(q, oq), name
        else:
            assert rc.worst_rel(v, ov) <= rc.ULP and rc.worst_rel(q, oq) <= rc.INFLATE_RTOL, name
        for thr in rc.THRESHOLDS:
            got = rc.prune(p, j, q, thr)
            ref = orc.prune((p, j, oq), thr)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), '%s, pruning %r: pattern' % (name, thr)
            if infl == 2.0:
                assert same(got, ref), '%s, pruning %r' % (name, thr)
            else:
                w = rc.worst_rel(got[2], ref[2])
                worst = max(worst, w)
                assert w <= rc.PRUNE_RTOL, '%s, pruning %r: %.3g' % (name, thr, w)
    print('inflation %.1f: worst relative difference model vs oracle %.3g' % (infl, worst))


@pytest.mark.parametrize('thr', rc.THRESHOLDS)
def test_stand_alone_prune_against_the_oracle(mats, thr):
    for name in ('prune', 'tall', 'empty'):
        p, j, x = mats[name]
        assert same(rc.prune(p, j, x, thr), orc.prune((p, j, x), thr)), name


def test_convergence_against_the_oracle():
    pairs = rc.convergence_pairs()
    assert len(pairs) == 1 + 12 + 12 + 1
    for name, M, last, positive in pairs:
        got = rc.convergence(M, last, rc.CONV_N)
        ref = np.float32(orc.convergence_stat(M, last))
        assert got.dtype == np.float32 and got.tobytes() == ref.tobytes(), '%s: %r vs %r' % (name, got, ref)
        assert (got > np.float32(1e-8)) == positive, '%s: %r' % (name, got)
        if name == 'identical' or '2^-18' in name:
            assert got == 0.0, name
    moved = [rc.convergence(M, last, rc.CONV_N) for name, M, last, _ in pairs if '2^-17' in name]
    assert all(m == np.float32(np.float32(2.0 ** -17) - np.float32(1e-5) * np.float32(0.5)) for m in moved)


@pytest.mark.parametrize('infl', [2.0, 1.4])
def test_block_ones_closed_form(infl):
    L = rc.block_ones()
    n = len(L[0]) - 1
    assert n == 619 and orc.links_shift(L) > 0
    p = 2.0 ** -6
    want = rc.block_ones_iteration0(p)
    lens = np.diff(want[0])
    o = 0
    for m in rc.BLOCKS:
        assert np.all(lens[o:o + m] == (m if m <= 64 else 1))
        o += m
    pre = orc.expand_links(L)
    it0 = orc.mcl(pre, 2, infl, 1, p, spgemm_mode=1, fx_shift=52)
    assert same(it0[:3], want)
    assert same(orc.links_iteration0(L, np.arange(n), infl, p)[:3], want)
    assert same(orc.links_iteration0(L, np.arange(150, 500), infl, p)[:3], rc.block_ones_iteration0(p, 150, 500))
    res = orc.mcl(pre, 2, infl, 200, p, spgemm_mode=1, fx_shift=52)
    assert res[4], 'the loop did not converge'
    assert rc.clusters_of(*orc.interpret(res[:3])) == rc.block_ones_clusters()
