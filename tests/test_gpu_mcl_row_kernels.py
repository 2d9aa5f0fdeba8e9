"""The row epilogue of an MCL iteration in its three implementations — the CSR row kernels of hhx_mcl.hip, the fused epilogues of
hhx_expand.hip (tiny, hash, compact and window classes, the class stream) and the dense-row epilogue — against the numpy float64 model
of tests/mcl_row_cases.py, on rows that take the branches stochastic random data never takes: a maximum below the threshold
(restored), two- and three-way tied maxima at lane, stride and wave seams (the first one is restored), a value equal to the threshold
(kept), empty and all-zero rows, lengths around 64 / 256 / 4096, three passes of the row grid, convergence operands of different
patterns.  Byte equality at inflation 2 (every row sum is exact in any order: tests/test_mcl_row_cases_cpu.py proves it); identical
pattern and 3 * 2^-23 / 6 * 2^-23 relative at the other inflations.
Run on the GPU box:  python -m pytest tests/test_gpu_mcl_row_kernels.py -m gpu -s"""
import numpy as np
import pytest

from haphic_amd import _lib
from tests import expand_classes as ec
from tests import mcl_row_cases as rc

pytestmark = pytest.mark.gpu

KNOBS = ('hash_max', 'links_sym', 'links_integer')
COUNTERS = ('expand_rows_window', 'expand_rows_compact', 'expand_rows_tiny', 'expand_rows_hash', 'expand_rows_hash_to_window',
            'expand_rows_hash_to_compact', 'expand_window_n_win')


@pytest.fixture(autouse=True)
def knobs_restored():
    yield
    for k in KNOBS:
        _lib.tune(k, None)


class Cases:
    """the host matrices and, computed once, what the model makes of them"""

    def __init__(self):
        self.m = dict(edge=rc.edge_matrix()[0], prune=rc.edge_matrix_prune()[0], counts=rc.edge_matrix_counts(), tall=rc.tall_matrix(),
                      empty=rc.empty_matrix())
        self._q, self._pruned = {}, {}

    def dev(self, name):
        return _lib.DeviceCSR.from_arrays(*self.m[name], n_cols=rc.N_COLS)

    def q(self, name, r):
        """inflated and normalised"""
        if (name, r) not in self._q:
            p, j, x = self.m[name]
            self._q[(name, r)] = rc.normalize(p, rc.inflate(x, r))
        return self._q[(name, r)]

    def pruned(self, name, r, thr):
        """r None: the stand-alone prune of the matrix itself"""
        if (name, r, thr) not in self._pruned:
            p, j, x = self.m[name]
            self._pruned[(name, r, thr)] = rc.prune(p, j, x if r is None else self.q(name, r), thr)
        return self._pruned[(name, r, thr)]


@pytest.fixture(scope='module')
def cases():
    return Cases()


def host(d):
    out = d.to_arrays()
    d.free()
    return out


def same(x, y):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y))


def compare(got, ref, r, rtol, what):
    """byte equality at inflation 2 (or without inflation); the same pattern and the bound otherwise -> worst relative difference"""
    exact = r is None or r == 2.0
    if not (np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])) or (exact and not same(got[2:], ref[2:])):
        gp, rp = np.asarray(got[0], np.int64), np.asarray(ref[0], np.int64)
        assert len(gp) == len(rp), what + ': number of rows'
        part = slice(1, 3 if exact else 2)
        bad = [k for k in range(len(rp) - 1) if not (same([x[gp[k]:gp[k + 1]] for x in got[part]], [x[rp[k]:rp[k + 1]] for x in ref[part]])
                                                      and gp[k + 1] - gp[k] == rp[k + 1] - rp[k])]
        k = bad[0]
        raise AssertionError('%s: %d rows differ (pattern%s), the first ones %r; row %d: columns %r values %r, the model says %r %r'
                             % (what, len(bad), ' or bits' if exact else '', bad[:64], k, got[1][gp[k]:gp[k + 1]][:8], got[2][gp[k]:gp[k + 1]][:8],
                                ref[1][rp[k]:rp[k + 1]][:8], ref[2][rp[k]:rp[k + 1]][:8]))
    if exact:
        return 0.0
    w = rc.worst_rel(got[2], ref[2])
    assert w <= rtol, '%s: worst relative difference %.3g > %.3g' % (what, w, rtol)
    return w


# ---------------------------------------------------------------- the CSR row kernels
def test_normalize_l1(cases):
    """worst relative difference: 0 (bit for bit; integer counts, mixed signs, unit rows, three grid passes, no entries at all)"""
    for name in ('counts', 'edge', 'tall', 'empty'):
        p, j, x = cases.m[name]
        d = cases.dev(name)
        _lib.normalize_l1(d)
        got = host(d)
        assert same(got, (p, j, rc.normalize(p, x))), name


@pytest.mark.parametrize('r', rc.INFLATIONS)
def test_inflate(cases, r):
    """inflate + normalise in place.  Bound at 1.5 / 3.0: 3 * 2^-23 = 3.6e-7 relative; measured worst relative difference on the
    MI355X: 0 at all three inflations (at 2.0 by construction)"""
    worst = 0.0
    for name in ('edge', 'tall', 'empty'):
        p, j, x = cases.m[name]
        d = cases.dev(name)
        _lib.inflate(d, r)
        worst = max(worst, compare(host(d), (p, j, cases.q(name, r)), r, rc.INFLATE_RTOL, 'inflate %r, %s' % (r, name)))
    print('inflate at %.1f: worst relative difference %.3g' % (r, worst))


@pytest.mark.parametrize('thr', rc.THRESHOLDS)
def test_prune(cases, thr):
    """the stand-alone prune: bit for bit, and the input is not written"""
    for name in ('prune', 'tall', 'empty'):
        d = cases.dev(name)
        got = host(_lib.prune(d, thr))
        assert same(host(d), cases.m[name]), '%s: prune wrote its input' % name
        compare(got, cases.pruned(name, None, thr), None, 0, 'prune at %r, %s' % (thr, name))


@pytest.mark.parametrize('thr', rc.THRESHOLDS)
@pytest.mark.parametrize('r', rc.INFLATIONS)
def test_inflate_prune_and_keep(cases, r, thr):
    """hhx_inflate_prune (leaves the inflated and normalised values in its input), hhx_inflate_prune_keep (leaves its input alone) and
    prune(inflate(x)).  Bound at 1.5 / 3.0: 6 * 2^-23 = 7.2e-7 relative; measured worst relative difference on the MI355X: 0 at every
    inflation and threshold"""
    worst = 0.0
    for name in ('edge', 'tall', 'empty'):
        ref = cases.pruned(name, r, thr)
        what = 'inflation %r, pruning %r, %s' % (r, thr, name)
        d = cases.dev(name)
        got = host(_lib.inflate_prune(d, r, thr))
        worst = max(worst, compare(got, ref, r, rc.PRUNE_RTOL, 'inflate_prune: ' + what))
        c = cases.dev(name)
        _lib.inflate(c, r)
        two_steps = host(_lib.prune(c, thr))
        assert same(host(d), host(c)), what + ': the input of inflate_prune does not hold the bits of inflate'
        assert same(two_steps, got), what + ': prune(inflate(x)) != inflate_prune(x)'
        d = cases.dev(name)
        kept = host(_lib.inflate_prune_keep(d, r, thr))
        assert same(host(d), cases.m[name]), what + ': inflate_prune_keep wrote its input'
        assert same(kept, got), what + ': inflate_prune_keep != inflate_prune'
    print('inflate_prune at %.1f, pruning %.3g: worst relative difference %.3g' % (r, thr, worst))


def test_convergence_stat():
    """bit for bit on every pair (operands of different patterns, the deciding entry at positions 0 / 63 / 64 / last), and the side of
    d <= 1e-8 each pair was built for"""
    for name, M, last, positive in rc.convergence_pairs():
        a = _lib.DeviceCSR.from_arrays(*M, n_cols=rc.CONV_N)
        b = _lib.DeviceCSR.from_arrays(*last, n_cols=rc.CONV_N)
        got = np.float32(_lib.convergence_stat(a, b))
        a.free()
        b.free()
        ref = rc.convergence(M, last, rc.CONV_N)
        assert got.tobytes() == ref.tobytes(), '%s: %r, the model says %r' % (name, got, ref)
        assert (not got <= np.float32(1e-8)) == positive, name


# ---------------------------------------------------------------- the fused epilogues
@pytest.fixture(scope='module')
def identity():
    n = rc.N_COLS
    I = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32))
    d = _lib.DeviceCSR.from_arrays(*I)
    yield I, d
    d.free()


@pytest.mark.parametrize('r', rc.INFLATIONS)
@pytest.mark.parametrize('hash_max', [None, 0])
def test_fused_epilogues(cases, identity, r, hash_max):
    """expand_inflate_prune(A, I): the products a * 1 are exact, so the result is the model's prune(normalize(inflate(A))).  Default
    hash_max: the rows of at most 32 entries in the tiny class, all others in the hash class; hash_max 0: tiny, compact, and the
    window class for the row of 4097.  Bound at 1.5 / 3.0: 7.2e-7 relative; measured worst relative difference on the MI355X: 0 in
    all six runs"""
    A = cases.m['edge']
    I, dI = identity
    lens = np.diff(A[0])
    want = ec.classes(A, I, hash_max)
    assert np.array_equal(want['f'], lens)
    assert want['tiny'] == int(np.sum(lens <= 32)) and want['tiny'] >= 8
    if hash_max is None:
        assert (want['hash'], want['compact'], want['window']) == (int(np.sum(lens > 32)), 0, 0)
    else:
        assert (want['hash'], want['window']) == (0, 1) and want['cls'][int(np.argmax(lens))] == 0
        assert want['compact'] == int(np.sum(lens > 32)) - 1
    dA = cases.dev('edge')
    worst = 0.0
    try:
        _lib.tune('hash_max', hash_max)
        for thr in rc.THRESHOLDS:
            _lib.profile_reset()
            _lib.profile_enable(True)
            try:
                out, f, nnz_c = _lib.expand_inflate_prune(dA, dI, r, thr)
            finally:
                _lib.profile_enable(False)
            cnt = {k: _lib.profile_counter(k) for k in COUNTERS}
            got = host(out)
            what = 'fused, hash_max %r, inflation %r, pruning %r' % (hash_max, r, thr)
            assert tuple(cnt['expand_rows_' + k] for k in ('window', 'compact', 'tiny', 'hash')) == \
                tuple(want[k] for k in ('window', 'compact', 'tiny', 'hash')), '%s: classes %r' % (what, cnt)
            if cnt['expand_rows_window'] + cnt['expand_rows_hash_to_window']:
                assert cnt['expand_window_n_win'] == want['n_win'], what
            assert f == int(lens.sum()) and nnz_c == int(lens.sum()), what
            worst = max(worst, compare(got, cases.pruned('edge', r, thr), r, rc.PRUNE_RTOL, what))
        assert same(host(dA), A), 'the fused step wrote its operand'
    finally:
        _lib.tune('hash_max', None)
    print('fused epilogues, hash_max %r, at %.1f: worst relative difference %.3g' % (hash_max, r, worst))


# ---------------------------------------------------------------- the links paths on the block-ones matrix
P6 = 2.0 ** -6


@pytest.fixture(scope='module')
def ones():
    L = rc.block_ones()
    d = _lib.DeviceCSR.from_arrays(*L)
    yield L, d, len(L[0]) - 1
    d.free()


@pytest.mark.parametrize('r', [2.0, 1.4])
def test_links_iteration0_closed_form(ones, r):
    """iteration 0 from the raw link matrix: blocks of up to 64 ones keep every entry at float32(1 / m) (the block of 64 sits on the
    threshold), the blocks of 65, 96, 128 and 200 keep their first column at 1.0 — under every arithmetic and layout, bit for bit"""
    L, d, n = ones
    want = rc.block_ones_iteration0(P6)
    for sym, integer, plan in ((1, 1, (True, 1)), (0, 1, (True, 0)), (1, 0, (False, 0)), (0, 0, (False, 0))):
        _lib.tune('links_sym', sym)
        _lib.tune('links_integer', integer)
        what = 'links_sym %d, links_integer %d, inflation %r' % (sym, integer, r)
        # (integer arithmetic, layout): 1 = the symmetric half into the square dense block + the dense epilogue; 0 = the class stream
        assert _lib.links_plan(d) == plan, what
        got = host(_lib.mcl(d, 2, r, 1, P6, links=True)[0])
        compare(got, want, None, 0, 'mcl iteration 0, ' + what)
        blk, f, nnz_c = _lib.expand_links(d, 150, 500, r, P6)          # cuts the block of 65 and the block of 200
        compare(host(blk), rc.block_ones_iteration0(P6, 150, 500), None, 0, 'expand_links rows 150:500, ' + what)
        m_of = np.repeat(rc.BLOCKS, rc.BLOCKS)[150:500].astype(np.int64)
        assert (f, nnz_c) == (int(np.sum(m_of * m_of)), int(m_of.sum())), what


@pytest.mark.parametrize('r', [2.0, 1.4])
def test_dense_rows_closed_form(ones, r):
    """the dense-row epilogue alone and in a group of inflations: at every inflation the block rows are uniform, so all of them give
    the same closed form"""
    L, d, n = ones
    want = rc.block_ones_iteration0(P6)
    assert _lib.links_plan(d) == (True, 1)
    rows = _lib.DenseRows(d, 0, n)
    try:
        compare(host(rows.inflate_prune(r, P6)), want, None, 0, 'dense rows, inflation %r' % r)
        for infl, got in zip((1.4, 2.0, 3.0), rows.inflate_prune_multi([1.4, 2.0, 3.0], P6)):
            compare(host(got), want, None, 0, 'dense rows, group of three, inflation %r' % infl)
    finally:
        rows.free()


def test_block_ones_clusters(ones):
    """the whole loop from the raw link matrix converges and its clusters are the blocks"""
    L, d, n = ones
    assert _lib.links_plan(d) == (True, 1)
    res, n_iter, conv = _lib.mcl(d, 2, 2.0, 200, P6, links=True)
    assert conv and n_iter < 200
    assert rc.clusters_of(*_lib.interpret(res)) == rc.block_ones_clusters()
    res.free()
