"""f4, normalisation on the device: the route and the branches tests/test_gpu_plot_norm.py does not reach (csrc/hhx_plotnorm.hip).  One block
through both implementations of bnewt (the one-workgroup kernel and the host-steered loop, switched with the "plotnorm_small" knob), the chunk
loops of the upload and of apply() ("plotnorm_chunk_cells"), the upload checks and the refusals of a handle, the mat-vec under cancellation
and at the largest count, and bit determinism where the reductions span workgroups."""
import hashlib
import types

import numpy as np
import pytest

from tests import plot_norm_fixture as nf
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return load_golden('plot_norm.npz')


@pytest.fixture(scope='module')
def cases(golden):
    return nf.load_cases(golden)


def _balanced(counts, sizes, small=None, chunk=None, twice=False):
    """one handle from upload to apply() under the given knobs -> the results and what the profile counters saw of the route"""
    from haphic_amd import _lib, plot
    out = types.SimpleNamespace()
    try:
        _lib.tune('plotnorm_small', small)
        _lib.tune('plotnorm_chunk_cells', chunk)
        _lib.profile_enable(True)
        _lib.profile_reset()
        pn = _lib.PlotNorm(counts)
        try:
            out.max, out.min, out.symmetric = pn.max, pn.min, pn.symmetric
            pn.set_blocks(*plot.block_bounds(pn.n, *nf.groups_of(sizes), nf.BIN_SIZE))
            out.outer, out.mvp, out.status = pn.balance()
            out.small_launches = _lib.profile_get('plotnorm_small_blocks')[1]
            out.grid_matvecs = _lib.profile_counter('plotnorm_matvecs')
            out.x_all, out.x_blocks = pn.x()
            if twice:
                again = pn.balance()
                assert all(np.array_equal(a, b) for a, b in zip(again, (out.outer, out.mvp, out.status)))
                out.x_again = pn.x()
            out.matrix = pn.apply()
            out.middle = pn.middle(True)
        finally:
            pn.destroy()
    finally:
        _lib.profile_enable(False)
        _lib.tune('plotnorm_small', None)
        _lib.tune('plotnorm_chunk_cells', None)
    return out


def _same_route(a, b):
    return np.array_equal(a.outer, b.outer) and np.array_equal(a.mvp, b.mvp) and np.array_equal(a.status, b.status)


# ------------------------------------------------------------------ b. one block, both implementations
@pytest.mark.parametrize('name', ['n110', 'n753'])
def test_one_block_through_both_implementations(golden, cases, name):
    """"plotnorm_small" 0 sends every block through bnewt_grid, the default sends them (all <= 512 bins here) through k_bnewt_small: the same
    steps, x within the spread the reference's own bnewt shows under a permutation; the whole matrix takes the host-steered loop both times"""
    sizes, counts = cases[name]
    tol = nf.tolerance(golden[name + '__perm_spread'])
    small, grid = _balanced(counts, sizes), _balanced(counts, sizes, small=0)
    print(name, 'outer', small.outer.tolist(), grid.outer.tolist(), 'mvp', small.mvp.tolist(), grid.mvp.tolist())
    assert not small.status.any() and not grid.status.any()
    # the route really differed: one launch of the one-workgroup kernel against none, the grid's own mat-vec count
    assert small.small_launches == 1 and grid.small_launches == 0
    assert small.grid_matvecs == small.mvp[-1] and grid.grid_matvecs == grid.mvp.sum()
    assert _same_route(small, grid)
    d = nf.rel_diff(grid.x_blocks, small.x_blocks)
    print(name, 'x_blocks, grid against one workgroup: %.3g  tolerance %.3g' % (d, tol))
    assert d <= tol and ((grid.x_blocks == 0) == (small.x_blocks == 0)).all()
    assert grid.x_all.tobytes() == small.x_all.tobytes()
    # both against the reference
    assert nf.rel_diff(grid.x_blocks, golden[name + '__x_blocks']) <= tol
    assert np.array_equal(grid.outer, golden[name + '__outer']) and np.array_equal(grid.mvp, golden[name + '__mvp'] - 1)
    assert grid.matrix.tobytes() == nf.expected_matrix(counts, sizes, grid.x_all, grid.x_blocks).tobytes()


def test_small_path_threshold(golden, cases):
    """n753 has blocks of 300, 200 and 250 bins: at "plotnorm_small" 300 the 300-bin block runs inside one workgroup, at 299 it is steered from
    the host (its mat-vecs show in the grid's counter); the knob is clamped to [0, 512]"""
    sizes, counts = cases['n753']
    tol = nf.tolerance(golden['n753__perm_spread'])
    assert [hi - lo for lo, hi in nf.blocks_of(sizes)] == [300, 200, 250]
    at, below, default = _balanced(counts, sizes, small=300), _balanced(counts, sizes, small=299), _balanced(counts, sizes)
    assert at.small_launches == 1 and below.small_launches == 1
    assert at.grid_matvecs == at.mvp[-1]
    assert below.grid_matvecs == below.mvp[0] + below.mvp[-1]
    assert _same_route(at, below) and _same_route(at, default)
    # 300: the same kernel on the same blocks as the default
    assert at.x_blocks.tobytes() == default.x_blocks.tobytes() and at.x_all.tobytes() == default.x_all.tobytes()
    assert nf.rel_diff(below.x_blocks, at.x_blocks) <= tol and below.x_all.tobytes() == at.x_all.tobytes()
    assert below.x_blocks[300:].tobytes() == at.x_blocks[300:].tobytes()          # the other two blocks stayed where they were
    sizes, counts = cases['n110']
    negative, huge, zero, default = (_balanced(counts, sizes, small=v) for v in (-5, 10 ** 6, 0, None))
    assert negative.small_launches == 0 and negative.x_blocks.tobytes() == zero.x_blocks.tobytes()
    assert huge.small_launches == 1 and huge.x_blocks.tobytes() == default.x_blocks.tobytes()


# ------------------------------------------------------------------ c. chunking
@pytest.mark.parametrize('name', ['n110', 'n753'])
def test_chunked_upload_and_apply(cases, name):
    """one row per chunk, nine rows per chunk with a ragged last one, and everything in one chunk: the same upload, the same matrix"""
    from haphic_amd import _lib
    sizes, counts = cases[name]
    n = len(counts)
    assert n % 9 != 0 and (9 * n + 1) // n == 9
    v = np.random.default_rng(5).lognormal(0, 1, n)
    runs = {}
    for chunk in (None, n, 9 * n + 1):
        runs[chunk] = _balanced(counts, sizes, chunk=chunk)
        try:
            _lib.tune('plotnorm_chunk_cells', chunk)
            pn = _lib.PlotNorm(counts)
            try:
                runs[chunk].product = pn.matvec(0, n, v)
            finally:
                pn.destroy()
        finally:
            _lib.tune('plotnorm_chunk_cells', None)
    whole = runs[None]
    assert (whole.max, whole.min, whole.symmetric) == (counts.max(), counts.min(), True)
    assert whole.matrix.tobytes() == nf.expected_matrix(counts, sizes, whole.x_all, whole.x_blocks).tobytes()
    for chunk in (n, 9 * n + 1):
        r = runs[chunk]
        assert (r.max, r.min, r.symmetric) == (whole.max, whole.min, whole.symmetric)
        assert r.product.tobytes() == whole.product.tobytes()
        assert _same_route(r, whole) and r.x_all.tobytes() == whole.x_all.tobytes() and r.x_blocks.tobytes() == whole.x_blocks.tobytes()
        assert r.matrix.tobytes() == whole.matrix.tobytes()
        assert r.matrix.tobytes() == nf.expected_matrix(counts, sizes, r.x_all, r.x_blocks).tobytes()
        assert r.middle[0] == whole.middle[0] and r.middle[1].tobytes() == whole.middle[1].tobytes()


# ------------------------------------------------------------------ d. upload checks and refusals
def _planted(counts, what):
    """-> (matrix, valid): one value planted in a copy of the counts (mirrored off the diagonal: the matrix stays symmetric)"""
    n = len(counts)
    m = counts.copy()
    mid = (n // 2, n // 2 - 1)
    cell, value = {'minus_one_first': ((0, 0), -1), 'minus_one_last': ((n - 1, n - 1), -1), 'two_to_31_first': ((0, 0), 2 ** 31),
                   'two_to_31_middle': (mid, 2 ** 31), 'two_to_31_less_one': (mid, 2 ** 31 - 1), 'all_negative': (None, None)}[what]
    if cell is None:
        m = -m - 3                              # every cell below zero: the largest is -3, not 0
    else:
        m[cell] = m[cell[::-1]] = value
    return m, what == 'two_to_31_less_one'


PLANTS = ['minus_one_first', 'minus_one_last', 'two_to_31_first', 'two_to_31_middle', 'two_to_31_less_one', 'all_negative']


@pytest.mark.parametrize('what', PLANTS)
@pytest.mark.parametrize('name', ['n5', 'n110'])
def test_upload_reports_the_extremes_and_an_invalid_handle_refuses(cases, name, what):
    from haphic_amd import _lib, plot
    sizes, counts = cases[name]
    m, valid = _planted(counts, what)
    n = len(m)
    # the planted value is the extreme the upload has to report (numpy's own min / max of the int64 matrix are the reference)
    planted = {'minus_one_first': -1, 'minus_one_last': -1, 'two_to_31_first': 2 ** 31, 'two_to_31_middle': 2 ** 31, 'two_to_31_less_one': 2 ** 31 - 1,
               'all_negative': -3}[what]
    want_min, want_max = int(m.min()), int(m.max())
    assert planted == (want_min if planted == -1 else want_max) and (want_min < 0) == (what.startswith('minus') or what == 'all_negative')
    group_list, group_size_dict = nf.groups_of(sizes)
    pn = _lib.PlotNorm(m)
    try:
        assert (pn.min, pn.max, pn.symmetric) == (want_min, want_max, True)
        pn.set_blocks(*plot.block_bounds(n, group_list, group_size_dict, nf.BIN_SIZE))
        v = np.ones(n)
        if valid:
            A = m.astype(np.longdouble) + np.longdouble(0.00001)
            want = A @ v.astype(np.longdouble)
            assert (np.abs(pn.matvec(0, n, v) - want) <= 2 * (n + 2) * 2.0 ** -53 * want).all()
            count, pair = pn.middle(False)
            cells = np.sort(np.concatenate([m[lo:hi, lo:hi][~np.eye(hi - lo, dtype=bool)] for lo, hi in nf.blocks_of(sizes)]))
            assert count == len(cells) and pair.tolist() == cells[[(count - 1) // 2, count // 2]].tolist()
            outer, mvp, status = pn.balance()
            assert not status.any()
            x_all, x_blocks = pn.x()
            A = m + 0.00001
            assert np.sum((1 - x_all * (A @ x_all)) ** 2) <= 1e-12 * (1 + 1e-6)          # the reference's stopping rule, on the host
            for lo, hi in nf.blocks_of(sizes):
                assert np.sum((1 - x_blocks[lo:hi] * (A[lo:hi, lo:hi] @ x_blocks[lo:hi])) ** 2) <= 1e-12 * (1 + 1e-6)
            assert pn.apply().tobytes() == nf.expected_matrix(m, sizes, x_all, x_blocks).tobytes()
        else:
            for call in (pn.balance, lambda: pn.matvec(0, n, v), lambda: pn.middle(False), lambda: pn.middle(True), pn.apply):
                with pytest.raises(RuntimeError, match='libhaphic_hip'):
                    call()
    finally:
        pn.destroy()
    if valid:
        return
    seen = []

    def original(*args):
        seen.append(args)
        return 'original', 7
    for mode in ('KR', 'none'):
        args = (m, group_list, group_size_dict, nf.BIN_SIZE, mode, nf.VMAX_COEF, -1)
        assert plot._normalize_matrix(*args, _original=original) == ('original', 7)
        assert all(a is b for a, b in zip(seen[-1], args))
        with pytest.raises(RuntimeError, match='reference normalize_matrix'):
            plot.normalize_matrix(*args)
    assert len(seen) == 2


@pytest.mark.parametrize('name', ['n5', 'n110'])
def test_symmetry_flag(cases, name):
    from haphic_amd import _lib
    sizes, counts = cases[name]
    n = len(counts)
    flags = {}
    for cell in (None, (0, n - 1), (n - 2, n - 1), (1, 0), (n - 1, 0), (n - 1, n - 1)):
        m = counts.copy()
        if cell:
            m[cell] += 1
        pn = _lib.PlotNorm(m)
        flags[cell] = pn.symmetric
        assert (pn.min, pn.max) == (m.min(), m.max())
        pn.destroy()
    assert flags == {None: True, (0, n - 1): False, (n - 2, n - 1): False, (1, 0): False, (n - 1, 0): False, (n - 1, n - 1): True}


def test_apply_and_kr_median_need_a_balance_of_these_blocks(cases):
    from haphic_amd import _lib, plot
    sizes, counts = cases['n110']
    bounds = plot.block_bounds(len(counts), *nf.groups_of(sizes), nf.BIN_SIZE)
    pn = _lib.PlotNorm(counts)
    try:
        def refused():
            for call in (pn.apply, lambda: pn.middle(True)):
                with pytest.raises(RuntimeError, match='no balancing has converged'):
                    call()
        refused()                                   # no blocks, no balance
        pn.set_blocks(*bounds)
        refused()
        assert pn.middle(False)[0] > 0              # the counts' own median needs no balance
        assert not pn.balance()[2].any()
        first = pn.apply()
        count, pair = pn.middle(True)
        pn.set_blocks(*bounds)                      # the blocks' x is no longer that of these blocks
        refused()
        assert not pn.balance()[2].any()
        assert pn.apply().tobytes() == first.tobytes() and pn.middle(True)[1].tobytes() == pair.tobytes()
    finally:
        pn.destroy()


# ------------------------------------------------------------------ e. mat-vec with cancellation and extreme counts
def test_matvec_with_cancellation_and_extreme_counts():
    """n = 70, counts from {0, 1, 7, 2^31 - 1}, vectors of both signs over 300 decades, every sub-block start 0 ... 8 and length 1 ... 40 and the
    whole matrix, against np.longdouble.  Bound per element: 2 (m + 2) 2^-53 (|A| @ |v|) — the dot-product bound of any summation order
    (m 2^-53), one rounding for c + 0.00001 and one for the product, doubled."""
    from haphic_amd import _lib
    n = 70
    rng = np.random.default_rng(23)
    upper = np.triu(rng.choice(np.array([0, 1, 7, 2 ** 31 - 1], np.int64), (n, n)))
    counts = upper + np.triu(upper, 1).T
    assert counts.max() == 2 ** 31 - 1 and counts.min() == 0 and np.array_equal(counts, counts.T)
    A = counts.astype(np.longdouble) + np.longdouble(0.00001)
    assert np.finfo(np.longdouble).nmant >= 63
    spans = [(lo, lo + m) for lo in range(0, 9) for m in range(1, 41)] + [(0, n)]
    pn = _lib.PlotNorm(counts)
    worst = 0.0
    try:
        assert (pn.min, pn.max, pn.symmetric) == (0, 2 ** 31 - 1, True)
        for k, (lo, hi) in enumerate(spans):
            m = hi - lo
            # one span in three in each regime: 300 decades, tiny, huge (2^31 * 1e150 * 70 is far from overflow)
            exponent = (rng.uniform(-150, 150, m), rng.uniform(-150, -140, m), rng.uniform(140, 150, m))[k % 3]
            v = rng.choice([-1.0, 1.0], m) * rng.uniform(1, 10, m) * 10.0 ** np.floor(exponent)
            got = pn.matvec(lo, hi, v)
            sub = A[lo:hi, lo:hi]
            want, scale = sub @ v.astype(np.longdouble), sub @ np.abs(v).astype(np.longdouble)
            bound = 2 * (m + 2) * 2.0 ** -53 * scale
            err = np.abs(got.astype(np.longdouble) - want)
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(got).all() and (err <= bound).all(), (lo, hi, float((err / bound).max()))
    finally:
        pn.destroy()
    print('mat-vec under cancellation: worst error / bound %.3g' % worst)


# ------------------------------------------------------------------ g. determinism
def _digest(r):
    return hashlib.sha256(r.x_all.tobytes() + r.x_blocks.tobytes() + r.matrix.tobytes()).hexdigest()


def test_n2055_two_balances_and_two_handles_give_the_same_bits(cases):
    """reductions over more than one workgroup (k_fold over 514 row partials, more than PN_T) and a block of 1302 bins"""
    sizes, counts = cases['n2055']
    a = _balanced(counts, sizes, twice=True)
    b = _balanced(counts, sizes)
    assert a.x_again[0].tobytes() == a.x_all.tobytes() and a.x_again[1].tobytes() == a.x_blocks.tobytes()
    assert _same_route(a, b) and _digest(a) == _digest(b)
    assert a.small_launches == 1 and a.grid_matvecs == a.mvp[3] + a.mvp[4]


def test_n753_host_steered_blocks_give_the_same_bits(cases):
    sizes, counts = cases['n753']
    a = _balanced(counts, sizes, small=0, twice=True)
    b = _balanced(counts, sizes, small=0)
    assert a.x_again[0].tobytes() == a.x_all.tobytes() and a.x_again[1].tobytes() == a.x_blocks.tobytes()
    assert _same_route(a, b) and _digest(a) == _digest(b) and a.small_launches == 0
