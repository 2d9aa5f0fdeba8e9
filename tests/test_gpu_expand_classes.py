"""The fused expansion (hhx_expand_impl) class by class: engineered operands that reach every row class, several column windows,
the compact kernel's rank windows and staged chunks, the exact class thresholds, every knob of the window kernel, a pool-overflow
retry, row blocks and a few chained iterations — each against the oracle (spgemm mode 1, fx_shift 52), and each first asserting,
from the device's own per-class counters, that the classes it is meant for really ran (tests/expand_classes.py mirrors the rule).
Run on the GPU box:  python -m pytest tests/test_gpu_expand_classes.py -m gpu"""
import numpy as np
import pytest

from haphic_amd import _lib
from oracle import oracle as orc
from tests import expand_classes as ec

pytestmark = pytest.mark.gpu

POW_RTOL = 1e-6                 # powf (oracle) vs float(pow) (device) at inflations other than 2
PRUNING = 1e-4
COUNTERS = ('expand_rows_window', 'expand_rows_compact', 'expand_rows_tiny', 'expand_rows_hash', 'expand_rows_hash_to_window',
            'expand_rows_hash_to_compact', 'expand_window_n_win', 'expand_pool_retries', 'expand_group_products',
            'expand_block_tile_launches')


def oracle_fused(A, B, infl):
    c = orc.spgemm(A, B, n_cols=len(B[0]) - 1, mode=1, fx_shift=52)
    x = orc.normalize_l1(c[0], orc.power(c[2], infl))
    return orc.prune((c[0], c[1], x), PRUNING), int(c[0][-1])


def fused(a, b, infl):
    """one fused step with the profile counters on: (CSR triple, products, nnz of the expanded matrix, counters)"""
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        p, f, z = _lib.expand_inflate_prune(a, b, infl, PRUNING)
    finally:
        _lib.profile_enable(False)
    cnt = {k: _lib.profile_counter(k) for k in COUNTERS}
    got = p.to_arrays()
    p.free()
    return got, f, z, cnt


def assert_classes(cnt, want, what):
    """the device's k_classify counts == the host mirror's, and the window launch used the mirror's window plan"""
    got = tuple(cnt['expand_rows_' + k] for k in ('window', 'compact', 'tiny', 'hash'))
    exp = tuple(want[k] for k in ('window', 'compact', 'tiny', 'hash'))
    assert got == exp, '%s: classes (window, compact, tiny, hash) %r, the mirror says %r' % (what, got, exp)
    if cnt['expand_rows_window'] + cnt['expand_rows_hash_to_window']:
        assert cnt['expand_window_n_win'] == want['n_win'], '%s: %d column windows, the plan says %d' % (what, cnt['expand_window_n_win'], want['n_win'])
    else:
        assert cnt['expand_window_n_win'] == 0


def same(x, y):
    return all(np.array_equal(u, v) for u, v in zip(x, y))


def assert_matches(got, ref, infl, what):
    assert np.array_equal(got[0], ref[0]), what + ': indptr'
    assert np.array_equal(got[1], ref[1]), what + ': indices'
    if infl == 2.0:
        assert np.array_equal(got[2], ref[2]), what + ': values (bit-equal at inflation 2)'
    else:
        np.testing.assert_allclose(got[2], ref[2], rtol=POW_RTOL, atol=0, err_msg=what)


@pytest.fixture(scope='module')
def multi():
    """the n = 45 000 operand of every class and three column windows, on the device, with the oracle's fused step at 2.0"""
    A, roles = ec.multi_window()
    n = len(A[0]) - 1
    c = ec.classes(A, A, 0)
    # the shape the cases below are written for
    assert n % 64 and c['n_win'] == 3 and n - 2 * c['cap_win'] < c['cap_win'], ec.describe(c)
    assert c['window'] >= 1024 and c['compact'] > 0 and c['tiny'] > 0, ec.describe(c)
    assert np.all(np.diff(A[0])[roles['heavy']] >= 128) and np.all(c['f'][roles['heavy']] >= c['window_min'])
    assert np.all(c['f'][roles['medium']] < c['window_min']) and np.all(np.diff(A[0])[roles['long']] > ec.STAGE)
    d = _lib.DeviceCSR.from_arrays(*A)
    ref, nnz_c = oracle_fused(A, A, 2.0)
    yield dict(A=A, roles=roles, d=d, n=n, ref=ref, nnz_c=nnz_c)
    d.free()


@pytest.mark.parametrize('infl', [2.0, 1.4, 1.1])
@pytest.mark.parametrize('hash_max', [0, None])
def test_multi_window_every_class(multi, infl, hash_max):
    """heavy rows in the window class over 3 column windows (the last one short), medium rows in the compact class with more
    distinct columns than one LDS rank window holds, rows of more than STAGE A entries, tiny rows — one launch sequence; with
    the hash class on, it takes every non-tiny row and hands the ones that do not fit back to the window and compact classes"""
    A, d = multi['A'], multi['d']
    want = ec.classes(A, A, hash_max)
    _lib.tune('hash_max', hash_max)
    try:
        got, f, nnz_c, cnt = fused(d, d, infl)
    finally:
        _lib.tune('hash_max', None)
    assert_classes(cnt, want, 'multi-window, hash_max %r' % hash_max)
    if hash_max is None:
        assert cnt['expand_rows_hash_to_window'] > 0 and cnt['expand_rows_hash_to_compact'] > 0, cnt
    ref, ref_nnz_c = (multi['ref'], multi['nnz_c']) if infl == 2.0 else oracle_fused(A, A, infl)
    assert f == int(want['f'].sum()) and nnz_c == ref_nnz_c
    assert_matches(got, ref, infl, 'multi-window fused step at %r, hash_max %r' % (infl, hash_max))


def test_multi_window_knob_matrix(multi):
    """every setting of every window-kernel knob gives the bits of the default run (which matches the oracle): the block tiles,
    the per-segment tiles, the wave batches, the grouped kernel, the row order, the hash class, and more column windows"""
    A, d = multi['A'], multi['d']
    base, _, _, cnt = fused(d, d, 2.0)
    assert_classes(cnt, ec.classes(A, A), 'knob matrix, default')
    assert cnt['expand_block_tile_launches'] == 3 and cnt['expand_group_products'] == 0
    assert_matches(base, multi['ref'], 2.0, 'knob matrix, default')
    plain = ec.classes(A, A, 0)

    def check(what, n_win=3):
        got, _, _, c = fused(d, d, 2.0)
        assert_classes(c, dict(plain, n_win=n_win), what)
        assert same(got, base), what + ' changed bits'
        return c

    _lib.tune('hash_max', 0)                 # the window-class rows straight from k_classify
    try:
        check('hash_max 0')
        for bt in (0, 1, 2, 5, 11, 15, 31):
            _lib.tune('block_tiles', bt)
            c = check('block_tiles %d' % bt)
            assert c['expand_block_tile_launches'] == (3 if bt else 0)
        _lib.tune('block_tiles', 0)
        for tu in (1, 2, 3, 4, 8):
            _lib.tune('tile_u', tu)
            check('block_tiles 0, tile_u %d' % tu)
        _lib.tune('tile_u', None)
        _lib.tune('block_tiles', None)
        for wb in (1, 3, 8, 16, 32):
            _lib.tune('win_batch', wb)
            check('win_batch %d' % wb)
        _lib.tune('win_batch', None)
        for r in (2, 4):
            _lib.tune('reuse', r)
            got, _, _, c = fused(d, d, 2.0)
            assert c['expand_group_products'] > 0, 'reuse %d: the grouped kernel did not run' % r
            assert (c['expand_rows_window'], c['expand_rows_compact']) == (plain['window'], plain['compact'])
            assert same(got, base), 'reuse %d changed bits' % r
        _lib.tune('reuse', None)
        _lib.tune('row_order', 0)
        check('row_order 0')
        _lib.tune('row_order', None)
        _lib.tune('cache_slice_mb', 1)       # 4 MB of B: 4 slices of 1 MB
        assert ec.window_plan(multi['n'], int(A[0][-1]), 1)[1] == 4
        check('cache_slice_mb 1', n_win=4)
    finally:
        for k in ('hash_max', 'block_tiles', 'tile_u', 'win_batch', 'reuse', 'row_order', 'cache_slice_mb'):
            _lib.tune(k, None)


def test_multi_window_row_blocks(multi):
    """row blocks cut through the window-class rows (a multi-GPU shard) give the rows of the whole matrix"""
    A, d, heavy = multi['A'], multi['d'], multi['roles']['heavy']
    whole = multi['ref']
    for r0, r1 in ((int(heavy[100]), int(heavy[700]) + 1), (int(heavy[701]) + 1, int(heavy[1400]))):
        lo, hi = A[0][r0], A[0][r1]
        blk = (np.ascontiguousarray(A[0][r0:r1 + 1] - lo), A[1][lo:hi], A[2][lo:hi])
        want = ec.classes(blk, A, None)
        db = d.row_block(r0, r1)
        try:
            got, _, _, cnt = fused(db, d, 2.0)
        finally:
            db.free()
        assert_classes(cnt, want, 'row block %d:%d' % (r0, r1))
        assert cnt['expand_rows_hash_to_window'] > 0
        a, b = whole[0][r0], whole[0][r1]
        assert np.array_equal(got[0], whole[0][r0:r1 + 1] - a)
        assert np.array_equal(got[1], whole[1][a:b]) and np.array_equal(got[2], whole[2][a:b]), 'row block %d:%d' % (r0, r1)


def test_multi_window_chained_iterations(multi):
    """three iterations of the loop picked up after iteration 0 (hhx_mcl_resume: every iteration's pools sized from the one
    before) against the oracle's loop: per-iteration statistics and the final matrix, bit for bit"""
    A, d = multi['A'], multi['d']
    res, n_iter, conv, stats = _lib.mcl_resume(d, 1, 2, 2.0, 4, PRUNING, want_stats=True)
    o = orc.mcl(A, 2, 2.0, 4, PRUNING, spgemm_mode=1, fx_shift=52, want_stats=True, first_it=1)
    assert (n_iter, conv) == (o[3], o[4])
    assert np.array_equal(stats, o[5]), (stats, o[5])
    assert_matches(res.to_arrays(), o[:3], 2.0, 'chained iterations')
    res.free()


def test_compact_rank_windows_and_stage_chunks(multi):
    """the compact rows alone (hash class off): medium rows wider than cap_cmp distinct columns and rows of more than STAGE A
    entries, through a row block that holds only such rows and light ones"""
    A, d, roles = multi['A'], multi['d'], multi['roles']
    c = ec.classes(A, A, 0)
    cc = orc.spgemm(A, A, mode=1, fx_shift=52)
    wide = np.diff(cc[0])
    assert np.all(wide[roles['medium']] > c['cap_cmp']) and np.all(wide[roles['long']] > c['cap_cmp'])
    ref = multi['ref']
    _lib.tune('hash_max', 0)
    try:
        got, _, _, cnt = fused(d, d, 2.0)
    finally:
        _lib.tune('hash_max', None)
    assert_classes(cnt, c, 'compact rows')
    for r in np.concatenate([roles['medium'][:64], roles['long']]):
        assert np.array_equal(got[1][got[0][r]:got[0][r + 1]], ref[1][ref[0][r]:ref[0][r + 1]]), 'compact row %d: pattern' % r
        assert np.array_equal(got[2][got[0][r]:got[0][r + 1]], ref[2][ref[0][r]:ref[0][r + 1]]), 'compact row %d: values' % r


@pytest.mark.parametrize('infl', [2.0, 1.4])
@pytest.mark.parametrize('hash_max', [0, None])
def test_class_boundaries(infl, hash_max):
    """rows with f exactly 32 / 33, window_min - 1 / window_min, the hash default / + 1, and rows of one entry"""
    A, rows_of = ec.boundaries()
    n = len(A[0]) - 1
    want = ec.classes(A, A, hash_max)
    f = want['f']
    for t, rows in rows_of.items():
        assert np.all(f[rows] == t), t
    wmin, hdef = ec.window_min(n), ec.hash_default(n)
    assert set(rows_of) == {1, 32, 33, wmin - 1, wmin, hdef, hdef + 1}
    cls = want['cls']
    assert np.all(cls[rows_of[32]] == 2) and np.all(cls[rows_of[33]] != 2) and np.all(cls[rows_of[1]] == 2)
    if hash_max is None:
        assert np.all(cls[rows_of[hdef]] == 3) and np.all(cls[rows_of[hdef + 1]] == 0) and np.all(cls[rows_of[wmin - 1]] == 3)
    else:
        assert np.all(cls[rows_of[wmin - 1]] == 1) and np.all(cls[rows_of[wmin]] == 0)
    d = _lib.DeviceCSR.from_arrays(*A)
    _lib.tune('hash_max', hash_max)
    try:
        got, fp, nnz_c, cnt = fused(d, d, infl)
    finally:
        _lib.tune('hash_max', None)
        d.free()
    assert_classes(cnt, want, 'boundaries, hash_max %r' % hash_max)
    ref, ref_nnz_c = oracle_fused(A, A, infl)
    assert fp == int(f.sum()) and nnz_c == ref_nnz_c
    assert_matches(got, ref, infl, 'class boundaries at %r, hash_max %r' % (infl, hash_max))


@pytest.fixture(scope='module')
def uniform():
    A = ec.uniform_rows()
    d = _lib.DeviceCSR.from_arrays(*A)
    ref, nnz_c = oracle_fused(A, A, 2.0)
    yield dict(A=A, d=d, ref=ref, nnz_c=nnz_c)
    d.free()


def test_pool_overflow_retry(uniform):
    """thousands of survivors per row: the first survivor pool (4 entries per entry of A, at least 4 M) overflows and every
    launch runs again with pools of the demand — the same result as the oracle"""
    A, d = uniform['A'], uniform['d']
    first_pool = max(4 * int(A[0][-1]) + 16 * (len(A[0]) - 1), 1 << 22)
    assert len(uniform['ref'][1]) > first_pool
    for hash_max in (None, 0):
        _lib.tune('hash_max', hash_max)
        try:
            got, f, nnz_c, cnt = fused(d, d, 2.0)
        finally:
            _lib.tune('hash_max', None)
        assert_classes(cnt, ec.classes(A, A, hash_max), 'pool retry, hash_max %r' % hash_max)
        assert cnt['expand_pool_retries'] > 0, 'the survivor pool did not overflow'
        assert nnz_c == uniform['nnz_c']
        assert_matches(got, uniform['ref'], 2.0, 'after a pool retry, hash_max %r' % hash_max)


def test_cache_slice_forces_windows_at_8000(uniform):
    """n = 8000 fits one column window; tune "cache_slice_mb" is the only way to get several there: same bits, 3 windows"""
    A, d = uniform['A'], uniform['d']
    plain = ec.classes(A, A, 0)
    assert plain['n_win'] == 1 and ec.window_plan(len(A[0]) - 1, int(A[0][-1]), 1)[1] == 3
    _lib.tune('hash_max', 0)
    try:
        base, _, _, cnt = fused(d, d, 2.0)
        assert_classes(cnt, plain, 'n = 8000, one window')
        _lib.tune('cache_slice_mb', 1)
        got, _, _, cnt = fused(d, d, 2.0)
        assert_classes(cnt, dict(plain, n_win=3), 'n = 8000, cache_slice_mb 1')
    finally:
        _lib.tune('cache_slice_mb', None)
        _lib.tune('hash_max', None)
    assert_matches(base, uniform['ref'], 2.0, 'n = 8000, one window')
    assert same(got, base), 'cache_slice_mb 1 changed bits'
