"""The dense epilogue of the inflation sweep (hhx_dense_inflate_prune, hhx_dense_inflate_prune_multi) at the smallest shapes where
the step tail that k_dense_epilogue_sw and k_dense_epilogue_multi share can go wrong: swizzled slots with partly empty last lanes,
a short last window, a change of `per` inside a row, the triangle's short last block row, a pool overflow in both drivers, an
empty and a one-row block.  Bit for bit against
  * iteration 0 of the fused path, _lib.mcl(links, 2, r, 1, pruning, links=True), which runs none of the dense epilogue kernels;
  * the oracle's DenseRows.inflate_prune (tests/oracle_lib.py: inflate_prune_keep) over the oracle's rows of M^2 in the integer
    arithmetic of a link matrix (orc.expand_links, as test_dense_sweep_equals_fused_iteration0 takes them — the rows
    oracle_lib.DenseRows itself forms are the float arithmetic's and differ in the last bit): indices exactly, values exactly at
    inflation 2.0, the only one where the oracle's powf and the device's float(exp2(r log2 x)) are the same function.
Run on the GPU box:  python -m pytest tests/test_gpu_dense_epilogue.py -m gpu"""
import contextlib

import numpy as np
import pytest

from haphic_amd import _lib
from oracle import oracle as orc
from tests import expand_classes as ec
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

INFLATIONS = (1.1, 1.4, 2.0, 3.0)
EIGHT = (1.3, 1.1, 1.2, 1.4, 1.5, 1.7, 2.5, 3.0)          # a full pass of the multi kernel (no 2.0: that one is routed away)
PRUNING = 1e-4
T_WIN = 1024                                                # EX_T_WIN: threads of an epilogue workgroup


@contextlib.contextmanager
def tuned(**knobs):
    try:
        for k, v in knobs.items():
            if v is not None:
                _lib.tune(k, v)
        yield
    finally:
        for k in knobs:
            _lib.tune(k, None)


def host(m):
    a = tuple(np.array(x) for x in m.to_arrays())
    m.free()
    return a


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def rows_of(a, r0, r1):
    p, j, x = a
    return p[r0:r1 + 1] - p[r0], j[p[r0]:p[r1]], x[p[r0]:p[r1]]


def step_shapes(n, cap, n_win):
    """(per, gm) of every window of a row: owned slots per thread and the swizzle mask of k_dense_epilogue_sw / _multi"""
    out = []
    for w in range(n_win):
        per = (min(n, (w + 1) * cap) - w * cap + T_WIN - 1) // T_WIN
        out.append((per, min(32, per & -per) - 1))
    return out


class Case:
    """a link matrix on the device, the window plan it is expanded under and the fused iteration 0 at any inflation"""

    def __init__(self, chr_len, n_pairs, slice_mb, plan, shapes):
        import torch
        from haphic_amd import synth
        gen = synth.make_genome(8, chr_len, 20_000, seed=8)
        n = gen.n
        lex = gen.lexical_rank()
        t = orc.FragTable(lex, gen.length, np.arange(n, dtype=np.int32), np.zeros(n, np.uint8), 0, lex, gen.length, np.ones(n, np.uint8))
        id1, p1, id2, p2 = synth.sample_pairs(gen, n_pairs, seed=9, device='cuda')
        ing = _lib.Ingest(t, 500_000, bins=False, skip_intra=True)
        ing.push_device(id1.numel(), id1.data_ptr(), p1.data_ptr(), id2.data_ptr(), p2.data_ptr())
        torch.cuda.synchronize()
        self.links = ing.link_matrix(np.ones(n, np.uint8))[0]
        ing.destroy()
        self.n = self.links.shape3[0]
        self.L = tuple(np.array(x) for x in self.links.to_arrays())
        self.knobs = dict(cache_slice_mb=slice_mb)
        # the plan this file relies on: a change of window_plan() must fail here, not silently empty the tests below
        self.cap, self.n_win = ec.window_plan(self.n, self.links.nnz, slice_mb or 0)
        assert (self.cap, self.n_win) == plan, (self.n, self.links.nnz, self.cap, self.n_win)
        assert step_shapes(self.n, self.cap, self.n_win) == shapes, step_shapes(self.n, self.cap, self.n_win)
        assert _lib.links_integer_ok(self.links)
        self.fused = {}

    def want(self, r, pruning=PRUNING):
        if (r, pruning) not in self.fused:
            with tuned(**self.knobs):
                self.fused[(r, pruning)] = host(_lib.mcl(self.links, 2, r, 1, pruning, links=True)[0])
        return self.fused[(r, pruning)]

    def block(self, r0=0, r1=None, **knobs):
        with tuned(**dict(self.knobs, **knobs)):
            return _lib.DenseRows(self.links, r0, self.n if r1 is None else r1)

    def oracle_rows(self, r0, r1):
        return ol.DeviceCSR(*orc.expand_links(self.L, rows=np.arange(r0, r1)), n_cols=self.n)


@pytest.fixture(scope='module')
def one_window():
    """~4000 contigs, one window of 4032 columns: per = 4, gm = 3 (swizzled slots); the last lane with slots owns fewer than four,
    the lanes behind it none"""
    c = Case(9_950_000, 600_000, None, (4032, 1), [(4, 3)])
    assert c.n % 4 != 0 and c.n < 4 * (T_WIN - 1)
    yield c
    c.links.free()


@pytest.fixture(scope='module')
def three_windows():
    """~6200 contigs under cache_slice_mb 1 (more than 2 MB of operand): windows of 2112 / 2112 / the rest, per = 3, 3, 2 and
    gm = 0, 0, 1 — a short last window (an odd number of columns: one lane owns a single slot) and a change of `per` inside a row"""
    c = Case(15_550_000, 1_000_000, 1, (2112, 3), [(3, 0), (3, 0), (2, 1)])
    assert c.links.nnz * 8 > 2 << 20 and ec.window_plan(c.n, c.links.nnz, 0)[1] == 1 and (c.n - 2 * c.cap) % 2 == 1
    yield c
    c.links.free()


def check_groupings(c, tri):
    """every grouping of the drivers on the whole matrix, against the fused iteration 0"""
    knobs = dict(dense_tri=1) if tri else {}

    def fresh(**more):
        blk = c.block(**dict(knobs, **more))
        if tri:                                             # the triangle is not addressable as rows: that is how it shows
            with pytest.raises(RuntimeError):
                blk.device()
        else:
            assert blk.device()[2:] == (c.cap, c.n_win)
        return blk

    def check_multi(blk, group, what):
        for r, got in zip(group, blk.inflate_prune_multi(group, PRUNING)):
            assert same(host(got), c.want(r)), '%s, group %r, inflation %r' % (what, group, r)

    blk = fresh()
    for r in INFLATIONS:                                    # the one-inflation driver, ascending: each call under the hint of the one before
        assert same(host(blk.inflate_prune(r, PRUNING)), c.want(r)), 'alone, inflation %r' % r
    for r in (1.1,):                                        # ... and below the hint the call at 3.0 left
        assert same(host(blk.inflate_prune(r, PRUNING)), c.want(r)), 'alone below the hint, inflation %r' % r
    blk.free()
    blk = fresh()                                           # under the seed hint
    check_multi(blk, (1.4, 2.0, 3.0, 1.1), '2.0 routed to the one-inflation kernel')
    check_multi(blk, EIGHT, 'a group of 8')
    check_multi(blk, EIGHT, 'the same group again, under the hint of the first call')
    check_multi(blk, (1.4,), 'a group of 1')
    blk.free()
    blk = fresh(dense_seed_hint=0)                          # no hint: the lowest inflation goes first and alone
    check_multi(blk, (1.4, 1.1, 3.0), 'dense_seed_hint 0')
    blk.free()


def test_one_window_swizzled_slots(one_window):
    check_groupings(one_window, tri=False)


def test_three_windows_square(three_windows):
    check_groupings(three_windows, tri=False)


def test_three_windows_triangle(three_windows):
    """the upper block triangle: block rows of 2112, 2112 and a short last one, the lower blocks turned one block row at a time"""
    c = three_windows
    assert 0 < c.n - 2 * c.cap < c.cap
    check_groupings(c, tri=True)


def test_against_the_oracle(one_window, three_windows):
    """row blocks through both drivers against the oracle: indices exactly, values exactly at inflation 2.0"""
    for c, (r0, r1) in ((one_window, (one_window.n - 40, one_window.n)), (three_windows, (4200, 4240))):          # (the second crosses a block row of the plan)
        rows = c.oracle_rows(r0, r1)
        blk = c.block(r0, r1)
        got = {('alone', r): host(blk.inflate_prune(r, PRUNING)) for r in INFLATIONS}
        got.update((('multi', r), host(g)) for r, g in zip(INFLATIONS, blk.inflate_prune_multi(INFLATIONS, PRUNING)))
        blk.free()
        for (how, r), g in got.items():
            ref = ol.inflate_prune_keep(rows, r, PRUNING).to_arrays()
            assert np.array_equal(g[0], ref[0]) and np.array_equal(g[1], ref[1]), (c.n, how, r)
            if r == 2.0:
                assert np.array_equal(g[2], ref[2]), (c.n, how, r)
            assert same(g, rows_of(c.want(r), r0, r1)), (c.n, how, r)


def test_pool_overflow_is_retried_in_both_drivers(one_window):
    """With the seed hint the first attempt's survivor pool holds max(0.6 * share * nnz(L), 8 * n_rows) + n_rows entries
    (hhx_expand_dense_impl + the one-row-per-row slack of the drivers; share = 1 for all rows).  At pruning 1e-7 and inflation 1.1
    the oracle keeps more than that, so the first attempt of either driver overflows and the result below is the retry's."""
    c = one_window
    thr = 1e-7
    rows = c.oracle_rows(0, c.n)
    first_pool = max(int(0.6 * c.links.nnz), 8 * c.n) + c.n
    ref = {r: ol.inflate_prune_keep(rows, r, thr).to_arrays() for r in (1.1, 1.4)}
    for r in ref:
        assert int(ref[r][0][-1]) > first_pool, (r, int(ref[r][0][-1]), first_pool)
    blk = c.block()
    got = host(blk.inflate_prune(1.1, thr))
    blk.free()
    assert same(got, c.want(1.1, thr)), 'one-inflation driver after a pool retry'
    assert np.array_equal(got[0], ref[1.1][0]) and np.array_equal(got[1], ref[1.1][1])
    blk = c.block()
    for r, g in zip((1.1, 1.4), blk.inflate_prune_multi((1.1, 1.4), thr)):
        g = host(g)
        assert same(g, c.want(r, thr)), 'multi driver after a pool retry, inflation %r' % r
        assert np.array_equal(g[0], ref[r][0]) and np.array_equal(g[1], ref[r][1])
    blk.free()


def test_empty_and_one_row_blocks(one_window, three_windows):
    c = one_window
    empty = c.block(100, 100)
    for e in [empty.inflate_prune(2.0, PRUNING), empty.inflate_prune(1.4, PRUNING)] + empty.inflate_prune_multi((1.4, 3.0, 2.0), PRUNING):
        assert e.shape3 == (0, c.n, 0)
        e.free()
    empty.free()
    for c, row in ((one_window, 7), (three_windows, 4223)):
        blk = c.block(row, row + 1)
        for r in INFLATIONS:
            assert same(host(blk.inflate_prune(r, PRUNING)), rows_of(c.want(r), row, row + 1)), (c.n, 'alone', r)
        for r, g in zip(INFLATIONS, blk.inflate_prune_multi(INFLATIONS, PRUNING)):
            assert same(host(g), rows_of(c.want(r), row, row + 1)), (c.n, 'multi', r)
        blk.free()
