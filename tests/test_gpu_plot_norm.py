"""f4, normalisation on the device (haphic_amd/csrc/hhx_plotnorm.hip behind haphic_amd.plot.normalize_matrix) against what the reference's
normalize_matrix / bnewt produced (tests/golden/plot_norm.npz).  KR results are compared within 1000 x the spread the reference's own bnewt
shows under a permutation of the matrix (floor 1e-12, tests/plot_norm_fixture.py tolerance); counts, zeros, `none` / `log10` are bit-exact."""
import logging
import types
import warnings

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


# (case, block index) -> evidence: a block whose step counts may differ from the reference's because a loop comparison of the restatement sits
# within a few ulp of its threshold at the step where the counts part (at most one of the 25 blocks).  None is needed.
STEP_COUNT_EXEMPT = {}


def _run(counts, sizes, mode, manual_vmax=-1):
    from haphic_amd import plot
    group_list, group_size_dict = nf.groups_of(sizes)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                      # np.median([]) of the one-bin case, as in the reference
        return plot.normalize_matrix(counts, group_list, group_size_dict, nf.BIN_SIZE, mode, nf.VMAX_COEF, manual_vmax)


@pytest.mark.parametrize('name', list(nf.CASES))
def test_kr_against_the_reference(golden, cases, name):
    from haphic_amd import _lib, plot
    sizes, counts = cases[name]
    tol = nf.tolerance(golden[name + '__perm_spread'])
    pn = _lib.PlotNorm(counts)
    try:
        assert pn.max == counts.max() and pn.min == counts.min() and pn.symmetric
        group_list, group_size_dict = nf.groups_of(sizes)
        pn.set_blocks(*plot.block_bounds(pn.n, group_list, group_size_dict, nf.BIN_SIZE))
        outer, mvp, status = pn.balance()
        assert not status.any()
        print(name, 'outer', outer.tolist(), 'reference', golden[name + '__outer'].tolist(), 'MVP', mvp.tolist(), 'reference A @ v', golden[name + '__mvp'].tolist())
        # the route, not only its fixed point: a wrong beta, step to the bound or rk update converges to the same x by other steps.  The
        # reference's counts do not move under a permutation of the matrix (tests/test_plot_norm.py pins the restatement to them); its
        # generator counts the very first product too, the device counts bnewt's own MVP.
        assert len(STEP_COUNT_EXEMPT) <= 1
        for k in range(len(outer)):
            if (name, k) not in STEP_COUNT_EXEMPT:
                assert outer[k] == golden[name + '__outer'][k] and mvp[k] == golden[name + '__mvp'][k] - 1, (name, k)
        x_all, x_blocks = pn.x()
    finally:
        pn.destroy()
    d_all, d_blk = nf.rel_diff(x_all, golden[name + '__x_all']), nf.rel_diff(x_blocks, golden[name + '__x_blocks'])
    print(name, 'tolerance %.3g  x_all %.3g  x_blocks %.3g' % (tol, d_all, d_blk))
    assert d_all <= tol and d_blk <= tol
    # the reference's own stopping rule on the whole matrix, recomputed on the host
    A = counts + 0.00001
    assert np.sum((1 - x_all * (A @ x_all)) ** 2) <= 1e-12 * (1 + 1e-6)
    got, vmax = _run(counts, sizes, 'KR')
    want = nf.expected_matrix(counts, sizes, golden[name + '__x_all'], golden[name + '__x_blocks'])
    assert got.dtype == np.float64 and got.shape == counts.shape and type(vmax) is np.float64
    d_m = nf.rel_diff(got, want)
    print(name, 'matrix %.3g  vmax %r  reference %r' % (d_m, vmax, golden[name + '__vmax_KR']))
    assert d_m <= tol
    assert ((got == 0) == (counts == 0)).all() and not np.signbit(got[counts == 0]).any()
    # the device's own x through the host formula: the same bits (multiplication order of d @ A @ d)
    assert got.tobytes() == nf.expected_matrix(counts, sizes, x_all, x_blocks).tobytes()
    want_vmax = golden[name + '__vmax_KR']
    # the host's median of the cells the host formula gives from the device's own x_blocks, before the zeros are restored: the same bits
    cells = nf.kr_block_cells(counts, sizes, x_blocks)
    if np.isnan(want_vmax):
        assert np.isnan(vmax) and not len(cells)
    else:
        assert abs(vmax - want_vmax) <= tol * want_vmax
        assert vmax.tobytes() == (np.median(cells) * nf.VMAX_COEF).tobytes()
    manual = _run(counts, sizes, 'KR', manual_vmax=3)
    assert manual[1] == 3 and type(manual[1]) is int and manual[0].tobytes() == got.tobytes()


@pytest.mark.parametrize('mode', ['none', 'log10'])
@pytest.mark.parametrize('name', list(nf.CASES))
def test_host_modes_are_bit_equal(golden, cases, name, mode):
    sizes, counts = cases[name]
    got, vmax = _run(counts, sizes, mode)
    want = golden['%s__vmax_%s' % (name, mode)]
    assert type(vmax) is np.float64 and vmax.tobytes() == want.tobytes()
    if mode == 'none':
        assert got is counts
    else:
        assert got.tobytes() == np.log10(counts + 1).tobytes()


def test_two_runs_give_the_same_bits(cases):
    sizes, counts = cases['n753']
    a, va = _run(counts, sizes, 'KR')
    b, vb = _run(counts, sizes, 'KR')
    assert a.tobytes() == b.tobytes() and va.tobytes() == vb.tobytes()


def test_median_select_against_numpy():
    from haphic_amd import _lib
    rng = np.random.default_rng(7)
    lists = [rng.random(100001), rng.random(100000) * 1e-300, rng.integers(0, 5, 65537).astype(np.float64), rng.integers(0, 3, 4096) * 1e-7,
             np.concatenate([np.zeros(500), rng.lognormal(0, 8, 501)]), np.array([2.5]), np.array([3.0, 1.0]), np.full(1000, 0.1),
             np.array([0.0, np.finfo(np.float64).max, 5e-324])]
    for v in lists:
        pair = _lib.select_middle(v)
        s = np.sort(v)
        assert pair.tobytes() == s[[(len(v) - 1) // 2, len(v) // 2]].tobytes()
        assert np.median(pair).tobytes() == np.median(v).tobytes()
    assert _lib.select_middle(np.zeros(0)) is None


def test_sub_block_matvec_against_numpy(cases):
    """every diagonal sub-block of the n = 110 case at every start (rows begin at any 4-byte offset) and lengths 1 ... 40"""
    from haphic_amd import _lib
    sizes, counts = cases['n110']
    A = counts + 0.00001
    rng = np.random.default_rng(11)
    pn = _lib.PlotNorm(counts)
    worst = 0.0
    try:
        spans = nf.blocks_of(sizes) + [(lo, lo + m) for lo in range(0, 9) for m in range(1, 41)] + [(0, 110), (69, 110)]
        for lo, hi in spans:
            v = rng.lognormal(0, 1, hi - lo)
            want = A[lo:hi, lo:hi] @ v
            worst = max(worst, nf.rel_diff(pn.matvec(lo, hi, v), want))
    finally:
        pn.destroy()
    print('sub-block mat-vec: worst relative difference %.3g' % worst)
    assert worst <= 1e-13


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.parametrize('name', ['n110', 'one_bin'])
def test_log_lines_through_patch_plot(golden, cases, name):
    from haphic_amd import plot
    sizes, counts = cases[name]
    keep = lambda *a, **k: None            # noqa: E731
    P = types.SimpleNamespace(parse_pairs=keep, parse_bam=keep, normalize_matrix=keep)
    plot.patch_plot(P)
    group_list, group_size_dict = nf.groups_of(sizes)
    handler = _Lines()
    plot.logger.addHandler(handler)
    level = plot.logger.level
    plot.logger.setLevel(logging.INFO)
    try:
        for mode in ('KR', 'log10', 'none'):
            handler.lines = []
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                _, vmax = P.normalize_matrix(counts, group_list, group_size_dict, nf.BIN_SIZE, mode, nf.VMAX_COEF, -1)
            want = golden['%s__log_%s' % (name, mode)].tobytes().decode().split('\n')
            if mode == 'KR' and not np.isnan(vmax):
                # the vmax line prints the float: equal up to the digits the tolerance leaves
                assert len(handler.lines) == len(want) == 2 and handler.lines[0] == want[0]
                head = 'The vmax for the KR-normalized matrix is calculated to be '
                assert handler.lines[1].startswith(head) and want[1].startswith(head) and handler.lines[1].endswith(' (1.5 * median)')
                assert handler.lines[1][:len(head) + 8] == want[1][:len(head) + 8]
            else:
                assert handler.lines == want
        handler.lines = []
        P.normalize_matrix(counts, group_list, group_size_dict, nf.BIN_SIZE, 'KR', nf.VMAX_COEF, 2)
        assert handler.lines == ['Normalizing contact mattrix using the Knight-Ruiz (KR) balancing algorithm',
                                 'The vmax for the KR-normalized matrix is manually designated as 2)']
    finally:
        plot.logger.removeHandler(handler)
        plot.logger.setLevel(level)
