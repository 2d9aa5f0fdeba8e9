"""f4, normalisation: the host side of haphic_amd.plot.normalize_matrix (HapHiC_plot.py normalize_matrix :407-504, bnewt :291-404)
and the fixture tests/golden/plot_norm.npz (make_golden_plot_norm.py), without a GPU."""
import inspect
import os
import re
import types

import numpy as np
import pytest

from tests import plot_norm_fixture as nf
from tests.conftest import ROOT, load_golden

SYMBOLS = ('hhx_plotnorm_create', 'hhx_plotnorm_set_blocks', 'hhx_plotnorm_balance', 'hhx_plotnorm_fetch_x', 'hhx_plotnorm_apply',
           'hhx_plotnorm_median', 'hhx_plotnorm_matvec', 'hhx_plotnorm_destroy', 'hhx_select_middle_u64')


@pytest.fixture(scope='module')
def golden():
    return load_golden('plot_norm.npz')


def test_header_bindings_and_exports_carry_plotnorm():
    from haphic_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'haphic_hip.h')).read()
    assert 'HapHiC_plot.py bnewt :291-404' in header and ':407-504' in header
    lib = _lib.load()
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(lib, sym) and re.search(r'\b%s\s*\(' % sym, header), sym
    assert hasattr(_lib, 'PlotNorm') and hasattr(_lib, 'select_middle')
    # null handles come back as an error code
    out = np.zeros(4, np.int64)
    assert lib.hhx_plotnorm_balance(None, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out)) != 0 and b'null' in lib.hhx_last_error()
    assert lib.hhx_plotnorm_apply(None, _lib.ptr(out)) != 0 and lib.hhx_plotnorm_set_blocks(None, 0, None, None) != 0
    assert lib.hhx_plotnorm_destroy(None) == 0


def test_normalize_matrix_has_the_reference_parameters():
    from haphic_amd import plot
    want = nf.PARAMETERS
    if os.path.isdir(nf.REFERENCE_SCRIPTS):
        P = nf.load_reference_plot()
        assert list(inspect.signature(P.normalize_matrix).parameters) == want
    assert list(inspect.signature(plot.normalize_matrix).parameters) == want


class StubNorm:
    """records what normalize_matrix asks of the device; answers with numpy"""
    calls = []

    def __init__(self, matrix):
        StubNorm.calls.append('create')
        self.n, self.matrix = matrix.shape[0], np.asarray(matrix)
        self.max, self.min, self.symmetric = int(matrix.max()), int(matrix.min()), True

    def set_blocks(self, lo, hi):
        StubNorm.calls.append('set_blocks')
        self.blocks = list(zip(lo.tolist(), hi.tolist()))

    def middle(self, kr):
        StubNorm.calls.append('middle')
        assert not kr
        vals = np.sort(np.concatenate([self.matrix[lo:hi, lo:hi][~np.eye(hi - lo, dtype=bool)] for lo, hi in self.blocks] or [np.zeros(0, np.int64)]))
        n = len(vals)
        return n, (vals[[(n - 1) // 2, n // 2]].astype(np.int64) if n else np.zeros(2, np.int64))

    def destroy(self):
        StubNorm.calls.append('destroy')


@pytest.fixture
def stub_lib(monkeypatch):
    from haphic_amd import plot
    StubNorm.calls = []
    monkeypatch.setattr(plot, '_lib', types.SimpleNamespace(load=lambda: None, PlotNorm=StubNorm))
    return StubNorm


def _stub_module():
    seen = []

    def original(*args):
        seen.append(args)
        return 'original', len(seen)
    keep = lambda *a, **k: None            # noqa: E731
    return types.SimpleNamespace(parse_pairs=keep, parse_bam=keep, normalize_matrix=original), original, seen


def test_patch_plot_rebinds_normalize_matrix_and_saved_restores_it(stub_lib):
    from haphic_amd import plot
    P, original, _ = _stub_module()
    saved = plot.patch_plot(P)
    assert set(saved) == {'parse_pairs', 'parse_bam', 'normalize_matrix'} and saved['normalize_matrix'] is original
    assert P.parse_pairs is plot.parse_pairs and P.parse_bam is plot.parse_bam
    assert P.normalize_matrix is not original and P.normalize_matrix.__wrapped__ is plot.normalize_matrix
    assert list(inspect.signature(P.normalize_matrix).parameters) == nf.PARAMETERS
    for name, fn in saved.items():
        setattr(P, name, fn)
    assert P.normalize_matrix is original


@pytest.mark.parametrize('what', ['float', 'two_to_31', 'negative', 'not_square', 'empty', 'not_an_array'])
@pytest.mark.parametrize('mode', ['KR', 'none'])
def test_unsupported_input_goes_to_the_original(stub_lib, what, mode):
    from haphic_amd import plot
    m = np.arange(16, dtype=np.int64).reshape(4, 4)
    m = m + m.T
    if what == 'float':
        m = m.astype(np.float64)
    elif what == 'two_to_31':
        m[1, 2] = m[2, 1] = 2 ** 31
    elif what == 'negative':
        m[0, 3] = m[3, 0] = -1
    elif what == 'not_square':
        m = m[:3]
    elif what == 'empty':
        m = m[:0, :0]
    else:
        m = m.tolist()
    P, original, seen = _stub_module()
    plot.patch_plot(P)
    args = (m, ['a'], {'a': 250}, 100, mode, 1.5, -1)
    assert P.normalize_matrix(*args) == ('original', 1)
    assert len(seen) == 1 and all(a is b for a, b in zip(seen[0], args))
    assert 'middle' not in stub_lib.calls and stub_lib.calls.count('create') == stub_lib.calls.count('destroy')
    # called directly there is no original to hand back to: an error, never a quiet host computation
    with pytest.raises(RuntimeError, match='reference normalize_matrix'):
        plot.normalize_matrix(*args)


@pytest.mark.parametrize('mode', ['log10', 'none'])
def test_manual_vmax_makes_no_device_call(stub_lib, mode, caplog):
    from haphic_amd import plot
    m = np.arange(25, dtype=np.int64).reshape(5, 5)
    with caplog.at_level('INFO', logger=plot.logger.name):
        got, vmax = plot.normalize_matrix(m, ['a', 'b'], {'a': 250, 'b': 100}, 100, mode, 1.5, 7)
    assert stub_lib.calls == [] and vmax == 7 and type(vmax) is int
    assert (got is m) if mode == 'none' else np.array_equal(got, np.log10(m + 1))
    what = 'log-normalized' if mode == 'log10' else 'raw'
    assert caplog.messages[-1] == 'The vmax for the %s matrix is manually designated as 7' % what


@pytest.mark.parametrize('mode', ['log10', 'none'])
@pytest.mark.parametrize('name', list(nf.CASES))
def test_host_modes_on_the_stub_match_the_reference(stub_lib, golden, name, mode):
    """log10 / none: the matrix is the host's numpy expression, vmax comes from the two middle counts: bit-equal to the reference's vmax"""
    import warnings
    from haphic_amd import plot
    sizes = golden[name + '__sizes'].tolist()
    counts = nf.unpack_upper(golden[name + '__upper'], nf.n_bins(sizes))
    group_list, group_size_dict = nf.groups_of(sizes)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got, vmax = plot.normalize_matrix(counts, group_list, group_size_dict, nf.BIN_SIZE, mode, nf.VMAX_COEF, -1)
    want = golden['%s__vmax_%s' % (name, mode)]
    assert type(vmax) is np.float64 and vmax.tobytes() == want.tobytes()
    assert stub_lib.calls == ['create', 'set_blocks', 'middle', 'destroy']
    assert (got is counts) if mode == 'none' else (got.dtype == np.float64 and np.array_equal(got, np.log10(counts + 1)))


def test_block_bounds_are_the_reference_ones():
    from haphic_amd import plot
    for name, (sizes, _, _, _) in nf.CASES.items():
        group_list, group_size_dict = nf.groups_of(sizes)
        lo, hi = plot.block_bounds(nf.n_bins(sizes), group_list, group_size_dict, nf.BIN_SIZE)
        assert list(zip(lo.tolist(), hi.tolist())) == nf.blocks_of(sizes)
    lo, hi = plot.block_bounds(5, *nf.groups_of([150, 99, 100]), 100)
    assert lo.tolist() == [0, 2, 3] and hi.tolist() == [2, 3, 4]          # the 100 bp scaffold owns two bins of the matrix, one of its block
    lo, hi = plot.block_bounds(3, *nf.groups_of([250, 250]), 100)         # a matrix smaller than its AGP claims: clipped as numpy clips a slice
    assert lo.tolist() == [0, 3] and hi.tolist() == [3, 3]


@pytest.mark.parametrize('name', list(nf.CASES))
def test_fixture_self_check(golden, name):
    """the stored x against the restatement of bnewt (plot_norm_fixture.bnewt), within the case's tolerance; the expected-matrix helper the GPU tests use against
    the reference's own matrix, bit for bit, where it is stored"""
    sizes = golden[name + '__sizes'].tolist()
    assert sizes == nf.CASES[name][0] and int(golden['bin_size']) == nf.BIN_SIZE and float(golden['vmax_coef']) == nf.VMAX_COEF
    n = nf.n_bins(sizes)
    counts = nf.unpack_upper(golden[name + '__upper'], n)
    assert np.array_equal(counts, nf.make_counts(name)) and np.array_equal(counts, counts.T)
    tol = nf.tolerance(golden[name + '__perm_spread'])
    assert 1e-12 <= tol < 1e-9
    A = counts + 0.00001
    x_all, x_blocks = golden[name + '__x_all'], golden[name + '__x_blocks']
    x, outer, mvp, _, _ = nf.bnewt(A)
    assert nf.rel_diff(x, x_all) <= tol
    steps = [(outer, mvp)]
    for lo, hi in nf.blocks_of(sizes):
        xg, o, m, _, _ = nf.bnewt(A[lo:hi, lo:hi])
        assert nf.rel_diff(xg, x_blocks[lo:hi]) <= tol
        steps.insert(-1, (o, m))
    print(name, 'outer / MVP (restatement):', steps, ' reference outer:', golden[name + '__outer'].tolist())
    owned = np.zeros(n, bool)
    for lo, hi in nf.blocks_of(sizes):
        owned[lo:hi] = True
    assert not x_blocks[~owned].any() and (x_blocks[owned] > 0).all()
    want = nf.expected_matrix(counts, sizes, x_all, x_blocks)
    if n <= nf.FULL_MATRIX_MAX_N:
        assert want.tobytes() == golden[name + '__matrix_KR'].tobytes()
    else:
        assert name + '__matrix_KR' not in golden
    assert ((want == 0) == (counts == 0)).all()
    # vmax of the KR mode: the median is taken BEFORE the zeros are restored (:447-450 runs before :454)
    cells = nf.kr_block_cells(counts, sizes, x_blocks)
    want_vmax = golden[name + '__vmax_KR']
    if len(cells):
        assert (np.median(cells) * nf.VMAX_COEF).tobytes() == want_vmax.tobytes()
    else:
        assert np.isnan(want_vmax)


# the blocks whose restated bnewt leaves an inner loop through the lower bound (ynew.min() <= delta :367); (lo, hi) of the whole matrix is (0, n)
LOWER_EXIT_BLOCKS = {('n753', (500, 750)), ('n2055', (0, 300)), ('n2055', (300, 500)), ('n2055', (500, 750)), ('n2055', (750, 2052)), ('n2055', (0, 2055))}
SMALL_PATH_MAX = 512            # PN_SMALL of csrc/hhx_plotnorm.hip: larger blocks, and every whole matrix, take the host-steered loop


def test_fixture_reaches_both_exits_on_both_paths(golden):
    """what the GPU tests rely on: the restatement's step counts are the stored ones for every block (outer == __outer, MVP == __mvp - 1: the
    generator's counter sees the very first product too), and both early exits of the inner loop are taken by a block of the one-workgroup
    path and by one of the host-steered path"""
    lower, upper, n_blocks = set(), set(), 0
    for name, (sizes, counts) in nf.load_cases(golden).items():
        A = counts + 0.00001
        spans = nf.blocks_of(sizes) + [(0, len(A))]
        for k, (lo, hi) in enumerate(spans):
            _, outer, mvp, n_lower, n_upper = nf.bnewt(A[lo:hi, lo:hi])
            assert outer == golden[name + '__outer'][k] and mvp == golden[name + '__mvp'][k] - 1, (name, lo, hi)
            grid = hi - lo > SMALL_PATH_MAX or k == len(spans) - 1
            if n_lower:
                lower.add((name, (lo, hi)))
            if n_upper:
                upper.add((name, (lo, hi), grid))
            n_blocks += 1
    assert n_blocks == 25 and lower == LOWER_EXIT_BLOCKS
    both = {(name, span, grid) for name, span, grid in upper if (name, span) in lower}
    assert ('n753', (500, 750), False) in both                                  # a block of at most 512 bins
    assert ('n2055', (750, 2052), True) in both and ('n2055', (0, 2055), True) in both           # a large block and a whole matrix
    for name in ('n110', 'n753'):                                               # the cases the path tests run through both implementations
        assert any(u[0] == name and not u[2] for u in upper) and any(u[0] == name and u[2] for u in upper)
