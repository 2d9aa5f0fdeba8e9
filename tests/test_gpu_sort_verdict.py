"""The verdict of `haphic sort` on the device (hhx_sort_verdict_sums, haphic_amd/csrc/hhx_sortverdict.hip) against tests/golden/sort_verdict.npz — the
sums of the reference's own find_lis for every case and rotation — as equal integers, in both forms of the kernel, and the mirror of
haphic_amd/sort.py on the device against the reference's verdicts and log lines."""
import numpy as np
import pytest

from haphic_amd import _lib, sort
from tests import sort_verdict_cases as vc

pytestmark = pytest.mark.gpu
CASES = [c.name for c in vc.cases()]
LDS_N_64 = 20479                            # the largest n whose tree of 8-byte cells fits the LDS of a CU (include/haphic_hip.h)
DEFAULT_SEAM = {4: 4095, 8: 2047}           # the largest n that takes the LDS form by default, by bytes per cell


@pytest.fixture(scope='module')
def fx():
    return vc.Fixture()


@pytest.fixture(autouse=True)
def default_seam():
    yield
    _lib.tune('sort_verdict_lds_n', None)


def inputs(fx, case):
    c = fx.case(case)
    return vc.values_of(c), [c.lens[ctg] for ctg, _ in c.fast]


@pytest.mark.parametrize('case', CASES)
def test_device_equals_the_reference(fx, case):
    value, lens = inputs(fx, case)
    n = len(value)
    whole, stats = _lib.sort_verdict_sums(value, lens, want_stats=True)
    assert whole.dtype == np.int64 and np.array_equal(whole, fx.sums(case))
    assert stats == {'lds_rotations': n - 1, 'hbm_rotations': 0, 'cell_bytes': 8 if sum(lens) >= 1 << 32 else 4}
    assert stats['cell_bytes'] == (8 if case.startswith('near_2_40') else 4)
    first, rest = _lib.sort_verdict_sums(value, lens, 0, 1), _lib.sort_verdict_sums(value, lens, 1, n - 1)
    assert first.shape == (1,) and rest.shape == (n - 2,) and np.array_equal(np.concatenate([first, rest]), fx.sums(case))


@pytest.mark.parametrize('case,seam', [('n65', 64), ('n257', 256), ('n257', 0), ('near_2_40_n65', 64), ('n1025', 1024)])
def test_the_hbm_form_gives_the_same_bits(fx, case, seam):
    """"sort_verdict_lds_n" one below n: the tree of every rotation on its scratch slab in HBM; at n itself: in LDS again"""
    value, lens = inputs(fx, case)
    n = len(value)
    _lib.tune('sort_verdict_lds_n', seam)
    got, stats = _lib.sort_verdict_sums(value, lens, want_stats=True)
    assert np.array_equal(got, fx.sums(case)) and (stats['lds_rotations'], stats['hbm_rotations']) == (0, n - 1)
    _lib.tune('sort_verdict_lds_n', n)
    got, stats = _lib.sort_verdict_sums(value, lens, want_stats=True)
    assert np.array_equal(got, fx.sums(case)) and (stats['lds_rotations'], stats['hbm_rotations']) == (n - 1, 0)


def test_the_knob_is_clamped_to_what_fits():
    """a setting past the LDS of a CU does not move the seam: n = 20480 with 8-byte cells (one contig past 2^32) stays in HBM, and takes its rotations
    there in turns; two rotations are enough to see it"""
    n = LDS_N_64 + 1
    rng = np.random.default_rng(7)
    value = (rng.permutation(n) + 1) * rng.choice([-1, 1], n)
    lens = rng.integers(1, 1000, n)
    lens[0] = 1 << 33
    _lib.tune('sort_verdict_lds_n', 1 << 40)
    got, stats = _lib.sort_verdict_sums(value, lens, 3, 5, want_stats=True)
    assert stats == {'lds_rotations': 0, 'hbm_rotations': 2, 'cell_bytes': 8}
    assert np.array_equal(got, vc.stand_in(value, lens, 3, 5))
    lens[0] = 1000                                       # 4-byte cells: the same n fits
    got, stats = _lib.sort_verdict_sums(value, lens, 3, 5, want_stats=True)
    assert stats == {'lds_rotations': 2, 'hbm_rotations': 0, 'cell_bytes': 4}
    assert np.array_equal(got, vc.stand_in(value, lens, 3, 5))


@pytest.mark.parametrize('cell_bytes', [4, 8])
def test_the_default_seam(cell_bytes):
    """the last n in LDS and the first in HBM with the knob unset; one rotation of each is enough to see the form, and its sum is the stand-in's"""
    for n, form in ((DEFAULT_SEAM[cell_bytes], 'lds_rotations'), (DEFAULT_SEAM[cell_bytes] + 1, 'hbm_rotations')):
        rng = np.random.default_rng(n)
        value = (rng.permutation(n) + 1) * rng.choice([-1, 1], n)
        lens = rng.integers(1, 1000, n) * (1 if cell_bytes == 4 else 1 << 22)
        got, stats = _lib.sort_verdict_sums(value, lens, n - 2, n - 1, want_stats=True)
        assert stats[form] == 1 and stats['cell_bytes'] == cell_bytes and stats['lds_rotations'] + stats['hbm_rotations'] == 1
        assert np.array_equal(got, vc.stand_in(value, lens, n - 2, n - 1))


@pytest.mark.parametrize('n', [300, 1025])
def test_random_signed_permutations_agree_with_the_stand_in(n):
    rng = np.random.default_rng(n)
    value = (rng.permutation(n) + 1) * rng.choice([-1, 1], n)
    lens = rng.integers(0, 1 << 20, n)
    want = vc.stand_in(value, lens)
    assert np.array_equal(_lib.sort_verdict_sums(value, lens), want)
    _lib.tune('sort_verdict_lds_n', 0)
    got, stats = _lib.sort_verdict_sums(value, lens * (1 << 20), want_stats=True)        # 8-byte cells, the HBM form
    assert stats == {'lds_rotations': 0, 'hbm_rotations': n - 1, 'cell_bytes': 8} and np.array_equal(got, want * (1 << 20))


def test_refusals_are_error_codes():
    L = _lib.load()
    sums, stats = np.zeros(8, np.int64), np.zeros(3, np.int64)

    def call(value, lens, r0=0, r1=None, n=None):
        v, ln = np.ascontiguousarray(value, np.int32), np.ascontiguousarray(lens, np.int64)
        return L.hhx_sort_verdict_sums(len(v) if n is None else n, _lib.ptr(v), _lib.ptr(ln), r0, len(v) - 1 if r1 is None else r1, _lib.ptr(sums),
                                       _lib.ptr(stats))
    assert call([1, 2, -3], [5, 5, 5]) == 0
    assert call([1], [5], 0, 0) == 1 and b'n = 1' in L.hhx_last_error()
    assert call([1, 0, 3], [5, 5, 5]) == 1 and b'value[1]' in L.hhx_last_error()
    assert call([1, -4, 3], [5, 5, 5]) == 1 and b'value[1]' in L.hhx_last_error()
    assert call([1, -2 ** 31, 3], [5, 5, 5]) == 1
    assert call([1, 2, -2], [5, 5, 5]) == 1 and b'taken' in L.hhx_last_error()
    assert call([1, 2, 3], [5, -1, 5]) == 1 and b'len[1]' in L.hhx_last_error()
    assert call([1, 2, 3], [1 << 61, 1 << 61, 0]) == 1 and b'2^62' in L.hhx_last_error()
    assert call([1, 2, 3], [1 << 62, 0, 0]) == 1 and call([1, 2, 3], [-2 ** 63, 0, 0]) == 1
    assert call([1, 2, 3], [(1 << 61) - 1, 1 << 61, 0]) == 0 and sums[0] == (1 << 62) - 1
    assert call([1, 2, 3], [5, 5, 5], 0, 3) == 1 and call([1, 2, 3], [5, 5, 5], -1, 2) == 1 and call([1, 2, 3], [5, 5, 5], 2, 1) == 1
    assert call([1, 2, 3], [5, 5, 5], 1, 1) == 0        # an empty range: nothing to do (n = 2 after its first rotation)
    assert L.hhx_sort_verdict_sums(3, None, None, 0, 2, _lib.ptr(sums), None) == 1 and b'null' in L.hhx_last_error()
    v = np.zeros(1, np.int32)
    assert L.hhx_sort_verdict_sums((1 << 18) + 1, _lib.ptr(v), _lib.ptr(sums), 0, 1, _lib.ptr(sums), None) == 2        # HHX_UNSUPPORTED, before a read
    with pytest.raises(_lib.SortVerdictUnsupported):
        _lib.sort_verdict_sums(np.zeros((1 << 18) + 1, np.int32), np.zeros((1 << 18) + 1, np.int64), 0, 1)
    with pytest.raises(RuntimeError):
        _lib.sort_verdict_sums([1, 1], [5, 5])
    with pytest.raises(RuntimeError):
        _lib.tune('sort_verdict_lds', 1)


@pytest.mark.parametrize('case', CASES)
def test_mirror_on_the_device_gives_the_golden_verdict_and_log_line(fx, case, tmp_path):
    S = vc.fake_module()
    S.compare_fast_sort_and_allhic = sort.bind_verdict(S)
    verdict, lines = vc.run_verdict(S, fx.case(case), tmp_path)
    assert verdict is fx.verdict(case) and lines == [fx.log(case)]
