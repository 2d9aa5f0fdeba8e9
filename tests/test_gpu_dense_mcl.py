"""--dense_matrix Markov clustering on the device (csrc/hhx_densemcl.hip) against the reference's dense mode (tests/golden/dense_mcl.npz) and the
float64 host model of tests/dense_mcl_cases.py.

The step test compares every round of every case with the float64 evaluation of that round FROM THE DEVICE'S OWN STATE, so the only difference
is one round's round-off.  Bound: 4 x ref_step_err[case], the reference's own float32-vs-float64 difference per round (0.9e-7 ... 3.8e-7 on
these cases): the kernel's sum is one sequential fmaf chain of length n where BLAS adds blocked partial sums (0.75-1.5e-7 x sum|ab| for chains
up to K = 1024, sum|ab| <= 1 for column-stochastic operands).  An entry whose float64 pre-prune value lies within that bound of `pruning` may
be kept by one side and pruned by the other; such a flip rescales the rest of its column by up to `pruning`, which is no round-off of the
other entries: the float64 round therefore takes the device's decision for the entries INSIDE the band (and only those), after which every
entry of the matrix, the band included, has to agree within the bound.  Outside the band the zero pattern must be identical."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

from tests import dense_mcl_cases as dc
from tests.conftest import load_golden
from tests.test_dense_mcl_cpu import clusters_of, final_of, source_of

pytestmark = pytest.mark.gpu

BAND_SHARE_MAX = 0.05


@pytest.fixture(scope='module')
def golden():
    return load_golden('dense_mcl.npz')


@pytest.fixture(scope='module')
def lib():
    from haphic_amd import _lib
    _lib.load()
    return _lib


def device_pre(lib, golden, case):
    """the matrix mcl() starts from, formed on the device as run_mcl_clustering forms it (:2144-2149) -> DenseMatrix"""
    src = source_of(golden, case)
    if case.public:
        return lib.DenseMatrix.from_numpy(src)
    links = lib.DenseMatrix.from_numpy(dc.matrix_from_edges(*src))
    try:
        lib.dmat_normalize_l1(links)
        return lib.dmat_power(links, case.expansion)
    finally:
        links.free()


# ------------------------------------------------------------------ 1. the product
@pytest.mark.parametrize('n', [1, 2, 31, 32, 33, 97, 129, 300, 513])
def test_gemm_is_the_exact_integer_product(lib, n):
    """small integers: every partial sum is exact in float32, so any k order gives the integer product bit for bit; A and B are not symmetric, so a
    swapped row / column or a wrong lane map cannot pass"""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 8, (n, n)).astype(np.float32)
    b = rng.integers(0, 8, (n, n)).astype(np.float32)
    b[0, n - 1] = 7.0
    if n > 1:
        b[n - 1, 0] = 0.0
        a[0, n - 1], a[n - 1, 0] = 0.0, 5.0
    want = (a.astype(np.int64) @ b.astype(np.int64)).astype(np.float32)
    assert want.max() < 2 ** 24
    da, db, eye = lib.DenseMatrix.from_numpy(a), lib.DenseMatrix.from_numpy(b), lib.DenseMatrix.from_numpy(np.eye(n, dtype=np.float32))
    try:
        assert np.array_equal(da.to_numpy(), a) and da.shape == (n, n)
        outs = [lib.dmat_gemm(da, db), lib.dmat_gemm(da, db), lib.dmat_gemm(eye, db), lib.dmat_gemm(da, eye)]
        got = [o.to_numpy() for o in outs]
        for o in outs:
            o.free()
        assert np.array_equal(got[0], want)
        assert got[0].tobytes() == got[1].tobytes()                 # the same product twice: the same bits
        assert np.array_equal(got[2], b) and np.array_equal(got[3], a)
        p3 = lib.dmat_power(da, 3)                                  # (a @ a) @ a, exact as well while it stays below 2^24
        small = (a.astype(np.int64) @ a.astype(np.int64)) @ a.astype(np.int64)
        if small.max() < 2 ** 24:
            assert np.array_equal(p3.to_numpy(), small.astype(np.float32))
        p3.free()
    finally:
        da.free(), db.free(), eye.free()


def test_power_follows_numpys_association_order(lib):
    """matrix_power on stochastic operands: expansion 1..6 against the float64 model in the same order"""
    m = dc.normalize_l1(dc.matrix_from_edges(*dc.sources()['planted33']))
    d = lib.DenseMatrix.from_numpy(m)
    try:
        for e in (1, 2, 3, 4, 5, 6):
            p = lib.dmat_power(d, e)
            got = p.to_numpy()
            p.free()
            assert np.abs(got - dc.matrix_power(m.astype(np.float64), e)).max() <= 4 * 1.5e-7      # chains of K = 33 on sum|ab| <= 1, a few products deep
    finally:
        d.free()


# ------------------------------------------------------------------ 2. one round at a time
def f64_round_with_band(state, k, case, dev_next, half):
    """round k in float64 from `state`; inside the band of half-width `half` around the threshold the device's keep / prune decision is taken.
    -> (float64 result, band mask)"""
    _, q = dc.step(state, k, case.expansion, case.inflation, case.pruning, want_pre_prune=True)
    thr = float(np.float32(case.pruning))
    band = np.abs(q - thr) <= half
    keep = q >= thr
    keep[q.argmax(axis=0), np.arange(q.shape[1])] = True
    keep = np.where(band, dev_next != 0, keep)
    return dc.normalize_l1(np.where(keep, q, 0.0)), band


@pytest.mark.parametrize('case', dc.cases(), ids=repr)
def test_every_round_matches_float64_from_the_same_state(lib, golden, case):
    err = float(golden[case.name + '_ref_step_err'])
    tol = 4 * err
    rounds = int(golden[case.name + '_rounds'])
    cur = device_pre(lib, golden, case)
    worst, worst_band = 0.0, 0.0
    try:
        for k in range(rounds):
            state = cur.to_numpy()
            nxt, n_iter, conv = lib.dmat_mcl(cur, case.expansion, case.inflation, k + 1, case.pruning, done=k)
            assert n_iter == k + 1 and not conv                      # a resumed call has no last_matrix
            cur.free()
            cur = nxt
            got = cur.to_numpy()
            want, band = f64_round_with_band(state.astype(np.float64), k, case, got, tol)
            assert np.array_equal((got != 0)[~band], (want != 0)[~band]), 'zero pattern differs outside the band in round %d' % k
            worst = max(worst, float(np.abs(got - want).max()))
            worst_band = max(worst_band, float(band.mean()))
        print('%s: worst |device - f64| %.3e, bound %.3e, largest band share %.4f' % (case.name, worst, tol, worst_band))
        assert worst <= tol
        assert worst_band <= BAND_SHARE_MAX
    finally:
        cur.free()


# ------------------------------------------------------------------ 3. whole runs through the public mirrors
@pytest.mark.parametrize('case', dc.cases(), ids=repr)
def test_whole_run_gives_the_references_rounds_clusters_and_matrix(lib, golden, case, caplog):
    from haphic_amd import cluster
    pre = device_pre(lib, golden, case)
    try:
        pre_np = pre.to_numpy()
    finally:
        pre.free()
    with caplog.at_level(logging.INFO, logger=cluster.logger.name):
        res = cluster.mcl(pre_np, case.expansion, case.inflation, case.max_iter, case.pruning, True)
    assert isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == pre_np.shape
    lines = [r.getMessage() for r in caplog.records if 'rounds of iterations' in r.getMessage()]
    assert lines == [dc.log_line(int(golden[case.name + '_rounds']), bool(golden[case.name + '_converged']), case)]
    got = cluster.interpret_result(res, True)
    want = clusters_of(golden, case)
    assert (got is None) == (want is None)
    if want is not None:
        assert set(got) == set(want)
    ref = final_of(golden, case, res.shape[0])
    diff = float(np.abs(res.astype(np.float64) - ref).max())
    print('%s: final matrix |device - reference| %.3e, bound %.3e' % (case.name, diff, 4 * float(golden[case.name + '_ref_step_err'])))
    assert np.array_equal(res != 0, ref != 0)
    assert diff <= 4 * float(golden[case.name + '_ref_step_err'])


def test_zero_column_goes_through_the_public_mcl(lib, golden):
    from haphic_amd import cluster
    z = golden['zerocol12_matrix']
    res = cluster.mcl(z, 2, 2.0, 200, dc.PRUNING, True)
    assert np.isfinite(res).all() and not res[:, 5].any()


# ------------------------------------------------------------------ 4. the seam
def seam_run(cluster, golden, link_matrix, outdir):
    s = dc.SEAM
    fa_dict, frag_index = dc.seam_inputs(int(golden[s['source'] + '_n']))
    return cluster.run_mcl_clustering(link_matrix, set(), {}, frag_index, s['expansion'], s['min_inflation'], s['max_inflation'], s['inflation_step'],
                                      s['max_iter'], s['pruning'], fa_dict, s['nchrs'], True, outdir_root=str(outdir))


@pytest.mark.parametrize('resident', [False, True], ids=['ndarray', 'resident'])
def test_run_mcl_clustering_writes_the_references_files(lib, golden, tmp_path, resident):
    import scipy.sparse as sp
    from haphic_amd import cluster
    s = dc.SEAM
    links = dc.matrix_from_edges(*source_of(golden, dc.Case('seam', s['source'], s['expansion'], 2.0)))
    arg = cluster.ResidentMatrix(lib.DeviceCSR.from_scipy_csc(sp.csc_matrix(links))) if resident else links
    rcl, nrounds = seam_run(cluster, golden, arg, tmp_path)
    assert nrounds == int(golden['seam_nrounds'])
    want = json.loads(bytes(golden['seam_result']).decode())
    assert [[str(infl), [[list(ctgs), int(length)] for ctgs, length in rc]] for infl, rc in rcl] == want
    files = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert files == golden['seam_files'].tolist() and len(files) > 3
    for k, f in enumerate(files):
        assert open(os.path.join(str(tmp_path), f), 'rb').read() == bytes(golden['seam_file%d' % k]), f


def test_frozen_table_stays_in_hbm_when_the_dense_seam_is_bound(lib, tmp_path, monkeypatch):
    """dict_to_matrix(..., dense_matrix=True, add_self_loops=True) on a frozen flank table (run() :2934): the ndarray by default, the
    ResidentMatrix of the sparse mode with the dense seam bound; run_mcl_clustering gives the same clusters from either"""
    from haphic_amd import cluster
    from tests.test_seam_containers import _args, _case, _s5
    gen, fa_dict, aln = _case()
    _full, flank, _ht, _clm, _frag_link, _coord, _ctg_len, nx = _s5(fa_dict, aln, _args())
    assert flank.frozen
    dense, idx = cluster.dict_to_matrix(flank, nx, dense_matrix=True, add_self_loops=True)
    assert isinstance(dense, np.ndarray) and flank.frozen
    monkeypatch.setattr(cluster, 'DENSE_SEAM_BOUND', True)
    plain, idx_plain = cluster.dict_to_matrix(flank, nx, dense_matrix=True, add_self_loops=False)       # the filters' form: still the ndarray
    assert isinstance(plain, np.ndarray) and idx_plain == idx
    resident, idx2 = cluster.dict_to_matrix(flank, nx, dense_matrix=True, add_self_loops=True)
    assert isinstance(resident, cluster.ResidentMatrix) and idx2 == idx and list(idx2) == list(idx) and flank.frozen
    assert np.array_equal(resident.toarray(), dense)
    common = (set(), {}, idx, 2, 1.5, 2.5, 0.5, 200, 1e-4, fa_dict, 3, True)
    (tmp_path / 'a').mkdir(), (tmp_path / 'b').mkdir()
    got_a = cluster.run_mcl_clustering(dense, *common, outdir_root=str(tmp_path / 'a'))
    got_b = cluster.run_mcl_clustering(resident, *common, outdir_root=str(tmp_path / 'b'))
    assert got_a == got_b and got_a[1] == 3 and len(got_a[0]) >= 1
    for d, _, fs in os.walk(str(tmp_path / 'a')):
        for f in fs:
            rel = os.path.relpath(os.path.join(d, f), str(tmp_path / 'a'))
            assert open(os.path.join(d, f), 'rb').read() == open(os.path.join(str(tmp_path / 'b'), rel), 'rb').read()


@pytest.mark.parametrize('name', ['planted33', 'planted97'])
def test_prune_and_csr_round_trip(lib, golden, name):
    from haphic_amd import cluster
    m = dc.normalize_l1(dc.matrix_from_edges(int(golden[name + '_n']), golden[name + '_i'].astype(np.int64), golden[name + '_j'].astype(np.int64),
                                             golden[name + '_cnt'].astype(np.float32)))
    m = (m @ m).astype(np.float32)                                   # entries on both sides of the threshold
    p = 2e-3
    got = cluster.prune(m, p, True)
    want = dc.prune(m.astype(np.float64), p)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got != 0, want != 0) and (got == 0).any()
    # one float32 sum of at most n <= 97 terms (a chain of one per thread, then a tree of depth 8) and one division: below 8 eps of values <= 1
    assert np.abs(got - want).max() <= 8 * np.finfo(np.float32).eps
    d = lib.DenseMatrix.from_numpy(got)
    csr = d.to_csr()
    back = lib.DenseMatrix.from_csr(csr)
    try:
        assert np.array_equal(csr.to_scipy_csc().toarray(), got)
        assert csr.nnz == int((got != 0).sum())
        assert back.to_numpy().tobytes() == got.tobytes()
        twice = lib.dmat_gemm(back, d)                               # the block rebuilt from CSR keeps the padding invariant: same product, same bits
        ref = lib.dmat_gemm(d, d)
        assert twice.to_numpy().tobytes() == ref.to_numpy().tobytes()
        twice.free(), ref.free()
    finally:
        d.free(), csr.free(), back.free()
    tie = golden['tie8_matrix']
    assert np.array_equal(cluster.prune(tie, 0.3, True), dc.prune(tie, 0.3))      # dyadic: exact, and the first of the tied maxima comes back


# ------------------------------------------------------------------ 5. ABI
def test_null_handles_are_errors_not_crashes(lib):
    L = lib.load()
    o, n_iter, conv = C.c_void_p(), C.c_int(0), C.c_int(0)
    buf = np.zeros(4, np.float32)
    calls = [lambda: L.hhx_dmat_from_host(2, None, C.byref(o)), lambda: L.hhx_dmat_from_host(2, lib.ptr(buf), None),
             lambda: L.hhx_dmat_from_csr(None, C.byref(o)), lambda: L.hhx_dmat_to_host(None, lib.ptr(buf)), lambda: L.hhx_dmat_to_csr(None, C.byref(o)),
             lambda: L.hhx_dmat_copy(None, C.byref(o)), lambda: L.hhx_dmat_shape(None, None, None, None), lambda: L.hhx_dmat_gemm(None, None, C.byref(o)),
             lambda: L.hhx_dmat_normalize_l1(None), lambda: L.hhx_dmat_prune(None, 1e-4, C.byref(o)), lambda: L.hhx_dmat_power(None, 2, C.byref(o)),
             lambda: L.hhx_dmat_mcl(None, 0, 2, 2.0, 10, 1e-4, C.byref(o), C.byref(n_iter), C.byref(conv))]
    for call in calls:
        assert call() != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_dmat_free(None) == 0
    assert L.hhx_dmat_from_host(0, lib.ptr(buf), C.byref(o)) != 0 and b'at least one row' in L.hhx_last_error()
    d = lib.DenseMatrix.from_numpy(np.eye(3, dtype=np.float32))
    try:
        assert L.hhx_dmat_power(d.h, 0, C.byref(o)) != 0 and L.hhx_dmat_mcl(d.h, -1, 2, 2.0, 10, 1e-4, C.byref(o), C.byref(n_iter), C.byref(conv)) != 0
        assert d.nbytes == 128 * 128 * 4
    finally:
        d.free()
