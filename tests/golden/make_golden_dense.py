#!/usr/bin/env python3
"""tests/golden/dense_mcl.npz: the REFERENCE's dense mode (--dense_matrix :2723; mcl :2026-2062, prune :1999-2014, interpret_result :2065-2095,
run_mcl_clustering :2132-2242 with dense_matrix=True) on the cases of tests/dense_mcl_cases.py.

Run in the dev container only (it imports the reference at run time, as make_golden.py does):
    python tests/golden/make_golden_dense.py
Data only.  Frozen: the link matrices as edge lists; per case the reference's round count, converged flag, clusters and final matrix (as triples),
and the yardstick `ref_step_err`: the largest |f32 - f64| over the rounds of the trajectory, where both sides are the reference's own functions
applied to the same float32 state entering that round (entries that one side prunes and the other keeps are threshold flips, not round-off, and
are left out).  A case is kept only if the float64 evaluation of the same recurrence (tests/dense_mcl_cases.py) gives the reference's round count
and clusters; the dropped ones are printed.  For SEAM of the case file: every file run_mcl_clustering writes, byte for byte, and what it returns."""
import io
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}),
                    ('portion', {'closed': None, 'empty': None})):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
sys.modules['sparse_dot_mkl'] = types.ModuleType('sparse_dot_mkl')          # no dot_product_mkl in it: INTEL_MKL = False, the dense mode
sys.path.insert(0, '/root/reference/scripts')
import HapHiC_cluster as H  # noqa: E402

from tests import dense_mcl_cases as dc  # noqa: E402


def ref_mcl(pre, case):
    """the reference's mcl() -> (matrix, its log line)"""
    buf = io.StringIO()
    handler = logging.StreamHandler(buf)
    handler.setFormatter(logging.Formatter('%(message)s'))
    H.logger.addHandler(handler)
    level = H.logger.level
    H.logger.setLevel('INFO')
    try:
        out = H.mcl(pre, case.expansion, float(case.inflation), case.max_iter, case.pruning, True)
    finally:
        H.logger.setLevel(level)
        H.logger.removeHandler(handler)
    return out, buf.getvalue().strip().splitlines()[-1]


def ref_step(state, k, case):
    m = H.matrix_power(state, case.expansion) if k != 0 else state
    return H.mcl(m, case.expansion, float(case.inflation), 1, case.pruning, True)


def main():
    H.logger.setLevel('WARNING')
    out = {}
    srcs, crafted = dc.sources(), dc.crafted()
    for name, (n, i, j, cnt) in srcs.items():
        out[name + '_n'], out[name + '_i'], out[name + '_j'], out[name + '_cnt'] = np.int32(n), i.astype(np.int16), j.astype(np.int16), cnt.astype(np.uint8)
    for name, a in crafted.items():
        out[name + '_matrix'] = a
    kept = []
    for case in dc.cases():
        if case.public:
            links = None
            pre = crafted[case.source].copy()
        else:
            links = dc.matrix_from_edges(*srcs[case.source])
            pre = H.matrix_power(H.normalize(links, norm='l1', axis=0), case.expansion)          # :2144-2149
        assert pre.dtype == np.float32
        final, line = ref_mcl(pre, case)
        converged = 'has converged' in line
        rounds = int(line.split(' after ')[1].split()[0])
        assert line == dc.log_line(rounds, converged, case), (line, dc.log_line(rounds, converged, case))
        clusters = H.interpret_result(final, True)
        # the trajectory, one reference step at a time (the same calls mcl() makes: same bits), and the yardstick
        state, err = pre, 0.0
        for k in range(rounds):
            nxt = ref_step(state, k, case)
            nxt64 = ref_step(state.astype(np.float64), k, case)
            same = (nxt != 0) == (nxt64 != 0)
            if same.any():
                err = max(err, float(np.abs(nxt.astype(np.float64) - nxt64)[same].max()))
            state = nxt
        assert np.array_equal(state, final)
        # the float64 evaluation of the same recurrence must tell the same story
        src64 = crafted[case.source].astype(np.float64) if case.public else dc.pre_expand(links.astype(np.float64), case.expansion)
        m64, rounds64, conv64, _ = dc.mcl(src64, case.expansion, case.inflation, case.max_iter, case.pruning)
        c64 = dc.clusters(m64)
        ref_c = None if clusters is None else sorted(tuple(c) for c in clusters)
        if (rounds64, conv64, c64) != (rounds, converged, ref_c):
            print('DROPPED', case.name, 'reference f32:', rounds, converged, 'float64:', rounds64, conv64, 'clusters equal:', c64 == ref_c)
            continue
        t = case.name + '_'
        fi, fj = np.nonzero(final)
        out[t + 'rounds'], out[t + 'converged'], out[t + 'ref_step_err'] = np.int32(rounds), np.bool_(converged), np.float64(err)
        out[t + 'final_i'], out[t + 'final_j'], out[t + 'final_x'] = fi.astype(np.int16), fj.astype(np.int16), final[fi, fj]
        out[t + 'valid'] = np.bool_(ref_c is not None)
        flat = [x for c in (ref_c or []) for x in c]
        out[t + 'cluster_ptr'] = np.cumsum([0] + [len(c) for c in (ref_c or [])]).astype(np.int32)
        out[t + 'cluster_members'] = np.array(flat, np.int16)
        kept.append(case.name)
        print('%-28s rounds %3d converged %d clusters %s ref_step_err %.2e nnz %d' % (case.name, rounds, converged,
                                                                                   None if ref_c is None else len(ref_c), err, len(fi)))
    out['cases'] = np.array(kept)
    # the seam: run_mcl_clustering(..., dense_matrix=True) of the reference, its files and what it returns
    s = dc.SEAM
    n, i, j, cnt = srcs[s['source']]
    fa_dict, frag_index = dc.seam_inputs(n)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            rcl, nrounds = H.run_mcl_clustering(dc.matrix_from_edges(n, i, j, cnt), set(), {}, frag_index, s['expansion'], s['min_inflation'],
                                                s['max_inflation'], s['inflation_step'], s['max_iter'], s['pruning'], fa_dict, s['nchrs'], True)
        finally:
            os.chdir(cwd)
        files = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)
        for k, f in enumerate(files):
            out['seam_file%d' % k] = np.frombuffer(open(os.path.join(tmp, f), 'rb').read(), np.uint8)
        out['seam_files'] = np.array(files)
    out['seam_result'] = np.frombuffer(json.dumps([[str(infl), [[ctgs, int(length)] for ctgs, length in rc]] for infl, rc in rcl]).encode(), np.uint8)
    out['seam_nrounds'] = np.int32(nrounds)
    path = os.path.join(HERE, 'dense_mcl.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(kept), 'cases;', len(files), 'seam files')


if __name__ == '__main__':
    main()
