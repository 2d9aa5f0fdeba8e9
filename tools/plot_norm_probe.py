#!/usr/bin/env python3
"""Time of the device normalize_matrix of `haphic plot` (hhx_plotnorm.hip) on synthetic scaffold-bin matrices of 24 scaffolds: end to
end (upload, Knight-Ruiz balancing of every block and of the whole matrix, median, scaled matrix back on the host), and the mat-vec kernel's
achieved bytes per second against its 4 n^2 model.
usage: plot_norm_probe.py [n_bins ...]                       -> one JSON line per size (default 5000 15000 30000)
       plot_norm_probe.py --reference SCRIPTS_DIR n_bins     -> the reference's own normalize_matrix on the host, one JSON line"""
import json
import logging
import os
import platform
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_SCAFFOLDS, BIN_SIZE = 24, 100


def synthetic(n):
    """Poisson counts with a distance decay inside 24 equal scaffolds, 0.5 % single hits between them, a log-normal per-bin bias; symmetric"""
    rng = np.random.default_rng(n)
    per = n // N_SCAFFOLDS
    sizes = [per * BIN_SIZE - 1] * (N_SCAFFOLDS - 1)                        # size // bin_size + 1 == per bins each
    sizes.append((n - per * (N_SCAFFOLDS - 1)) * BIN_SIZE - 1)
    counts = np.zeros((n, n), np.int64)
    bias = rng.lognormal(0.0, 0.5, n)
    at = 0
    for s in sizes:
        m = s // BIN_SIZE + 1
        d = np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])
        lam = 40.0 / (1.0 + d) * bias[at:at + m, None] * bias[None, at:at + m]
        up = np.triu(rng.poisson(lam))
        counts[at:at + m, at:at + m] = up + np.triu(up, 1).T
        at += m
    k = int(0.0025 * n * n)
    i, j = rng.integers(0, n, k), rng.integers(0, n, k)
    far = (i // per) != (j // per)
    counts[i[far], j[far]] = 1
    counts[j[far], i[far]] = 1
    names = ['scaffold_%d' % (g + 1) for g in range(N_SCAFFOLDS)]
    return counts, names, dict(zip(names, sizes))


def device(sizes):
    from haphic_amd import _lib, plot
    plot.logger.setLevel(logging.WARNING)
    _lib.load()
    for n in sizes:
        counts, names, size_of = synthetic(n)
        plot.normalize_matrix(counts[:64, :64].copy(), names[:1], {names[0]: 6399}, BIN_SIZE, 'KR', 1.5, -1)        # first-call costs
        t0 = time.perf_counter()
        got, vmax = plot.normalize_matrix(counts, names, size_of, BIN_SIZE, 'KR', 1.5, -1)
        end_to_end = time.perf_counter() - t0
        del got
        # the whole-matrix balancing alone: the mat-vec kernel's time from its HIP events
        t0 = time.perf_counter()
        pn = _lib.PlotNorm(counts)
        upload = time.perf_counter() - t0
        pn.set_blocks([], [])
        _lib.profile_enable(True)
        _lib.profile_reset()
        t0 = time.perf_counter()
        outer, mvp, status = pn.balance()
        whole = time.perf_counter() - t0
        ms, launches = _lib.profile_get('plotnorm_matvec')
        _lib.profile_enable(False)
        pn.destroy()
        print(json.dumps({'probe': 'plot_norm', 'bins': n, 'scaffolds': N_SCAFFOLDS, 'zeros': float((counts == 0).mean()), 'vmax': float(vmax),
                          'normalize_matrix_s': end_to_end, 'upload_s': upload, 'whole_matrix_bnewt_s': whole, 'outer': int(outer[-1]),
                          'matvecs': int(mvp[-1]), 'status': int(status[-1]), 'matvec_kernel_ms': ms / max(launches, 1), 'matvec_launches_timed': launches,
                          'matvec_model_bytes': 4 * n * n, 'matvec_GBs': 4.0 * n * n * launches / (ms * 1e-3) / 1e9 if ms else None}), flush=True)


def reference(scripts, n):
    import importlib.util
    import types
    for mod in ('pysam', 'portion'):
        if mod not in sys.modules:
            m = types.ModuleType(mod)
            m.set_verbosity = lambda *a, **k: None
            m.closed = None
            sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location('_haphic_plot_reference_private', os.path.join(scripts, 'HapHiC_plot.py'))
    P = importlib.util.module_from_spec(spec)
    sys.path.insert(0, scripts)
    spec.loader.exec_module(P)
    P.logger.setLevel(logging.WARNING)
    counts, names, size_of = synthetic(n)
    t0 = time.perf_counter()
    _, vmax = P.normalize_matrix(counts, names, size_of, BIN_SIZE, 'KR', 1.5, -1)
    print(json.dumps({'probe': 'plot_norm_reference', 'stored': True, 'box': '%s, %d CPUs' % (platform.processor() or platform.machine(), os.cpu_count()),
                      'numpy': np.__version__, 'bins': n, 'scaffolds': N_SCAFFOLDS, 'normalize_matrix_s': time.perf_counter() - t0, 'vmax': float(vmax)}))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--reference':
        reference(sys.argv[2], int(sys.argv[3]))
    else:
        device([int(a) for a in sys.argv[1:]] or [5000, 15000, 30000])
