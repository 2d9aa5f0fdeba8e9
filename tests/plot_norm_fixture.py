"""Shared by tests/golden/make_golden_plot_norm.py and the plot-normalisation tests: the synthetic scaffold-bin matrices, the
reference's block bounds, the expected matrix rebuilt from x, and the private loader of the reference's HapHiC_plot.py."""
import importlib.util
import os
import sys
import types
from math import ceil

import numpy as np

REFERENCE_SCRIPTS = '/root/reference/scripts'
BIN_SIZE = 100
VMAX_COEF = 1.5
FULL_MATRIX_MAX_N = 128
# name -> (scaffold sizes in bp, depth, empty bins, seed)
CASES = {
    'n5': ([150, 99, 100], 3.0, 0, 1),                                  # a one-bin block, a scaffold of exactly one bin_size
    'n110': ([4000, 2500, 1000, 3000, 50], 3.0, 5, 2),                  # three multiples of bin_size: shifted blocks; five empty bins
    'n753': ([30000, 20000, 25000], 0.5, 20, 3),                        # odd n, rows longer than one wave's load
    'n2055': ([30000, 20000, 25000, 130150], 0.12, 30, 4),              # reductions over more than one workgroup; a block of 1302 bins at bin 753
    'one_bin': ([50, 60, 99, 100, 30], 3.0, 0, 5),                      # every block is one bin: the off-diagonal list is empty
}
PARAMETERS = ['contact_matrix', 'group_list', 'group_size_dict', 'bin_size', 'normalization', 'vmax_coef', 'manual_vmax']


def groups_of(sizes):
    names = ['scaffold_%d' % (k + 1) for k in range(len(sizes))]
    return names, dict(zip(names, sizes))


def n_bins(sizes, bin_size=BIN_SIZE):
    """generate_contact_matrix :127: size // bin_size + 1 bins per scaffold"""
    return sum(s // bin_size + 1 for s in sizes)


def blocks_of(sizes, bin_size=BIN_SIZE):
    """normalize_matrix :422-426: ceil(size / bin_size) consecutive bins per scaffold from bin 0"""
    out, at = [], 0
    for s in sizes:
        m = ceil(s / bin_size)
        out.append((at, at + m))
        at += m
    return out


def make_counts(name):
    """symmetric Poisson counts: distance decay inside a scaffold, a weak level between scaffolds, a log-normal per-bin bias, some empty bins"""
    sizes, depth, n_empty, seed = CASES[name]
    rng = np.random.default_rng(seed)
    n = n_bins(sizes)
    owner = np.concatenate([np.full(s // BIN_SIZE + 1, k) for k, s in enumerate(sizes)])
    pos = np.arange(n)
    same = owner[:, None] == owner[None, :]
    lam = np.where(same, depth * 20.0 / (1.0 + np.abs(pos[:, None] - pos[None, :])) ** 2, depth * 0.02)
    bias = rng.lognormal(0.0, 1.0, n)
    lam = lam * bias[:, None] * bias[None, :]
    upper = np.triu(rng.poisson(lam))
    counts = upper + np.triu(upper, 1).T
    if n_empty:
        empty = rng.choice(n, n_empty, replace=False)
        counts[empty, :] = 0
        counts[:, empty] = 0
    return counts.astype(np.int64)


def pack_upper(counts):
    return counts[np.triu_indices(counts.shape[0])].astype(np.int32)


def unpack_upper(upper, n):
    out = np.zeros((n, n), np.int64)
    out[np.triu_indices(n)] = upper
    return out + np.triu(out, 1).T


def expected_matrix(counts, sizes, x_all, x_blocks):
    """d @ A @ d with the blocks' own x inside the blocks and the zeros restored (:431-454): (x_i * A_ij) * x_j"""
    A = counts + 0.00001
    out = (x_all[:, None] * A) * x_all[None, :]
    for lo, hi in blocks_of(sizes):
        lo, hi = min(lo, len(A)), min(hi, len(A))
        xg = x_blocks[lo:hi]
        out[lo:hi, lo:hi] = (xg[:, None] * A[lo:hi, lo:hi]) * xg[None, :]
    out[counts == 0] = 0
    return out


def kr_block_cells(counts, sizes, x_blocks):
    """the list behind the KR vmax (:447-450): the off-diagonal cells (x_i * A_ij) * x_j of every block, taken BEFORE the zeros are restored (:454)"""
    A = counts + 0.00001
    cells = [((x_blocks[lo:hi, None] * A[lo:hi, lo:hi]) * x_blocks[None, lo:hi])[~np.eye(hi - lo, dtype=bool)] for lo, hi in blocks_of(sizes)]
    return np.concatenate(cells)


def load_cases(golden):
    """name -> (sizes, read-only int64 counts) of the stored cases"""
    out = {}
    for name in CASES:
        sizes = golden[name + '__sizes'].tolist()
        counts = unpack_upper(golden[name + '__upper'], n_bins(sizes))
        counts.setflags(write=False)
        out[name] = (sizes, counts)
    return out


def tolerance(perm_spread):
    """1000 x the spread the reference's own bnewt shows under a permutation of the rows and columns, at least 1e-12"""
    return max(1000.0 * float(perm_spread), 1e-12)


def rel_diff(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.maximum(np.abs(want), np.finfo(np.float64).tiny)
    return float(np.max(np.abs(got - want) / scale)) if got.size else 0.0


def bnewt(A, tol=1e-6, delta=0.1, Delta=3, g=0.9, etamax=0.1):
    """numpy restatement of bnewt :291-404 in the precision of A -> (x, outer steps, mat-vec count MVP, lower exits, upper exits): how often an
    inner loop left through the `delta` bound (:367-371) and through the `Delta` bound (:372-376).  MVP is the reference's own counter: its first
    product v = x * (A @ x) is not in it."""
    n = A.shape[0]
    x, eta, rt, MVP, nn, lower, upper = np.ones(n, A.dtype), etamax, tol ** 2, 0, 0, 0, 0
    v = x * (A @ x)
    rk = 1 - v
    rho_km1 = rout = rold = rk @ rk
    while rout > rt:
        nn += 1
        assert nn <= 1000
        k, y, innertol = 0, np.ones(n, A.dtype), max(eta ** 2 * rout, rt)
        while rho_km1 > innertol:
            k += 1
            assert k <= 10000
            if k == 1:
                Z = rk / v
                p = Z
                rho_km1 = rk @ Z
            else:
                p = Z + (rho_km1 / rho_km2) * p
            w = x * (A @ (x * p)) + v * p
            alpha = rho_km1 / (p @ w)
            ap = alpha * p
            ynew = y + ap
            if ynew.min() <= delta:
                ind = ap < 0
                y = y + ((delta - y[ind]) / ap[ind]).min() * ap
                lower += 1
                break
            if ynew.max() >= Delta:
                ind = ynew > Delta
                y = y + ((Delta - y[ind]) / ap[ind]).min() * ap
                upper += 1
                break
            y, rk, rho_km2 = ynew, rk - alpha * w, rho_km1
            Z = rk / v
            rho_km1 = rk @ Z
        x = x * y
        v = x * (A @ x)
        rk = 1 - v
        rho_km1 = rout = rk @ rk
        MVP += k + 1
        rat, rold, eta_o = rout / rold, rout, eta
        eta = g * rat
        if g * eta_o ** 2 > 0.1:
            eta = max(eta, g * eta_o ** 2)
        eta = max(min(eta, etamax), tol * 0.5 / np.sqrt(rout))
    return x, nn, MVP, lower, upper


def load_reference_plot(scripts=REFERENCE_SCRIPTS, name='_haphic_plot_reference_private'):
    """HapHiC_plot.py under a private module name (the cached `HapHiC_plot` may carry the product's seams); pysam / portion stubbed"""
    from oracle.plot_oracle import Closed             # the stand-in tests/test_plot.py installs, should this run first
    for mod, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': Closed})):
        if mod not in sys.modules:
            m = types.ModuleType(mod)
            m.__dict__.update(attrs)
            sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, 'HapHiC_plot.py'))
    module = importlib.util.module_from_spec(spec)
    sys.path.insert(0, scripts)
    try:
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(scripts)
    return module
