"""Dev container only (needs the reference checkout): tests/golden/plot_norm.npz from the reference's OWN normalize_matrix / bnewt
(HapHiC_plot.py :407-504 / :291-404) on the synthetic matrices of tests/plot_norm_fixture.py.  Data only: the counts as the int32 upper
triangle, x of the whole matrix and of the blocks, vmax of the three modes, the log lines, the normalised matrix where n <= 128, the
reference's outer-step and mat-vec counts, and perm_spread: the largest relative difference of x and of d A d between the reference's
bnewt on the matrix and on a row / column permutation of it (the same algorithm, another summation order) — the test tolerance is
1000 x that.

    python tests/golden/make_golden_plot_norm.py [reference scripts dir]
"""
import logging
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import plot_norm_fixture as nf  # noqa: E402


class Counting(np.ndarray):
    """counts the A @ v products bnewt makes"""
    products = 0

    def __matmul__(self, other):
        Counting.products += 1
        return np.asarray(self) @ other


def bnewt_counted(P, A):
    Counting.products = 0
    x, res = P.bnewt(np.ascontiguousarray(A).view(Counting), fl=1)
    return np.asarray(x), len(res), Counting.products


def spread(P, A, x, rng):
    perm = rng.permutation(len(A))
    xp, _ = P.bnewt(np.ascontiguousarray(A[np.ix_(perm, perm)]))
    back = np.empty_like(xp)
    back[perm] = xp
    a = (x[:, None] * A) * x[None, :]
    b = (back[:, None] * A) * back[None, :]
    return max(nf.rel_diff(back, x), nf.rel_diff(b, a))


class Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def main():
    P = nf.load_reference_plot(sys.argv[1] if len(sys.argv) > 1 else nf.REFERENCE_SCRIPTS)
    handler = Lines()
    P.logger.addHandler(handler)
    P.logger.propagate = False
    out = {'bin_size': np.int64(nf.BIN_SIZE), 'vmax_coef': np.float64(nf.VMAX_COEF)}
    for name, (sizes, _, _, seed) in nf.CASES.items():
        counts = nf.make_counts(name)
        n = len(counts)
        group_list, group_size_dict = nf.groups_of(sizes)
        A = counts + 0.00001
        rng = np.random.default_rng(1000 + seed)
        x_all, outer, mvp = bnewt_counted(P, A)
        outers, mvps, worst = [], [], spread(P, A, x_all, rng)
        x_blocks = np.zeros(n)
        for lo, hi in nf.blocks_of(sizes):
            sub = A[lo:hi, lo:hi]
            xg, o, m = bnewt_counted(P, sub)
            x_blocks[lo:hi] = xg
            outers.append(o)
            mvps.append(m)
            worst = max(worst, spread(P, sub, xg, rng))
        out[name + '__sizes'] = np.array(sizes, np.int64)
        out[name + '__upper'] = nf.pack_upper(counts)
        out[name + '__x_all'] = x_all
        out[name + '__x_blocks'] = x_blocks
        out[name + '__outer'] = np.array(outers + [outer], np.int64)
        out[name + '__mvp'] = np.array(mvps + [mvp], np.int64)
        out[name + '__perm_spread'] = np.float64(worst)
        for mode in ('KR', 'log10', 'none'):
            handler.lines = []
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')              # np.median([]) of the one-bin case
                matrix, vmax = P.normalize_matrix(counts.copy(), group_list, group_size_dict, nf.BIN_SIZE, mode, nf.VMAX_COEF, -1)
            assert isinstance(vmax, np.float64)
            out['%s__vmax_%s' % (name, mode)] = vmax
            out['%s__log_%s' % (name, mode)] = np.frombuffer('\n'.join(handler.lines).encode(), np.uint8)
            if mode == 'KR':
                assert np.array_equal(matrix, nf.expected_matrix(counts, sizes, x_all, x_blocks)), name
                if n <= nf.FULL_MATRIX_MAX_N:
                    out[name + '__matrix_KR'] = matrix
        zeros = float((counts == 0).mean())
        live = x_all[counts.sum(1) > 0]
        print('%-8s n %5d  zeros %.3f  x_all %.3g .. %.3g  outer %s  mvp %s  perm_spread %.2e  vmax KR %r' % (
            name, n, zeros, live.min() if len(live) else 0, live.max() if len(live) else 0, outers + [outer], mvps + [mvp], worst, out[name + '__vmax_KR']))
    path = os.path.join(HERE, 'plot_norm.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
