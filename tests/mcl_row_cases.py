"""The row epilogue of one Markov-clustering iteration — inflate, normalise, prune, normalise, test convergence — as a plain numpy
float64 model on CSR triples, and the rows at which an implementation of it can go wrong unnoticed: a row maximum below the
threshold (restored), tied maxima (the first one is restored), a value exactly equal to the threshold (kept), empty and all-zero
rows, row lengths around the 64-lane wave and the 256-thread workgroup, more rows than one pass of the row grid, convergence
operands whose patterns differ.

The arithmetic is specified exactly (float32 x*x, float64 row sums, float(double / double)), so wherever every row sum is exact in
float64 whatever the order of the additions (exact_sums) the model predicts the bits of every implementation.  The generators
below prove that on the CPU for what the tests compare byte for byte: the inflated values, the first-normalised values and the
survivors.  No GPU and no oracle needed here."""
import itertools

import numpy as np

THRESHOLDS = (0.5, 2.0 ** -6, 2.0 ** -10, 1e-4)
INFLATIONS = (2.0, 1.5, 3.0)
ULP = 2.0 ** -23
INFLATE_RTOL = 3 * ULP          # after inflate + normalise at an inflation other than 2: the device forms float(exp2(r log2 x)) in float64,
#                                 the model float(pow): one float32 ulp (2^-23) apart at most per inflated value; the row sum inherits
#                                 2^-23 and the division adds a rounding of 2^-24
PRUNE_RTOL = 6 * ULP            # after the second normalisation (7.2e-7)
MARGIN = 8 * ULP                # no decision (>= threshold, row maximum) of a bounded comparison hangs on less than this

N_COLS = 5000
EDGE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
TIE_POSITIONS = (0, 1, 31, 32, 63, 64, 65, 127, 128, 199)
TRIPLE_POSITIONS = ((5, 69, 133), (63, 64, 65), (199, 0, 100))
TALL_ROWS = 2 * 32768 + 5       # the row grid is capped at 8192 workgroups x 4 rows: a second and a third pass


# ---------------------------------------------------------------- the model
def _segments(p):
    """(start of every non-empty row, index of every non-empty row)"""
    p = np.asarray(p, np.int64)
    rows = np.flatnonzero(np.diff(p) > 0)
    return p[rows], rows


def row_sums(p, x):
    """float64 sum of |x| over every row (0 for an empty row)"""
    s = np.zeros(len(p) - 1, np.float64)
    starts, rows = _segments(p)
    if len(rows):
        s[rows] = np.add.reduceat(np.abs(np.asarray(x, np.float64)), starts)
    return s


def inflate(x, r):
    x = np.asarray(x, np.float32)
    if r == 2:
        return x * x
    return (x.astype(np.float64) ** np.float64(np.float32(r))).astype(np.float32)


def normalize(p, x):
    x = np.asarray(x, np.float32)
    s = np.repeat(row_sums(p, x), np.diff(p))
    out = x.copy()
    nz = s != 0
    out[nz] = (x[nz].astype(np.float64) / s[nz]).astype(np.float32)
    return out


def first_max(p, q):
    """position of the first maximum of every row (-1 for an empty row)"""
    am = np.full(len(p) - 1, -1, np.int64)
    starts, rows = _segments(p)
    if len(rows):
        q = np.asarray(q)
        top = np.zeros(len(p) - 1, q.dtype)
        top[rows] = np.maximum.reduceat(q, starts)
        at_top = q == np.repeat(top, np.diff(p))
        am[rows] = np.minimum.reduceat(np.where(at_top, np.arange(len(q)), len(q)), starts)
    return am


def prune(p, j, q, pruning):
    """q: inflated and normalised.  Keeps q >= float32(pruning) and the first maximum of every row, then normalises."""
    p = np.asarray(p, np.int64)
    q = np.asarray(q, np.float32)
    keep = q >= np.float32(pruning)
    am = first_max(p, q)
    keep[am[am >= 0]] = True
    cs = np.concatenate([[0], np.cumsum(keep)])
    op = cs[p].astype(np.int32)
    return op, np.asarray(j, np.int32)[keep], normalize(op, q[keep])


def inflate_prune(p, j, x, r, pruning):
    """(inflated and normalised values, pruned CSR triple): steps 3 and 4 of an iteration"""
    q = normalize(p, inflate(x, r))
    return q, prune(p, j, q, pruning)


def convergence(A, B, n_cols):
    """max(0, max over the union of both patterns of abs(m - l) - float32(1e-5) * abs(l)): float32, every operation rounded"""
    def keys(M):
        p = np.asarray(M[0], np.int64)
        return np.repeat(np.arange(len(p) - 1, dtype=np.int64), np.diff(p)) * n_cols + np.asarray(M[1], np.int64)
    ka, kb = keys(A), keys(B)
    u = np.union1d(ka, kb)
    m = np.zeros(len(u), np.float32)
    l = np.zeros(len(u), np.float32)
    m[np.searchsorted(u, ka)] = np.asarray(A[2], np.float32)
    l[np.searchsorted(u, kb)] = np.asarray(B[2], np.float32)
    d = np.abs(m - l) - np.float32(1e-5) * np.abs(l)
    return np.float32(max(np.float32(0), d.max())) if len(u) else np.float32(0)


def exact_sums(p, x):
    """True when the float64 sum of |x| over every row is the same number in every order of the additions: all terms of a row are
    multiples of one 2^-k (k from the lowest set mantissa bit of its terms) and the row total stays below 2^(53 - k), so that every
    partial sum is an integer multiple of 2^-k that a double holds exactly."""
    v = np.abs(np.asarray(x, np.float64))
    f, e = np.frexp(v)
    mant = np.ldexp(f, 53).astype(np.int64)                       # v = mant * 2^(e - 53)
    low = mant & -mant
    grid = np.where(v > 0, e.astype(np.int64) - 53 + np.log2(np.maximum(low, 1)).astype(np.int64), 10000)
    starts, rows = _segments(p)
    if not len(rows):
        return True
    g = np.minimum.reduceat(grid, starts)                         # 2^g: the grid of the row
    g_of = np.zeros(len(p) - 1, np.int64)
    g_of[rows] = np.where(g == 10000, 0, g)
    units = np.ldexp(v, (-np.repeat(g_of, np.diff(p))).astype(np.int64))      # exact: a power of two
    if not np.all(units == np.rint(units)) or not np.all(np.isfinite(units)):
        return False
    return bool(np.all(np.add.reduceat(units, starts) < 2.0 ** 53))


def worst_rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nz = ref != 0
    if not np.all(got[~nz] == 0):
        return np.inf
    return float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0


def margins(p, q, thresholds=THRESHOLDS):
    """(nearest relative distance of a first-normalised value to a threshold, smallest relative gap between the two largest distinct
    values of a row), over the rows that hold at least two different values.  A row of equal entries needs no margin: its L equal
    inflated values v sum to L * v exactly, so every q is the correctly rounded 1 / L on the device and in the model alike."""
    p = np.asarray(p, np.int64)
    near, gap = np.inf, np.inf
    for r in range(len(p) - 1):
        row = np.asarray(q[p[r]:p[r + 1]], np.float64)
        if len(row) < 2:
            continue
        top = np.unique(row)
        if len(top) < 2:
            continue
        for t in thresholds:
            t = float(np.float32(t))
            near = min(near, float(np.min(np.abs(row - t))) / t)
        gap = min(gap, (top[-1] - top[-2]) / top[-1])
    return near, gap


# ---------------------------------------------------------------- unit rows
def unit_row(rng, length, m=None):
    """`length` integer units u >= 1, u < 2^12, that add up to 2^m (m <= 13): the values u * 2^-m are a stochastic row, u * u is exact
    in float32 and every sum of the epilogue is exact"""
    if m is None:
        m = min(13, max(3, int(np.ceil(np.log2(length))) + 3))
    assert length <= 2 ** m and m <= 13
    u = 1 + rng.multinomial(2 ** m - length, np.full(length, 1.0 / length))
    assert u.sum() == 2 ** m and u.min() >= 1 and u.max() < 2 ** 12
    return u.astype(np.int64), m


def _columns(rng, length, n_cols=N_COLS):
    return np.sort(rng.choice(n_cols, size=length, replace=False))


def _assemble(rows, n_cols=N_COLS):
    """rows: list of (columns, float32 values) -> CSR triple"""
    lens = np.array([len(c) for c, _ in rows], np.int64)
    p = np.zeros(len(rows) + 1, np.int32)
    p[1:] = np.cumsum(lens)
    j = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    x = np.concatenate([np.asarray(v, np.float32) for _, v in rows] + [np.zeros(0, np.float32)]).astype(np.float32)
    for c, _ in rows:
        assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < n_cols))
    return p, j, x


EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.float32))


def tie_row(rng, length, positions, top, total_log2):
    u = np.ones(length, np.int64)
    u[list(positions)] = top
    assert u.sum() == 2 ** total_log2
    return _columns(rng, length), (u * 2.0 ** -total_log2).astype(np.float32)


def edge_rows(seed=1):
    """the unit-row part of the edge matrix as a list of (columns, values) and the names of its rows"""
    rng = np.random.default_rng(seed)
    rows, names = [EMPTY], ['empty first']
    for k, n in enumerate(EDGE_LENGTHS):
        u, m = unit_row(rng, n)
        rows.append((_columns(rng, n), (u * 2.0 ** -m).astype(np.float32)))
        names.append('length %d' % n)
        if k % 4 == 3:
            rows.append(EMPTY)
            names.append('empty between')
    for a, b in itertools.combinations(TIE_POSITIONS, 2):        # base 1 unit, two maxima of 29: 198 + 58 = 256
        rows.append(tie_row(rng, 200, (a, b), 29, 8))
        names.append('tie %d,%d' % (a, b))
    for pos in TRIPLE_POSITIONS:                                  # base 1 unit, three maxima of 19: 199 + 57 = 256
        rows.append(tie_row(rng, 202, pos, 19, 8))
        names.append('tie %d,%d,%d' % pos)
    # rows of at most 32 entries (the thread-per-row class of the fused expansion): maxima of 5 units at positions 1 and 3 of 8
    # (after inflation 2: 0.446, restored at 0.5), three maxima in rows of 28 and 32, and 32 equal entries
    for pos, top, n in (((1, 3), 5, 8), ((31 - 4, 0, 16), 13, 28), ((2, 30, 31), 33, 32)):
        u = np.ones(n, np.int64)
        u[list(pos)] = top
        m = int(np.log2(u.sum()))
        assert u.sum() == 2 ** m
        rows.append((_columns(rng, n), (u * 2.0 ** -m).astype(np.float32)))
        names.append('short tie ' + ','.join(str(k) for k in pos))
    for n in (2, 32):                                             # q = 0.5: on the largest threshold; q = 2^-5: a 32-way tie, restored at 0.5
        rows.append((_columns(rng, n), np.full(n, 1.0 / n, np.float32)))
        names.append('%d equal' % n)
    for n in (64, 128):                                           # q = 2^-6 (the threshold itself: all kept) and 2^-7 (one restored)
        rows.append((_columns(rng, n), np.full(n, 1.0 / n, np.float32)))
        names.append('%d equal' % n)
    rows.append(EMPTY)
    names.append('empty last')
    return rows, names


def edge_matrix(seed=1):
    """the unit rows alone: what the fused kernels accept (stochastic operand) -> (CSR triple, row names)"""
    rows, names = edge_rows(seed)
    return _assemble(rows), names


def edge_matrix_prune(seed=1):
    """the edge matrix + the rows of the stand-alone prune: values at, just below and just above float32(2^-6), and five stored zeros"""
    rows, names = edge_rows(seed)
    rng = np.random.default_rng(seed + 100)
    thr = np.float32(2.0 ** -6)
    rows.insert(-1, (_columns(rng, 4), np.array([thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1)), 0.5], np.float32)))
    rows.insert(-1, (_columns(rng, 5), np.zeros(5, np.float32)))
    names[-1:-1] = ['threshold neighbours', 'all zero']
    return _assemble(rows), names


def edge_matrix_counts(seed=1):
    """normalize_l1 alone: the edge matrix, rows of integer counts up to 65535 of the same lengths, a row of mixed signs (the row sum
    is over |x|), an all-zero row"""
    rows, names = edge_rows(seed)
    rng = np.random.default_rng(seed + 200)
    for n in EDGE_LENGTHS:
        v = rng.integers(1, 65536, size=n).astype(np.float32)
        v[0] = 65535.0
        rows.insert(-1, (_columns(rng, n), v))
    v = rng.integers(1, 1000, size=130).astype(np.float32)
    v[::3] *= -1.0
    rows.insert(-1, (_columns(rng, 130), v))
    rows.insert(-1, (_columns(rng, 5), np.zeros(5, np.float32)))
    return _assemble(rows)


def tall_matrix(seed=2, n_rows=TALL_ROWS):
    """more rows than two passes of the capped row grid: 1-3 entries of integer units that add up to 16"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, size=n_rows)
    p = np.zeros(n_rows + 1, np.int32)
    p[1:] = np.cumsum(lens)
    first = rng.integers(0, N_COLS - 3, size=n_rows)
    row_of = np.repeat(np.arange(n_rows), lens)
    within = np.arange(p[-1]) - p[:-1][row_of]
    j = (first[row_of] + within).astype(np.int32)
    # units: (16), (a, 16 - a), (a, b, 16 - a - b)
    a = rng.integers(1, 8, size=n_rows)
    b = rng.integers(1, 8, size=n_rows)
    u = np.zeros(p[-1], np.int64)
    u[p[:-1]] = np.where(lens == 1, 16, a)
    two, three = lens == 2, lens == 3
    u[p[:-1][two] + 1] = 16 - a[two]
    u[p[:-1][three] + 1] = b[three]
    u[p[:-1][three] + 2] = 16 - a[three] - b[three]
    assert u.min() >= 1 and np.all(np.add.reduceat(u, p[:-1]) == 16)
    return p, j, (u / 16.0).astype(np.float32)


def empty_matrix(n_rows=300):
    return np.zeros(n_rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)


def exact_everywhere(M, pruning_values=THRESHOLDS):
    """the proof behind byte equality at inflation 2 on M: exact row sums of the inflated values, of the first-normalised values (the
    second sweep adds up the survivors among them) and of the survivors at every threshold"""
    p, j, x = M
    v = inflate(x, 2.0)
    if not (exact_sums(p, x) and exact_sums(p, v)):
        return False
    q = normalize(p, v)
    if not exact_sums(p, q):
        return False
    for t in pruning_values:
        for src in (x, q):                                        # stand-alone prune of M itself, and of its inflated rows
            keep = src >= np.float32(t)
            am = first_max(p, src)
            keep[am[am >= 0]] = True
            cs = np.concatenate([[0], np.cumsum(keep)])
            if not exact_sums(cs[np.asarray(p, np.int64)], src[keep]):
                return False
    return True


# ---------------------------------------------------------------- convergence pairs
CONV_N = 300


def _conv_pattern(seed=3):
    """300 rows x 300 columns with rows of lengths 0, 64, 65 and 199 among short ones; columns 0 and 299 are left free so that an
    entry can be added before the first and after the last stored column of any row"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 30, size=CONV_N)
    special = {0: 0, 7: 64, 8: 65, 150: 199, 151: 0, CONV_N - 1: 0}
    for r, n in special.items():
        lens[r] = n
    rows = []
    for n in lens:
        c = 1 + np.sort(rng.choice(CONV_N - 2, size=n, replace=False))
        rows.append((c, (rng.integers(1, 256, size=n) / 1024.0).astype(np.float32)))
    return rows


def _with_entry(rows, r, col, val):
    c, v = rows[r]
    k = int(np.searchsorted(c, col))
    assert k == len(c) or c[k] != col
    out = list(rows)
    out[r] = (np.insert(c, k, col), np.insert(v, k, np.float32(val)))
    return out


def convergence_pairs():
    """list of (name, M, last, positive): `positive` says on which side of the test d <= 1e-8 the pair was built"""
    base = _conv_pattern()
    asm = lambda rows: _assemble(rows, CONV_N)
    pairs = [('identical', asm(base), asm(base), False)]
    for name, delta, positive in (('2^-17', 2.0 ** -17, True), ('2^-18', 2.0 ** -18, False)):
        for r, pos in ((150, 0), (150, 63), (150, 64), (150, 198), (7, 63), (8, 64)):
            last = list(base)
            c, v = base[r]
            v = v.copy()
            v[pos] = 0.5
            last[r] = (c, v)
            m = list(last)
            w = v.copy()
            w[pos] = np.float32(0.5 + delta)
            m[r] = (c, w)
            pairs.append(('moved by %s at row of %d, position %d' % (name, len(c), pos), asm(m), asm(last), positive))
    for r, col, where in ((150, 0, 'first column'), (150, CONV_N - 1, 'last column'), (8, 0, 'first column, row of 65'),
                          (151, 17, 'empty row'), (0, 0, 'empty first row'), (CONV_N - 1, CONV_N - 1, 'empty last row')):
        extra = _with_entry(base, r, col, 2.0 ** -10)
        pairs.append(('only in M: ' + where, asm(extra), asm(base), True))
        pairs.append(('only in last: ' + where, asm(base), asm(extra), True))
    rng = np.random.default_rng(4)
    two = []
    for _ in range(2):
        rows = []
        for _ in range(CONV_N):
            n = int(rng.integers(0, 70))
            rows.append((np.sort(rng.choice(CONV_N, size=n, replace=False)), rng.random(n).astype(np.float32)))
        M = asm(rows)
        two.append((M[0], M[1], normalize(M[0], M[2])))
    pairs.append(('unrelated stochastic matrices', two[0], two[1], True))
    return pairs


# ---------------------------------------------------------------- the block-ones link matrix
BLOCKS = (1, 2, 63, 64, 65, 96, 128, 200)


def block_ones():
    """block diagonal, every block all ones: symmetric integer counts.  Every entry of a block of M^2 is the same number, so every
    first-normalised value of a block row is float32(1 / m) at any inflation."""
    rows = []
    o = 0
    for m in BLOCKS:
        for _ in range(m):
            rows.append((np.arange(o, o + m), np.ones(m, np.float32)))
        o += m
    return _assemble(rows, o)


def block_ones_iteration0(pruning, r0=0, r1=None):
    """iteration 0 of mcl() on block_ones(), rows [r0, r1), in closed form: float32(1 / m) >= float32(pruning) keeps the m entries of
    the row at float32(1 / m) (m equal survivors v: v / (m v) is the correctly rounded 1 / m again); otherwise the first maximum is
    restored — the block's first column — at 1.0"""
    rows = []
    o = 0
    for m in BLOCKS:
        q = np.float32(1.0 / m)
        for _ in range(m):
            rows.append((np.arange(o, o + m), np.full(m, q, np.float32)) if q >= np.float32(pruning) else (np.array([o]), np.ones(1, np.float32)))
        o += m
    return _assemble(rows[r0:r1], o)


def block_ones_clusters():
    o, out = 0, []
    for m in BLOCKS:
        out.append(tuple(range(o, o + m)))
        o += m
    return sorted(out)


def clusters_of(att, ptr, mem):
    """the distinct member sets (in a block that keeps all its entries every row is an attractor of the same cluster)"""
    return sorted(set(tuple(sorted(int(v) for v in mem[ptr[k]:ptr[k + 1]])) for k in range(len(att))))
