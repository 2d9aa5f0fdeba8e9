"""Host mirror of how hhx_expand_impl (haphic_amd/csrc/hhx_expand.hip) sorts the rows of A * B into its kernel classes, and
engineered operands that reach every class, window count and tile path of the fused expansion.  The mirror is written from the
formulas of the .hip file; the GPU tests compare it with the device's own per-class counters (hhx_profile_counter
"expand_rows_*"), so a threshold that moves under a test makes the test fail instead of silently leaving its class.
No GPU needed here."""
import numpy as np

from oracle import oracle as orc

# constants of hhx_expand.hip
TINY_MAX = 32                   # k_classify: rows with at most this many products -> thread-per-row kernel
STAGE = 1024                    # compact kernel: staged A entries per chunk
MAX_WIN = 512
EX_WAVES_MAX = 1024 // 64
WIN_FIXED_BYTES = 784           # win_fixed_bytes()
HASH_C, HASH_LIMIT, HASH_STAGE, HASH_T, WAVE = 4096, 3072, 256, 512, 64
LDS_MAX = 160 * 1024


def product_counts(A, B):
    """f of every row of A * B: the number of products sum_k |B row k| over the entries (i, k) of A"""
    ap, aj = np.asarray(A[0], np.int64), np.asarray(A[1], np.int64)
    blen = np.diff(np.asarray(B[0], np.int64))
    per_entry = blen[aj]
    cs = np.concatenate([[0], np.cumsum(per_entry)])
    return cs[ap[1:]] - cs[ap[:-1]]


def window_plan(n_cols, nnz_b, cache_slice_mb=0):
    """window_plan(): (cap_win, n_win) of the window class"""
    slice_bytes = cache_slice_mb << 20 if cache_slice_mb > 0 else 1 << 60
    cap_max = ((LDS_MAX - WIN_FIXED_BYTES) // 8) & ~63
    n_win = (n_cols + cap_max - 1) // cap_max
    by_cache = (nnz_b * 8 + slice_bytes - 1) // slice_bytes
    widest = max(1, n_cols // 2048)
    n_win = max(n_win, min(by_cache, widest))
    cap_win = min((((n_cols + n_win - 1) // n_win) + 63) & ~63, cap_max)
    return cap_win, (n_cols + cap_win - 1) // cap_win


def cap_cmp(n_cols):
    """columns of one LDS rank window of the compact kernel"""
    W = (n_cols + 31) // 32
    fixed = STAGE * (8 + 4 + 4) + EX_WAVES_MAX * (8 + 4 + 4) + 8 + MAX_WIN * (8 + 4) + W * 8      # ex_fixed_bytes(W, MAX_WIN)
    budget = 64 * 1024
    if fixed + 2048 * 8 > budget:
        budget = LDS_MAX
    return ((budget - fixed) // 8) & ~63


def hash_lds_bytes(W):
    tail = max(W * 8, (HASH_T // WAVE) * WAVE * 8)
    return (HASH_C + WAVE) * 8 + HASH_C * 4 + HASH_STAGE * (8 + 4 + 4) + EX_WAVES_MAX * (8 + 4 + 4) + 8 + (8 + 4) + 16 + tail


def window_min(n_cols):
    return max(4096, int(float(n_cols) * 0.5))          # HHX_WINDOW_FACTOR unset


def hash_default(n_cols):
    return min(4_000_000, max(65536, int(4.5 * float(n_cols))))


def hash_max(B, n_cols, tuned=None):
    """the hash class's largest product count: tuned = the hhx_tune('hash_max') value (None: the default)"""
    n_b = len(B[0]) - 1
    nnz_b = int(B[0][-1])
    fits = hash_lds_bytes((n_cols + 31) // 32) <= LDS_MAX and n_b > 0 and nnz_b // n_b <= HASH_LIMIT // 2
    if not fits:
        return 0
    return max(0, hash_default(n_cols) if tuned is None else int(tuned))


def classes(A, B, tuned_hash_max=None, cache_slice_mb=0):
    """what k_classify decides for the fused expansion of A * B (float operands, iterations >= 1): a dict with the per-row
    product counts `f`, the thresholds and the row count of every class (window / compact / tiny / hash, before the hash
    kernel hands rows back), and the window plan"""
    n_cols = len(B[0]) - 1
    f = product_counts(A, B)
    wmin, hmax = window_min(n_cols), hash_max(B, n_cols, tuned_hash_max)
    cls = np.where(f <= TINY_MAX, 2, np.where(f <= hmax, 3, np.where(f >= wmin, 0, 1)))
    cap_win, n_win = window_plan(n_cols, int(B[0][-1]), cache_slice_mb)
    cnt = np.bincount(cls, minlength=4)
    return dict(f=f, cls=cls, tiny_max=TINY_MAX, hash_max=hmax, window_min=wmin, cap_win=cap_win, n_win=n_win, cap_cmp=cap_cmp(n_cols),
                window=int(cnt[0]), compact=int(cnt[1]), tiny=int(cnt[2]), hash=int(cnt[3]))


def describe(c):
    return ('window %d, compact %d, tiny %d, hash %d (f <= %d tiny, <= %d hash, >= %d window); n_win %d x %d cols, cap_cmp %d'
            % (c['window'], c['compact'], c['tiny'], c['hash'], c['tiny_max'], c['hash_max'], c['window_min'], c['n_win'], c['cap_win'],
               c['cap_cmp']))


# ---------------------------------------------------------------- engineered operands (CSR triples, rows L1-normalised)
def _csr_from_rows(n, rows_cols, rows_vals):
    lens = np.array([len(c) for c in rows_cols], np.int64)
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    cols = np.concatenate(rows_cols).astype(np.int64)
    vals = np.concatenate(rows_vals).astype(np.float32)
    # sort every row by column (the CSR invariant) and check there are no duplicates
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    order = np.lexsort((cols, row_of))
    cols, vals = cols[order], vals[order]
    key = row_of[order] * n + cols
    assert np.all(np.diff(key) > 0), 'duplicate entry in an engineered row'
    indptr = indptr.astype(np.int32)
    return indptr, cols.astype(np.int32), orc.normalize_l1(indptr, vals)


def _pick(rng, pool, k, exclude=None):
    """k distinct members of pool (a sorted int array), none equal to `exclude`"""
    if exclude is not None:
        pool = pool[pool != exclude]
    return rng.choice(pool, size=k, replace=False)


def multi_window(n=45000, n_heavy=1536, heavy_to_heavy=150, heavy_rand=30, n_medium=512, medium_len=120, n_long=8, long_len=1500,
                 seed=5):
    """Every class in one launch sequence at several column windows (n > 2 x 20352: 3 windows, the last one short, n_cols not a
    multiple of 64).  Heavy rows (window class: f >= window_min, > 128 A entries each, > 1024 of them so the min-hash row order
    runs) point at other heavy rows and at random columns, so the product fills many distinct columns across all windows; groups
    of four heavy rows share their largest entry (an attractor: the grouped kernel of tune "reuse" takes them together).  Medium
    rows point at heavy rows only: f just below window_min, more distinct columns than cap_cmp (compact, several LDS rank
    windows).  Long rows: more than STAGE A entries pointing at light rows (compact, staged in chunks).  The rest are light rows:
    1-7 entries inside 64-wide diagonal blocks (tiny or compact)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    heavy = np.sort(perm[:n_heavy])
    medium = np.sort(perm[n_heavy:n_heavy + n_medium])
    longr = np.sort(perm[n_heavy + n_medium:n_heavy + n_medium + n_long])
    light = np.sort(perm[n_heavy + n_medium + n_long:])
    role = np.zeros(n, np.int8)
    role[heavy], role[medium], role[longr] = 1, 2, 3
    non_heavy = np.sort(np.concatenate([medium, longr, light]))
    cols, vals = [None] * n, [None] * n
    for g, h in enumerate(heavy):
        att = light[g // 4]                                 # the group's attractor: a column only its four rows hold at 8x the weight
        c = np.concatenate([_pick(rng, heavy, heavy_to_heavy, exclude=h), _pick(rng, non_heavy, heavy_rand - 1, exclude=att), [att]])
        v = rng.random(c.size).astype(np.float32) + np.float32(0.5)
        v[c == att] = 8.0
        cols[h], vals[h] = c, v
    for m in medium:
        c = _pick(rng, heavy, medium_len)
        cols[m], vals[m] = c, rng.random(c.size).astype(np.float32) + np.float32(0.5)
    for r in longr:
        c = _pick(rng, light, long_len)
        cols[r], vals[r] = c, rng.random(c.size).astype(np.float32) + np.float32(0.5)
    for r in light:
        b0 = (r // 64) * 64
        k = int(rng.integers(1, 8))
        c = b0 + rng.choice(min(64, n - b0), size=min(k, n - b0), replace=False)
        cols[r], vals[r] = c, rng.random(c.size).astype(np.float32) + np.float32(0.5)
    return _csr_from_rows(n, cols, vals), dict(heavy=heavy, medium=medium, long=longr, light=light, role=role)


def uniform_rows(n=8000, row_len=70, seed=6):
    """every row row_len distinct random columns: f = row_len^2 for every row (the window class at n = 8000 once row_len^2 >=
    4096), thousands of distinct columns per row and nearly all of them survive the pruning — far more survivors than the first
    pool holds"""
    rng = np.random.default_rng(seed)
    cols = [rng.choice(n, size=row_len, replace=False) for _ in range(n)]
    vals = [rng.random(row_len).astype(np.float32) + np.float32(0.5) for _ in range(n)]
    return _csr_from_rows(n, cols, vals)


def boundaries(n=20000, seed=7):
    """rows whose product counts sit exactly on the class thresholds: f = 32 / 33 (tiny | next class), window_min - 1 /
    window_min, hash default / + 1, and rows of one entry.  Built from prescribed row lengths of B: donor rows of length 1 and of
    length 100; a boundary row of target f points at f // 100 long donors and f % 100 short ones.  Returns (operand, dict of
    the boundary row index per target)."""
    rng = np.random.default_rng(seed)
    wmin, hdef = window_min(n), hash_default(n)
    targets = [1, 32, 33, wmin - 1, wmin, hdef, hdef + 1]
    n_long_d = max(t // 100 for t in targets) + 8
    n_short_d = 200
    perm = rng.permutation(n)
    long_d = np.sort(perm[:n_long_d])
    short_d = np.sort(perm[n_long_d:n_long_d + n_short_d])
    bnd = perm[n_long_d + n_short_d:n_long_d + n_short_d + 4 * len(targets)]          # four rows per target
    rest = perm[n_long_d + n_short_d + 4 * len(targets):]
    cols, vals = [None] * n, [None] * n
    for r in long_d:
        cols[r] = rng.choice(n, size=100, replace=False)
    for r in short_d:
        cols[r] = rng.choice(n, size=1, replace=False)
    rows_of = {}
    for i, t in enumerate(targets):
        rows_of[t] = np.sort(bnd[4 * i:4 * i + 4])
        for r in rows_of[t]:
            q, s = divmod(t, 100)
            cols[r] = np.concatenate([rng.choice(long_d, size=q, replace=False), rng.choice(short_d, size=s, replace=False)])
    for r in rest:                                           # light filler in 64-wide diagonal blocks, pointing at filler rows only
        b0 = (r // 64) * 64
        blk = np.arange(b0, min(n, b0 + 64))
        k = int(rng.integers(1, 4))
        cols[r] = rng.choice(blk, size=min(k, blk.size), replace=False)
    # a filler entry may point at a donor or a boundary row: that only changes the filler row's own f (the mirror counts it)
    for r in range(n):
        vals[r] = rng.random(len(cols[r])).astype(np.float32) + np.float32(0.5)
    return _csr_from_rows(n, cols, vals), rows_of


if __name__ == '__main__':                       # the intended class counts of the operands of tests/test_gpu_expand_classes.py
    import time
    for name, make in (('multi_window', lambda: multi_window()[0]), ('uniform_rows', uniform_rows), ('boundaries', lambda: boundaries()[0])):
        t0 = time.time()
        A = make()
        t1 = time.time()
        for hm in (0, None):
            print('%-12s hash_max=%-7s %s' % (name, hm, describe(classes(A, A, hm))))
        print('%-12s nnz %d, built in %.2f s' % (name, int(A[0][-1]), t1 - t0))
    A = uniform_rows()
    print('uniform_rows cache_slice_mb=1: n_win %d' % classes(A, A, 0, cache_slice_mb=1)['n_win'])
    A = multi_window()[0]
    print('multi_window cache_slice_mb=1: n_win %d' % classes(A, A, 0, cache_slice_mb=1)['n_win'])
