"""The cases of the --dense_matrix Markov clustering (csrc/hhx_densemcl.hip) shared by tests/golden/make_golden_dense.py, the CPU test and
the GPU test, and the numpy host model the GPU results are compared against.

The host model restates the dense recurrence of the reference in plain numpy (no sklearn), in float64 or float32:
    run_mcl_clustering :2144-2149   every column divided by its sum of absolute values (a zero column stays), matrix_power in numpy's order
    mcl :2026-2062                  per round: matrix_power (not in round 0), elementwise power, column L1 normalise, prune, and from the third
                                    round on allclose(matrix, last_matrix): |a - b| <= 1e-8 + 1e-5 |b| on every entry
    prune :1999-2014 (dense)        entries < pruning zeroed, the FIRST maximum of every column of the un-pruned matrix put back, normalise
    interpret_result :2065-2095     attractors = rows with a non-zero diagonal entry, a cluster = the non-zero columns of such a row
"""
import numpy as np

PRUNING = 1e-4
ORDERS = (1, 31, 33, 97, 300, 513)      # n < 32, n % 32 = +-1, n % 128 != 0, odd K, more than one 128-tile, pitch padding (513 -> 640)
EXPANSIONS = (2, 3)
INFLATIONS = (1.2, 2.0, 3.0)
MAX_ITER = 200


class Case:
    def __init__(self, name, source, expansion, inflation, max_iter=MAX_ITER, pruning=PRUNING, public=False):
        self.name, self.source, self.expansion, self.inflation, self.max_iter, self.pruning = name, source, expansion, inflation, max_iter, pruning
        self.public = public            # the input goes to the public mcl() as it is (not normalised / pre-expanded first)

    def __repr__(self):
        return self.name


def planted(n, seed):
    """symmetric link matrix of planted clusters: integer link counts 1..39, density 0.3 inside a cluster and 0.01 between clusters, self loops 1.
    Returns the edge list (i < j, count) as int32 arrays."""
    rng = np.random.default_rng(seed)
    k = max(1, min(6, n // 12))
    label = np.sort(rng.integers(0, k, n))
    iu, ju = np.triu_indices(n, 1)
    p = np.where(label[iu] == label[ju], 0.3, 0.01)
    keep = rng.random(len(iu)) < p
    cnt = rng.integers(1, 40, len(iu))
    return iu[keep].astype(np.int32), ju[keep].astype(np.int32), cnt[keep].astype(np.int32)


def matrix_from_edges(n, i, j, cnt):
    m = np.zeros((n, n), np.float32)
    m[i, j] = cnt
    m[j, i] = cnt
    m[np.arange(n), np.arange(n)] = 1.0
    return m


def sources():
    """name -> (n, i, j, count): the link matrices (as the generator freezes them into the golden file)"""
    return {'planted%d' % n: (n,) + planted(n, 1000 + n) for n in ORDERS}


def crafted():
    """name -> float32 matrix handed to the public mcl() / prune() as it is"""
    out = {}
    # (a) dyadic values, pruning 0.3: column 0 has its maximum 0.25 twice (rows 1 and 5: row 1 must win) and that maximum is below the threshold;
    #     column 3 has an exact tie 0.5 / 0.5 (rows 2 and 3) above it
    a = np.zeros((8, 8), np.float32)
    a[:, 0] = [0.125, 0.25, 0.125, 0.125, 0.0, 0.25, 0.0625, 0.0625]
    a[:, 1] = [0.0, 0.75, 0.25, 0, 0, 0, 0, 0]
    a[:, 2] = [0.0, 0.25, 0.5, 0.25, 0, 0, 0, 0]
    a[:, 3] = [0.0, 0.0, 0.5, 0.5, 0, 0, 0, 0]
    a[:, 4] = [0, 0, 0, 0, 0.25, 0.25, 0.25, 0.25]       # stays a four-fold tie at 0.25 < 0.3 after inflate + normalise: all pruned, row 4 comes back
    a[:, 5] = [0, 0, 0, 0, 0.25, 0.5, 0.125, 0.125]
    a[:, 6] = [0, 0, 0, 0, 0.125, 0.125, 0.5, 0.25]
    a[:, 7] = [0, 0, 0, 0, 0.125, 0.125, 0.25, 0.5]
    out['tie8'] = a
    # (b) a column of zeros (and the row of the same node) inside an otherwise stochastic matrix
    b = normalize_l1(matrix_from_edges(12, *planted(12, 7)).astype(np.float32))
    b[:, 5] = 0.0
    b[5, :] = 0.0
    out['zerocol12'] = normalize_l1(b)
    return out


def cases():
    out = [Case('planted%d_e%d_i%s' % (n, e, r), 'planted%d' % n, e, r) for n in ORDERS for e in EXPANSIONS for r in INFLATIONS]
    out.append(Case('planted97_e4_i2.0', 'planted97', 4, 2.0))
    out.append(Case('tie8_prune0.3', 'tie8', 2, 2.0, pruning=0.3, public=True))
    out.append(Case('tie8_prune0.3_iter1', 'tie8', 2, 2.0, max_iter=1, pruning=0.3, public=True))
    out.append(Case('zerocol12', 'zerocol12', 2, 2.0, public=True))
    out += [Case('planted33_e2_i2.0_iter%d' % k, 'planted33', 2, 2.0, max_iter=k) for k in (1, 2, 3)]       # (c) convergence is looked at from round 3
    out.append(Case('planted97_e2_i1.2_iter6', 'planted97', 2, 1.2, max_iter=6))                              # (d) does not converge in max_iter
    return out


# the one run of run_mcl_clustering(..., dense_matrix=True) whose files the golden file holds byte for byte
SEAM = dict(source='planted33', expansion=2, min_inflation=1.4, max_inflation=2.6, inflation_step=0.6, max_iter=200, pruning=PRUNING, nchrs=2)


def seam_inputs(n):
    """-> (fa_dict, frag_index_dict) of n whole contigs (no bins) with distinct lengths"""
    names = ['ctg%03d' % k for k in range(n)]
    fa_dict = {c: [None, 10000 + 137 * ((k * 7) % n) + k, 10 + k % 13] for k, c in enumerate(names)}
    return fa_dict, {c: k for k, c in enumerate(names)}


# ------------------------------------------------------------------ the host model
def normalize_l1(m):
    s = np.abs(m).sum(axis=0, dtype=m.dtype)
    s = np.where(s == 0, np.ones_like(s), s)
    return (m / s[None, :]).astype(m.dtype)


def matrix_power(m, e):
    """numpy.linalg.matrix_power's association order, written out"""
    if e == 1:
        return m.copy()
    if e == 2:
        return m @ m
    if e == 3:
        return (m @ m) @ m
    z = result = None
    while e > 0:
        z = m if z is None else z @ z
        e, bit = divmod(e, 2)
        if bit:
            result = z if result is None else result @ z
    return result


def inflate(m, inflation):
    if inflation == 2.0:
        return m * m
    return np.power(m, m.dtype.type(np.float32(inflation)))


def prune(m, pruning):
    thr = m.dtype.type(np.float32(pruning))
    out = m.copy()
    out[out < thr] = 0
    cols = np.arange(m.shape[1])
    rows = m.argmax(axis=0)
    out[rows, cols] = m[rows, cols]
    return normalize_l1(out)


def step(state, k, expansion, inflation, pruning, want_pre_prune=False):
    """round k of mcl() from the matrix the rounds before left (k = 0: the pre-expanded matrix)"""
    m = matrix_power(state, expansion) if k != 0 else state
    q = normalize_l1(inflate(m, inflation))
    out = prune(q, pruning)
    return (out, q) if want_pre_prune else out


def allclose(a, b):
    one = a.dtype.type
    return bool(np.all(np.abs(a - b) <= one(1e-8) + one(1e-5) * np.abs(b)))


def mcl(pre, expansion, inflation, max_iter, pruning):
    """-> (matrix, rounds, converged, the state entering every round)"""
    m, last, states = pre, None, []
    for k in range(max_iter):
        states.append(m)
        m = step(m, k, expansion, inflation, pruning)
        if k > 1 and allclose(m, last):
            return m, k + 1, True, states
        last = m
    return m, max_iter, False, states


def pre_expand(links, expansion):
    return matrix_power(normalize_l1(links), expansion)


def clusters(m):
    n = m.shape[0]
    out = set()
    for a in np.flatnonzero(np.diagonal(m) != 0).tolist():
        out.add(tuple(np.flatnonzero(m[a] != 0).tolist()))
    seen = set()
    for c in out:
        for node in c:
            if node in seen:
                return None
            seen.add(node)
    return sorted(out) if len(seen) == n else None


def case_input(case, src):
    """src: sources() / crafted() entry -> the float32 matrix mcl() starts from"""
    if case.public:
        return np.asarray(src, np.float32)
    n, i, j, cnt = src
    return pre_expand(matrix_from_edges(n, i, j, cnt), case.expansion)


def log_line(rounds, converged, case):
    head = 'The matrix has converged after {} rounds of iterations ' if converged else 'The matrix does not converge after {} rounds of iterations '
    return (head + '(expansion: {}, inflation: {}, maximum iterations: {}, pruning threshold: {})').format(
        rounds, case.expansion, float(case.inflation), case.max_iter, case.pruning)
