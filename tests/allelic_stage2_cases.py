"""Inputs shared by the stage-2 tests of --remove_allelic_links (tests/test_allelic_stage2_cpu.py, tests/test_gpu_allelic_stage2.py): the matrix
families the assignment solver is pinned on, with scipy's answers computed once, and random / hand-built (keys, allele groups) inputs of
allelic.nonmax_keys.  Test infrastructure only."""
import functools
import itertools

import numpy as np


@functools.lru_cache(maxsize=None)
def families():
    """{name: count matrices [n, d, d] int64}; the reference solves linear_sum_assignment(-matrix) :568.
    Every d x d matrix over {0, 1, 2} for d = 1, 2, 3; every 4 x 4 matrix over {0, 1}; 22,500 random matrices, d = 4..8, entries below 2, 4 and
    1000 with 40 % of the cells zeroed: ties are the rule."""
    out = {}
    for d in (1, 2, 3):
        out['all %dx%d over 0..2' % (d, d)] = np.array(list(itertools.product(range(3), repeat=d * d)), np.int64).reshape(-1, d, d)
    out['all 4x4 over 0..1'] = ((np.arange(1 << 16)[:, None] >> np.arange(16)) & 1).astype(np.int64).reshape(-1, 4, 4)
    rng = np.random.default_rng(568)
    for d in range(4, 9):
        for top in (2, 4, 1000):
            m = rng.integers(0, top, (1500, d, d))
            m[rng.random(m.shape) < 0.4] = 0
            out['random %dx%d below %d' % (d, d, top)] = m.astype(np.int64)
    for m in out.values():
        m.setflags(write=False)
    return out


def scipy_col4row(matrices):
    from scipy.optimize import linear_sum_assignment
    return np.array([linear_sum_assignment(-m)[1] for m in matrices], np.int64).reshape(len(matrices), matrices.shape[1])


@functools.lru_cache(maxsize=None)
def family_answers():
    """{name: col4row [n, d]} of scipy on -matrix"""
    return {name: scipy_col4row(m) for name, m in families().items()}


def wide_counts(n=600, d=8, seed=40):
    """d = 8 with counts up to 2^40 (sums of 8 stay far below 2^53: scipy's doubles are exact) and many equal cells"""
    rng = np.random.default_rng(seed)
    levels = rng.integers(1, 2 ** 40, 6)
    m = levels[rng.integers(0, 6, (n, d, d))]
    m[rng.random(m.shape) < 0.4] = 0
    m[::3] += rng.integers(0, 3, m[::3].shape)
    return m.astype(np.int64)


def contig_names(n, seed):
    """names whose order is not the id order"""
    rng = np.random.default_rng(seed)
    return ['c%03d' % k for k in rng.permutation(1000)[:n].tolist()]


def random_groups_and_keys(seed, n_ctg, n_groups, n_keys, sizes=(2, 8), share=0.3):
    """(names, groups as sorted name tuples, ki, kj, kcnt): groups of sizes[0]..sizes[1] contigs, `share` of the slots taken from contigs that
    already sit in a group (a contig ends up in one to three groups), distinct keys between contigs that share no group (a key inside a group
    is what the reference's `assert`s :652-659 trip over; the hand-built cases cover it), counts 1..5"""
    rng = np.random.default_rng(seed)
    names = contig_names(n_ctg, seed)
    member_of = [[] for _ in range(n_ctg)]
    groups, fresh = [], rng.permutation(n_ctg).tolist()
    used = []
    for g in range(n_groups):
        size = int(rng.integers(sizes[0], sizes[1] + 1))
        mem = set()
        while len(mem) < size:
            again = [c for c in used if len(member_of[c]) < 3 and c not in mem]
            if (again and rng.random() < share) or not fresh:
                if not again:
                    break
                mem.add(again[int(rng.integers(len(again)))])
            else:
                mem.add(fresh.pop())
        if len(mem) < 2:
            continue
        for c in mem:
            member_of[c].append(g)
            if c not in used:
                used.append(c)
        groups.append(tuple(sorted(names[c] for c in mem)))
    groups = list(dict.fromkeys(groups))
    in_group = [set(g) for g in groups]
    keys, tries = {}, 0
    while len(keys) < n_keys and tries < 20 * n_keys + 100:
        tries += 1
        a, b = rng.integers(0, n_ctg, 2).tolist()
        if a == b or (a, b) in keys or (b, a) in keys or any(names[a] in g and names[b] in g for g in in_group):
            continue
        # three keys in four between grouped contigs: the candidates are the interesting ones
        if rng.random() < 0.75 and not (member_of[a] and member_of[b]):
            continue
        keys[(a, b)] = int(rng.integers(1, 6))
    ki = np.array([k[0] for k in keys], np.int32)
    kj = np.array([k[1] for k in keys], np.int32)
    kcnt = np.array(list(keys.values()), np.int64)
    return names, groups, ki, kj, kcnt


def group_csr(groups, names):
    """(gptr int64, gmem int32) of the groups in the reference's tuple order"""
    cid = {n: k for k, n in enumerate(names)}
    groups = sorted(groups)
    gptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    gmem = np.array([cid[c] for g in groups for c in g], np.int32)
    return gptr, gmem


LETTERS = ['a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i', 'j', 'k', 'l']


def hand_built():
    """{name: (names, groups, keys [(i, j, count)])} — ids index LETTERS"""
    L = LETTERS
    t = lambda *ids: tuple(L[i] for i in ids)                    # noqa: E731
    return {
        'no groups': (L, [], [(0, 1, 3), (2, 3, 1)]),
        'no candidate': (L, [t(0, 1), t(2, 3)], [(0, 5, 3), (6, 7, 1), (4, 2, 2)]),
        'no keys': (L, [t(0, 1), t(2, 3)], []),
        'a pair reached by a single key': (L, [t(0, 1), t(2, 3)], [(0, 2, 4), (5, 6, 1)]),
        'two keys on one row: the cheaper one is not in the matching': (L, [t(0, 1), t(2, 3)], [(0, 2, 4), (0, 3, 9)]),
        'ties: every optimum has the same sum': (L, [t(0, 1), t(2, 3)], [(0, 2, 1), (0, 3, 1), (1, 2, 1), (1, 3, 1)]),
        'both contigs in both groups of a pair': (L, [t(0, 1, 2), t(0, 1, 3)], [(0, 1, 3), (2, 3, 5), (2, 0, 2), (3, 0, 2)]),
        'ga == gb': (L, [t(0, 1, 2, 3)], [(0, 1, 2), (1, 2, 3), (3, 0, 3), (2, 3, 2)]),
        'groups of unequal length': (L, [t(0, 1, 2, 3, 4), t(5, 6), t(7, 8, 9)], [(0, 5, 1), (1, 5, 2), (1, 6, 2), (4, 6, 1), (5, 7, 1), (6, 7, 1), (6, 9, 3), (3, 8, 2), (2, 8, 2)]),
        'eight by eight': (L, [t(0, 1, 2, 3, 4, 5, 6, 7), t(8, 9, 10, 11)], [(i, 8 + j, 1 + (i * j) % 3) for i in range(8) for j in range(4) if (i + j) % 3]),
    }
