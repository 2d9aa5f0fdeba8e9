"""The corpus for the front of `haphic sort` — run() :898-923: HT_links.pkl and get_sub_HT_dict :117-143 per group (haphic_amd/sort.py bind_heads,
hhx_pickle_group_heads of haphic_amd/csrc/hhx_pickleread.hip) — and a host engine with the interface of _lib.LinkPickle whose group_heads restates
the rule of include/haphic_hip.h with numpy, nothing about how.  tests/golden/sort_heads.npz (written by tests/golden/make_golden_sort_heads.py from
the reference's own get_sub_HT_dict) holds what every case must give.

A case is a table — the items of HT_link_dict in file order — and the groups extracted from it one after the other, each a list of contigs in the
order parse_group returns them."""
import os
import pickle
from collections import defaultdict, namedtuple
from itertools import combinations, product

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sort_heads.npz')
PASS_KEYS = 64 * 4                   # keys one wavefront of k_heads_pass takes per step (HD_PER each lane); a wavefront's range is whole steps

Case = namedtuple('Case', 'name items groups kind')        # kind: 'int' | 'float' (hand-back) | 'plain_dict' (a file the reader refuses)


# ------------------------------------------------------------------ host engine
def table_arrays(items):
    """items -> (i, j, value, names): ids in order of first appearance, i before j, key by key (what hhx_pickle_open leaves)"""
    ids = {}
    i, j = np.empty(len(items), np.int32), np.empty(len(items), np.int32)
    for k, ((x, y), _v) in enumerate(items):
        i[k] = ids.setdefault(x, len(ids))
        j[k] = ids.setdefault(y, len(ids))
    values = [v for _k, v in items]
    any_float = any(type(v) is float for v in values)
    return i, j, np.array(values, np.float64 if any_float else np.int64).reshape(len(items)), list(ids)


class HostPickle:
    """_lib.LinkPickle over a file read with pickle.load; open() answers None for what is no defaultdict(int) of 2-tuples of names"""
    opened = 0

    def __init__(self, table):
        self.i, self.j, self.value, self._names = table_arrays(list(table.items()))
        self.n_keys, self.n_names = len(self.i), len(self._names)
        self.any_float = self.value.dtype.kind == 'f'
        self.closed = False
        self.calls = 0

    @classmethod
    def from_arrays(cls, i, j, value, names):
        """the same over arrays as hhx_pickle_open leaves them (tables too large for a Python object per key)"""
        self = cls.__new__(cls)
        self.i, self.j, self.value, self._names = np.asarray(i, np.int32), np.asarray(j, np.int32), np.asarray(value), list(names)
        self.n_keys, self.n_names = len(self.i), len(self._names)
        self.any_float = self.value.dtype.kind == 'f'
        self.closed, self.calls = False, 0
        return self

    @classmethod
    def open(cls, path):
        with open(path, 'rb') as f:
            table = pickle.load(f)
        if type(table) is not defaultdict or table.default_factory is not int:
            return None
        if not all(type(k) is tuple and len(k) == 2 and type(k[0]) is str and type(k[1]) is str and type(v) in (int, float) for k, v in table.items()):
            return None
        cls.opened += 1
        return cls(table)

    def names(self):
        assert not self.closed
        return list(self._names)

    def arrays(self):
        assert not self.closed
        is_float = np.array([True] * self.n_keys) if self.any_float else None
        return self.i, self.j, self.value, is_float, list(self._names)

    def group_heads(self, n, slot, rank):
        assert not self.closed and not self.any_float and n >= 2
        self.calls += 1
        slot, rank = np.asarray(slot, np.int64), np.asarray(rank, np.int64)
        assert slot.size == self.n_names and rank.size == n and sorted(rank.tolist()) == list(range(n))
        sx, sy = slot[self.i], slot[self.j]
        ok = (sx >= 0) & (sy >= 0)
        px, py = np.where(ok, sx >> 1, 0), np.where(ok, sy >> 1, 1)
        ok &= (px != py) & (rank[px] < rank[py]) & (self.value != 0)
        sx, sy, px, py, w = sx[ok], sy[ok], px[ok], py[ok], self.value[ok]
        key = ((np.minimum(px, py) * n + np.maximum(px, py)) << 2) | (2 * (sx & 1) + (sy & 1))
        order = np.argsort(key, kind='stable')
        lo = 0 if rank[0] < rank[1] else 1

        def index(pos, suffix):
            first = np.where(pos == lo, np.where(suffix == 1, 3, 0), np.where(suffix == 1, 2, 1))
            return np.where(pos >= 2, 2 * pos + suffix, first).astype(np.int32)
        return index(px, sx & 1)[order], index(py, sy & 1)[order], w[order].astype(np.int64)

    def close(self):
        self.closed = True


# ------------------------------------------------------------------ corpus
def all_keys(ctgs):
    """every key get_sub_HT_dict looks up for the group, in its order"""
    out = []
    for c1, c2 in combinations(ctgs, 2):
        c1, c2 = sorted([c1, c2])
        out += [(c1 + s1, c2 + s2) for s1, s2 in product(('_H', '_T'), repeat=2)]
    return out


def _noise(rng, n, others):
    """n distinct keys that no group of the case keeps: links among the contigs of another group"""
    keys = all_keys(others)
    assert n <= len(keys)
    return [keys[k] for k in rng.permutation(len(keys))[:n]]


def _names(prefix, n):
    return ['%s%04d' % (prefix, k) for k in range(n)]


def survivors_case(name, n, n_keep, n_noise, seed, at=None):
    """n contigs, exactly n_keep surviving keys among n_noise keys of another group; at: the table positions of the survivors (else shuffled)"""
    rng = np.random.default_rng(seed)
    ctgs = [c for c in rng.permutation(_names('g', n))]
    ctgs = [str(c) for c in ctgs]
    keys = all_keys(ctgs)
    keep = [keys[k] for k in rng.permutation(len(keys))[:n_keep]]
    noise = _noise(rng, n_noise, _names('x', 1 + int(np.ceil(np.sqrt(n_noise / 2 + 1))) + 1))
    total = n_keep + n_noise
    where = np.sort(rng.permutation(total)[:n_keep]) if at is None else np.asarray(at)
    assert where.size == n_keep and (n_keep == 0 or where.max() < total)
    is_keep = np.zeros(total, bool)
    is_keep[where] = True
    keep_it, noise_it = iter(keep), iter(noise)
    items = [(next(keep_it) if is_keep[k] else next(noise_it), int(rng.integers(1, 1000))) for k in range(total)]
    return Case(name, items, [ctgs], 'int')


def small_cases():
    v = iter(range(1, 10 ** 6))
    full = lambda ctgs: [(k, next(v)) for k in all_keys(ctgs)]          # noqa: E731
    rev = lambda items: [((y, x), w + 5000) for (x, y), w in items]      # noqa: E731
    out = []
    t = full(['a', 'b'])
    out.append(Case('n1', t, [['a'], ['b'], []], 'int'))
    out.append(Case('n2_ab', t + rev(t), [['a', 'b']], 'int'))          # both orientations of every pair present
    out.append(Case('n2_ba', t, [['b', 'a']], 'int'))
    out.append(Case('n3', full(['q', 'p', 'r']), [['q', 'p', 'r'], ['r', 'q', 'p'], ['p', 'r']], 'int'))
    # length order against name order: 'b10' < 'b9', 'B' < 'a', a name beyond ASCII (compared by code point: 'é' > 'z', 'É' < 'é')
    odd = ['b9', 'b10', 'a', 'B', 'é', 'z', 'É', 'b1']
    out.append(Case('name_order', full(odd)[::-1], [odd, odd[::-1], ['b10', 'b9'], ['é', 'B', 'z']], 'int'))
    # contigs whose own names end in a suffix: whole names are matched, nothing is stripped
    sfx = ['a', 'a_H', 'a_T', 'a_H_H']
    out.append(Case('suffix_names', full(sfx) + [(('a_H', 'a_T'), 7), (('a_H_H', 'a_H_T'), 8), (('a', 'a_H'), 9)], [sfx, ['a_H', 'a'], ['a_T', 'a_H_H', 'a']], 'int'))
    # a contig with no name in the file, names that end in neither suffix, contigs of other groups, names that are a prefix away
    t = full(['m1', 'm2', 'o1', 'o2'])
    t += [(('m1', 'm2'), 3), (('m1_X', 'm2_H'), 4), (('m1_H', 'm2'), 5), (('m1_h', 'm2_t'), 6), (('m1_H ', 'm2_H'), 7), (('_H', '_T'), 8), (('m1_HH', 'm2_TT'), 9)]
    out.append(Case('strangers', t, [['m1', 'm2', 'absent'], ['absent', 'm2', 'gone', 'm1'], ['o2', 'absent', 'o1'], ['absent', 'gone']], 'int'))
    # only the reversed orientation present: never found; same-contig keys; zero values; values at and beyond 2^53, negative values
    t = [(('s2_H', 's1_T'), 11), (('s1_H', 's1_T'), 12), (('s1_T', 's1_H'), 13), (('s1_H', 's2_H'), 0), (('s1_H', 's2_T'), 2 ** 53), (('s1_T', 's2_T'), 2 ** 53 + 1),
         (('s1_T', 's3_H'), -5), (('s2_T', 's3_T'), -2 ** 62), (('s2_H', 's3_H'), 2 ** 63 - 1), (('s1_H', 's3_T'), 0), (('s3_T', 's1_H'), 1)]
    out.append(Case('values', t, [['s1', 's2', 's3'], ['s3', 's2'], ['s2', 's1']], 'int'))
    return out


def cases():
    out = small_cases()
    for k in (0, 1, 63, 64, 65, 255, 256, 257):
        out.append(survivors_case('keep%d' % k, 24, k, 300 + k, 100 + k))
    out.append(survivors_case('all_keys', 50, 4 * 50 * 49 // 2, 0, 7))                     # every key survives
    # survivors on both sides of every border between the ranges of two wavefronts (at this size a range is one step; borders between two workgroups
    # are among them), and a table that ends inside a quad.  Several steps per wavefront: hhx_tune "heads_grid" on every case, and big_table()
    n_total = 16 * PASS_KEYS + 3
    at = sorted({p for b in range(PASS_KEYS, n_total, PASS_KEYS) for p in (b - 4, b - 1, b, b + 1, b + 3, b + 4) if p < n_total} | {0, 3, 255, 256, n_total - 4, n_total - 3, n_total - 1})
    out.append(survivors_case('borders', 12, len(at), n_total - len(at), 11, at=at))
    # the order key on two and on three radix digits
    out.append(survivors_case('n64', 64, 3000, 500, 64))
    out.append(survivors_case('n65', 65, 3000, 501, 65))
    out.append(survivors_case('n1025', 1025, 20000, 2000, 1025))
    # two groups from one handle, then the first again: nothing of a call is left for the next
    rng = np.random.default_rng(5)
    g1, g2 = _names('u', 9), _names('v', 7)
    both = all_keys(g1) + all_keys(g2) + all_keys([g1[0], g2[0], g1[1], g2[1]])
    both = list(dict.fromkeys(both))
    items = [(both[k], int(rng.integers(1, 50))) for k in rng.permutation(len(both))]
    out.append(Case('two_groups', items, [g1, g2, g1, [g2[0], g1[0], g2[1]]], 'int'))
    # handed back to the reference's function
    t = [(k, 1 + n) for n, k in enumerate(all_keys(['d1', 'd2', 'd3']))]
    out.append(Case('duplicate', t, [['d1', 'd2', 'd1'], ['d3', 'd3'], ['d2', 'd3']], 'int'))
    out.append(Case('floats', [(k, w + 0.5) for k, w in t], [['d1', 'd2', 'd3'], ['d3', 'd1']], 'float'))
    out.append(Case('plain_dict', t, [['d2', 'd1', 'd3']], 'plain_dict'))
    return out


GRID_WAVES = 1536 * 4               # wavefronts of the passes at the default grid (HD_GRID * HD_WAVES)


def big_table(n_keys, seed, n_ctg=4000):
    """arrays of a table large enough that every wavefront of the full grid walks several steps: n_keys distinct keys between the ends of n_ctg
    contigs (names k%05d_H / _T, the smaller name first), about one value in sixteen zero, and two groups of a quarter of the contigs each in a
    shuffled order -> (i, j, value, names, groups, in_group[g][contig])"""
    rng = np.random.default_rng(seed)
    code = np.unique(rng.integers(0, n_ctg * n_ctg * 4, int(n_keys * 2.6)))
    lo, hi = (code >> 2) // n_ctg, (code >> 2) % n_ctg
    code = code[lo < hi]
    code = code[rng.permutation(code.size)[:n_keys]]
    assert code.size == n_keys
    lo, hi, ends = (code >> 2) // n_ctg, (code >> 2) % n_ctg, code & 3
    i, j = (2 * lo + (ends >> 1)).astype(np.int32), (2 * hi + (ends & 1)).astype(np.int32)
    value = rng.integers(0, 16, n_keys).astype(np.int64) * rng.integers(1, 1000, n_keys)
    names = ['k%05d_%s' % (k >> 1, 'HT'[k & 1]) for k in range(2 * n_ctg)]
    order = rng.permutation(n_ctg)
    groups, member = [], []
    for g in range(2):
        ctgs = order[g * (n_ctg // 4):(g + 1) * (n_ctg // 4)]
        groups.append(['k%05d' % c for c in ctgs.tolist()])
        m = np.zeros(n_ctg, bool)
        m[ctgs] = True
        member.append(m)
    return i, j, value, names, groups, member


def table_of(case):
    """the object HT_links.pkl of the case holds"""
    if case.kind == 'plain_dict':
        return dict(case.items)
    table = defaultdict(int)
    table.update(case.items)
    assert len(table) == len(case.items)
    return table


def write_python(case, path):
    with open(path, 'wb') as f:
        pickle.dump(table_of(case), f, protocol=4)


def write_library(case, path):
    """the dialect of hhx_write_link_pickle (integer tables only)"""
    from haphic_amd import _lib
    i, j, value, names = table_arrays(case.items)
    _lib.write_link_pickle(path, i, j, value, names)


# ------------------------------------------------------------------ fixture
class Fixture:
    def __init__(self, path=GOLDEN):
        with np.load(path, allow_pickle=False) as z:
            self.z = {k: z[k] for k in z.files}
        self.names = [str(s) for s in self.z['cases']]

    def n_groups(self, case):
        return int(self.z[case + '/n_groups'])

    def table(self, case):
        """(names, i, j, values)"""
        return [str(s) for s in self.z[case + '/names']], self.z[case + '/ti'], self.z[case + '/tj'], self.z[case + '/tv']

    def group(self, case, g):
        """(ctgs, i, j, w, index names, index values) of the g-th extraction: the reference's items and HT_index_dict in insertion order"""
        p = '{}/{}/'.format(case, g)
        return ([str(s) for s in self.z[p + 'ctgs']], self.z[p + 'i'], self.z[p + 'j'], self.z[p + 'w'], [str(s) for s in self.z[p + 'index_names']],
                self.z[p + 'index_values'])


def expected_pair(fx, case, g):
    """(items of sub_HT_dict, items of HT_index_dict) as lists, from the fixture"""
    _ctgs, i, j, w, names, values = fx.group(case, g)
    return list(zip(zip(i.tolist(), j.tolist()), w.tolist())), list(zip(names, values.tolist()))


def result_pair(sub, index):
    """the same of what a get_sub_HT_dict returned; a frozen container is read through its arrays"""
    if getattr(sub, 'frozen', False):
        items = list(zip(zip(sub.i.tolist(), sub.j.tolist()), sub.w.tolist()))
    else:
        items = list(sub.items())
    return items, list(index.items())


# ------------------------------------------------------------------ a module without the checkout, and a toy job for run()
def fake_module():
    """what sort.bind / bind_heads read of HapHiC_sort, with originals that say so when a call is handed back"""
    import types

    def original(name):
        def fn(*a, **k):
            raise AssertionError('{} was handed to the reference'.format(name))
        return fn
    S = types.SimpleNamespace(**{name: original(name) for name in ('dict_to_matrix', 'get_density_graph', 'get_unfiltered_confidence_graph',
                                                                   'filter_confidence_graph', 'remove_shortest_path', 'update', 'fast_sort',
                                                                   'get_sub_HT_dict')})
    S.pickle = pickle
    S.Pool = object
    return S


def toy_job(tmp):
    """two groups of a few dozen short contigs in directory tmp: asm.fa, HT_links.pkl (Python's pickler), group1.txt, group2.txt -> the argv of
    `haphic sort` for it (quick view: fast sorting alone)"""
    from tests import sort_cases as sc
    rng = np.random.default_rng(9)
    groups = [sc.chain_case('group1', 33, 33, method='sum', lengths=(2000, 20000)), sc.chain_case('group2', 20, 21, lengths=(2000, 20000))]
    table = defaultdict(int)
    with open(os.path.join(tmp, 'asm.fa'), 'w') as fa:
        for g, case in enumerate(groups):
            rename = lambda c, g=g: c if g == 0 else 'd' + c[1:]          # noqa: E731
            with open(os.path.join(tmp, 'group%d.txt' % (g + 1)), 'w') as f:
                f.write('#Contig\tRECounts\tLength\n')
                for ctg, ln in case.ctgs:
                    f.write('{}\t{}\t{}\n'.format(rename(ctg), 1 + ln // 400, ln))
                    fa.write('>{}\n{}\n'.format(rename(ctg), ''.join(rng.choice(list('ACGT'), ln))))
            for (x, y), w in case.links.items():
                x, y = sorted([rename(x), rename(y)])                    # the renamed names keep their order: one letter for all
                table[(x, y)] = w
        table[('c0000_H', 'd0000_H')] = 9                                # between the groups: in neither
        table[('c0001_T', 'c0001_H')] = 4
    with open(os.path.join(tmp, 'HT_links.pkl'), 'wb') as f:
        pickle.dump(table, f, protocol=4)
    return ['asm.fa', 'HT_links.pkl', 'split_clms', 'group1.txt', 'group2.txt', '--quick_view', '--processes', '1']


def run_job(S, tmp, argv, monkeypatch):
    """S.run() on the job in tmp -> {file name: bytes} of the tour files and final_tours links.  The checkout ships no allhic binary and quick view
    never starts it: the existence check of run() :884-890 is answered for that one path."""
    import sys
    real = os.path.exists
    monkeypatch.setattr(os.path, 'exists', lambda p: True if str(p).endswith(os.sep + 'allhic') else real(p))
    monkeypatch.setattr(sys, 'argv', ['haphic sort'] + list(argv))
    monkeypatch.chdir(tmp)
    S.run(S.parse_arguments())
    out = {}
    for name in sorted(os.listdir(tmp)):
        if name.endswith('.tour'):
            with open(os.path.join(tmp, name), 'rb') as f:
                out[name] = f.read()
    out['final_tours'] = sorted((n, os.readlink(os.path.join(tmp, 'final_tours', n))) for n in os.listdir(os.path.join(tmp, 'final_tours')))
    return out
