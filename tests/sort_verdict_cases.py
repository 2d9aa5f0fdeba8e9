"""The corpus for the verdict of `haphic sort` — fast sorting or ALLHiC, compare_fast_sort_and_allhic (HapHiC_sort.py :645-724) — behind
haphic_amd/sort.py bind_verdict and haphic_amd/csrc/hhx_sortverdict.hip: the cases, a host engine with the signature of _lib.sort_verdict_sums,
the reader of tests/golden/sort_verdict.npz, and (`python -m tests.sort_verdict_cases`, where the reference checkout exists) the freeze of that
file from the reference's own function: verdict and log line from compare_fast_sort_and_allhic itself, the sums of all n - 1 rotations from its
nested find_lis, run from the function's code constants (it closes over nothing).  Only results are stored.

A case is two tours over the contigs 0 .. n - 1 — fast (the .tour.sav of fast sorting) and allhic (the .tour of ALLHiC), lists of (contig, '+' | '-')
— and the contig lengths."""
import bisect
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sort_verdict.npz')
CHUNK = 64                           # elements a wave of hhx_sortverdict.hip takes per read: its seams are the multiples of 64
OUTCOMES = ('ratio', 'first', 'later', 'none')

Case = namedtuple('Case', 'name fast allhic lens')


# ------------------------------------------------------------------ host engine
def stand_in(value, lengths, r0=0, r1=None):
    """_lib.sort_verdict_sums on the host: per rotation and class a staircase of (value, dp) in which dp rises with the value, one bisect per element"""
    value, lengths = [int(v) for v in value], [int(x) for x in lengths]
    n = len(value)
    r1 = n - 1 if r1 is None else r1
    assert n >= 2 and 0 <= r0 <= r1 <= n - 1 and sorted(abs(v) for v in value) == list(range(1, n + 1)) and min(lengths) >= 0
    sums = []
    for r in range(r0, r1):
        order = list(range(r, n)) + list(range(r))
        best = 0
        for sign in (1, -1):
            vals, dps = [], []
            for i in order:
                if value[i] * sign < 0:
                    continue
                at = bisect.bisect_left(vals, value[i])
                dp = lengths[i] + (dps[at - 1] if at else 0)
                end = at
                while end < len(vals) and dps[end] <= dp:
                    end += 1
                vals[at:end], dps[at:end] = [value[i]], [dp]
            best = max([best] + dps[-1:])
        sums.append(best)
    return np.array(sums, np.int64)


def values_of(case):
    """compare_list :697-705 of rotation 0: +(pos + 1) where the orientations agree, -(pos + 1) where they do not"""
    where = {c: (j, o) for j, (c, o) in enumerate(case.allhic)}
    return [where[c][0] + 1 if o == where[c][1] else -where[c][0] - 1 for c, o in case.fast]


# ------------------------------------------------------------------ corpus
def _lens(rng, n, ratio=21.0, lo=1000, hi=100_000):
    """one long contig and a tail of short ones: group length / longest contig is about `ratio` (the rule :686 lets groups up to 50 through)"""
    ln = rng.integers(lo, hi, n)
    ln[0] = max(int(ln[1:].sum() / (ratio - 1)), int(ln.max()) + 1)
    return [int(x) for x in ln]


def shuffled(name, n, seed, blocks=8, flips=True, ratio=21.0, scale=1):
    """the ALLHiC tour as the fast-sort tour cut into blocks that are shuffled, some reversed with their orientations flipped: the tours disagree
    in every rotation, which is when all n - 1 of them are evaluated"""
    rng = np.random.default_rng(seed)
    fast = [(int(c), '+-'[int(o)]) for c, o in zip(rng.permutation(n), rng.integers(0, 2, n))]
    cuts = sorted(set(rng.integers(1, n, blocks - 1).tolist())) if n > 2 else []
    pieces = [fast[a:b] for a, b in zip([0] + cuts, cuts + [n])]
    allhic = []
    for k in rng.permutation(len(pieces)):
        piece = pieces[k]
        if flips and rng.integers(0, 2):
            piece = [(c, '-' if o == '+' else '+') for c, o in reversed(piece)]
        allhic += piece
    if n == 2:
        allhic = list(reversed(fast))
    return Case(name, fast, allhic, [x * scale for x in _lens(rng, n, ratio)])


def rotated(name, n, k):
    """allhic[j] = fast[(k + j) mod n], equal lengths: rotation k of the fast-sort tour is the ALLHiC tour"""
    fast = [(c, '+-'[c % 2]) for c in range(n)]
    return Case(name, fast, fast[k:] + fast[:k], [1000] * n)


def cases():
    rng = np.random.default_rng(5)
    n = 8
    ident = shuffled('identical', n, 11)
    rev = [(c, '+') for c in rng.permutation(12).tolist()]
    perm = [int(c) for c in rng.permutation(20)]
    zero = shuffled('zero_length', 9, 19, blocks=4)
    out = [shuffled('n2', 2, 2), shuffled('n3', 3, 3, blocks=3), shuffled('n4', 4, 4, blocks=3)]
    out += [shuffled('n%d' % m, m, m) for m in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 257)]
    out += [
        shuffled('n1025', 1025, 1025, blocks=24),                                        # ranks past 2^10: one more level of the tree
        ident._replace(allhic=list(ident.fast)),                                         # rotation 0 gives 1.0
        rotated('rot_1', n, 1), rotated('rot_last', n, n - 2), rotated('rot_unseen', n, n - 1),
        Case('reversed_flipped', rev, [(c, '-') for c, _ in reversed(rev)], _lens(rng, 12)),      # the negative class carries it
        Case('no_positive', [(c, '+') for c in range(20)], [(c, '-') for c in perm], _lens(rng, 20)),
        Case('no_negative', [(c, '-') for c in range(20)], [(c, '-') for c in perm], _lens(rng, 20)),
        zero._replace(lens=[0 if c == zero.fast[4][0] else x for c, x in enumerate(zero.lens)]),
        shuffled('near_2_40', 5, 40, blocks=3, scale=1 << 24),                           # lengths around 2^40: 8-byte tree cells
        shuffled('near_2_40_n65', CHUNK + 1, 41, scale=1 << 24),
        Case('threshold_at', [(0, '+'), (1, '+')], [(1, '+'), (0, '+')], [900_000, 100_000]),      # 0.9 exactly: >= holds
        Case('threshold_below', [(0, '+'), (1, '+')], [(1, '+'), (0, '+')], [899_999, 100_001]),
        Case('ratio_50', [(c, '+') for c in range(50)], [(c, '+') for c in reversed(range(50))], [100] * 50),          # 50 is not > 50
        Case('ratio_above_50', [(c, '+') for c in range(51)], [(c, '+') for c in reversed(range(51))], [100] * 50 + [1]),
        shuffled('shuffled_n65', CHUNK + 1, 65, blocks=12),                              # disagreeing tours: the True verdict
    ]
    assert len({c.name for c in out}) == len(out)
    return out


def ctg_name(c):
    return 'c%04d' % c


def write_tours(case, prefix):
    """<prefix>.tour.sav and <prefix>.tour as output_tour_file :440-453 and ALLHiC leave them (parse_tours reads the last non-empty line);
    -> fa_dict as `haphic sort` holds it: {contig: length}"""
    for path, tour in ((prefix + '.tour.sav', case.fast), (prefix + '.tour', case.allhic)):
        with open(path, 'w') as f:
            f.write('>INIT\n' + ' '.join(ctg_name(c) + o for c, o in tour) + '\n')
    return {ctg_name(c): int(x) for c, x in enumerate(case.lens)}


def run_verdict(S, case, tmp):
    """the module's compare_fast_sort_and_allhic on a case, in directory tmp, with the relative prefix run() uses -> (verdict, log lines)"""
    import io
    import logging
    cwd = os.getcwd()
    os.chdir(str(tmp))
    stream = io.StringIO()
    handler = logging.StreamHandler(stream)
    handler.setFormatter(logging.Formatter('%(message)s'))
    loggers = [S.logger] + ([S.parse_tours.__globals__['logger']] if 'logger' in getattr(S.parse_tours, '__globals__', {}) else [])
    saved = [(lg, lg.level, lg.propagate) for lg in loggers]
    for lg in loggers:
        lg.addHandler(handler)
        lg.setLevel(logging.INFO)
        lg.propagate = False
    try:
        fa_dict = write_tours(case, case.name)
        verdict = S.compare_fast_sort_and_allhic(case.name, fa_dict)
    finally:
        os.chdir(cwd)
        for lg, level, propagate in saved:
            lg.removeHandler(handler)
            lg.setLevel(level)
            lg.propagate = propagate
    return verdict, stream.getvalue().splitlines()


def fake_module(tmp_logger_name='sort_verdict_fake'):
    """what bind_verdict needs of HapHiC_sort where the checkout is absent: a parse_tours with the reference's interface (the last non-empty line of
    the file, (contig, orientation) pairs under one group key), a logger, and an original function that must not be reached"""
    import logging
    import types
    S = types.ModuleType(tmp_logger_name)
    S.logger = logging.getLogger(tmp_logger_name)

    def parse_tours(tour_files, fa_dict):
        tours = {}
        for path in tour_files:
            with open(path) as f:
                last = [line.strip() for line in f if line.strip()][-1]
            tours[path] = [(item[:-1], item[-1]) for item in last.split()]
        return tours, None

    def compare_fast_sort_and_allhic(prefix, fa_dict):
        raise AssertionError('handed back to the original function')
    S.parse_tours, S.compare_fast_sort_and_allhic = parse_tours, compare_fast_sort_and_allhic
    return S


# ------------------------------------------------------------------ fixture
class Fixture:
    def __init__(self, path=GOLDEN):
        with np.load(path, allow_pickle=False) as z:
            self.z = {k: z[k] for k in z.files}
        self.names = [str(s) for s in self.z['cases']]

    def get(self, case, key):
        return self.z['{}/{}'.format(case, key)]

    def case(self, name):
        tour = lambda k: [(int(c), '+-'[int(o)]) for c, o in zip(self.get(name, k + '_ctg'), self.get(name, k + '_ori'))]      # noqa: E731
        return Case(name, tour('fast'), tour('allhic'), [int(x) for x in self.get(name, 'lens')])

    def verdict(self, name):
        return bool(self.get(name, 'verdict'))

    def log(self, name):
        return str(self.get(name, 'log'))

    def sums(self, name):
        return self.get(name, 'sums')

    def outcome(self, name):
        """which of the four ways out of the function the reference took"""
        log = self.log(name)
        if 'longest contig' in log:
            return 'ratio'
        if 'choose fast sorting' in log:
            return 'none'
        g = int(self.get(name, 'lens').sum())
        return 'first' if int(self.sums(name)[0]) / g >= 0.9 else 'later'

    def self_check(self):
        assert self.names == [c.name for c in cases()]
        for c in cases():
            assert self.case(c.name) == c, c.name
            assert self.sums(c.name).shape == (len(c.lens) - 1,) and self.sums(c.name).dtype == np.int64
        assert {self.outcome(n) for n in self.names} == set(OUTCOMES)
        assert self.outcome('identical') == 'first' and self.outcome('rot_1') == 'later' and self.outcome('rot_last') == 'later'
        assert self.outcome('rot_unseen') == 'none' and self.verdict('rot_unseen') and self.outcome('shuffled_n65') == 'none'
        assert self.outcome('reversed_flipped') == 'first' and self.outcome('ratio_50') != 'ratio' and self.outcome('ratio_above_50') == 'ratio'
        assert not self.verdict('threshold_at') and self.verdict('threshold_below')
        assert min(values_of(self.case('no_positive'))) < 0 and max(values_of(self.case('no_positive'))) < 0
        assert min(values_of(self.case('no_negative'))) > 0
        assert int(self.get('near_2_40', 'lens').max()) > 1 << 39 and 0 in self.get('zero_length', 'lens')
        assert os.path.getsize(GOLDEN) < 256 * 1024


# ------------------------------------------------------------------ freeze (needs the reference checkout)
def reference_sums(S, case):
    """max(find_lis(forward), find_lis(reverse)) :707-710 of every rotation :696, from the reference's own nested function"""
    import types
    code = [c for c in S.compare_fast_sort_and_allhic.__code__.co_consts if isinstance(c, types.CodeType) and c.co_name == 'find_lis']
    find_lis = types.FunctionType(code[0], {'__builtins__': __builtins__})
    value = values_of(case)
    lens = [case.lens[c] for c, _ in case.fast]
    n = len(value)
    sums = []
    for r in range(n - 1):
        compare_list = value[r:] + value[:r]
        order_len_dict = dict(zip(compare_list, lens[r:] + lens[:r]))
        sums.append(max(find_lis(compare_list, order_len_dict, True), find_lis(compare_list, order_len_dict, False)))
    return np.array(sums, np.int64)


def freeze(path=GOLDEN):
    import tempfile
    from tests import sort_cases
    S = sort_cases.load_reference_sort(name='_haphic_sort_reference_verdict_freeze')
    out = {'cases': np.array([c.name for c in cases()])}
    with tempfile.TemporaryDirectory() as tmp:
        for c in cases():
            verdict, lines = run_verdict(S, c, tmp)
            mine = [line for line in lines if line.startswith(c.name + ': choose')]
            assert len(mine) == 1, lines
            for k, tour in (('fast', c.fast), ('allhic', c.allhic)):
                out['{}/{}_ctg'.format(c.name, k)] = np.array([ctg for ctg, _ in tour], np.int32)
                out['{}/{}_ori'.format(c.name, k)] = np.array(['+-'.index(o) for _, o in tour], np.uint8)
            out[c.name + '/lens'] = np.array(c.lens, np.int64)
            out[c.name + '/verdict'] = np.array(bool(verdict))
            out[c.name + '/log'] = np.array(mine[0])
            out[c.name + '/sums'] = reference_sums(S, c)
            print(c.name, len(c.lens), verdict, mine[0], flush=True)
    np.savez_compressed(path, **out)
    Fixture(path).self_check()
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    freeze()
