"""Assembly correction at the places where a wave-per-segment implementation of it goes wrong unnoticed: bin counts around the 64-bin
chunk of k_detect / k_apply_diff (haphic_amd/csrc/hhx_correct.hip), the rule edges of detect_break_points (half-integer medians, a bin
exactly at the coverage cutoff, a run exactly region_cutoff long, tied minima, zero and non-zero valleys together, zeros outside the
outermost counting runs, a median of 0), more segments than one lap of the 2048-block grid, and the closed-interval ends of the pair
rules of break_and_update_ctgs.  Named, deterministic cases built with numpy alone: nothing here imports haphic_amd or the reference.

A case (`cases()`) is a dict: name, res, lens, cov (one int32 array per contig), pos ([lo, hi, lo, hi, ...] per contig, file order),
ratios (median_cov_ratio, region_len_ratio, min_region_cutoff), rounds (breaking rounds whose table is compared; one more detection
follows the last of them).  Coverage is injected, not pushed: it is the coverage its own pairs induce plus a non-negative baseline, so no
round can take a bin below 0 (kth_smallest reads the bins as unsigned) — asserted below for every case.  The one exception is marked per
pair (`uncounted`): a pair that touches a zero-coverage break point cannot have been counted in that bin; such cases break at zero coverage
only, where no coverage is ever taken back.

A pass-one case (`pass_one_cases()`) is a record batch (id1, pos1, id2, pos2) for CorrectTable.push.

The expected results live in tests/golden/correction_edges.npz (tests/golden/make_golden_correction_edges.py, the reference's own
code); `Packer` / `load_fixture` are the file's layout: every integer list in one flat int32 array, the structure in a JSON string."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'correction_edges.npz')
INT32_MAX = 2 ** 31 - 1
H = 20                                                            # the high coverage of most profiles: cutoff 4 at ratio 0.2
LAP_CONTIGS = 2112                                                # the grid of k_detect / k_apply_diff / k_break_pairs is capped at 2048 blocks

# float64 products the cases below hang on
assert 5 * 0.2 == 1.0                                             # a bin of 1 sits exactly on the cutoff
assert 15 * 0.2 == 3.0                                            # exact in float64 (and in float32): a bin of 3 is high
assert 120 * 0.25 == 30.0
assert 180 * 0.35 == 62.99999999999999                            # below the exact product 63
assert 50 * 0.14 == 7.000000000000001                             # above the exact product 7: a run of 7 does not count, a bin of 7 under median 50 is low


def induced(nb, res, pos, skip=()):
    """the coverage the pairs of one contig put on its nb bins (numpy clips the slice at the last bin, :1341)"""
    cov = np.zeros(nb, np.int64)
    for k in range(len(pos) // 2):
        if k not in skip:
            cov[pos[2 * k] // res:pos[2 * k + 1] // res + 1] += 1
    return cov


def prof(*parts):
    """a coverage profile from values, lists of values and (value, count) runs"""
    out = []
    for p in parts:
        if isinstance(p, tuple):
            out += [p[0]] * p[1]
        elif isinstance(p, list):
            out += p
        else:
            out.append(p)
    return np.array(out, np.int64)


def make(name, res, lens, cov, pos=None, ratios=(0.2, 0.0, 1), rounds=0, uncounted=None):
    lens = [int(n) for n in lens]
    cov = [np.asarray(c, np.int64) for c in cov]
    pos = [list(map(int, p)) for p in (pos if pos is not None else [[] for _ in lens])]
    uncounted = uncounted if uncounted is not None else [() for _ in lens]
    assert len(lens) == len(cov) == len(pos) == len(uncounted) and res > 0 and rounds >= 0
    for n, c, p, u in zip(lens, cov, pos, uncounted):
        assert n > 0 and len(c) == n // res + 1, (name, n, len(c))
        assert len(p) % 2 == 0 and all(0 <= p[2 * k] <= p[2 * k + 1] <= INT32_MAX for k in range(len(p) // 2)), name
        assert c.min() >= 0 and c.max() <= INT32_MAX, name
        assert (c - induced(len(c), res, p, u) >= 0).all(), name + ': coverage below what its own pairs induce'
    return dict(name=name, res=int(res), lens=lens, cov=[c.astype(np.int32) for c in cov], pos=pos,
                ratios=(float(ratios[0]), float(ratios[1]), int(ratios[2])), rounds=int(rounds))


def det(name, cov, res=1, ratios=(0.2, 0.0, 1), extra=0, rounds=0):
    """one contig without pairs; at res 1 min_region_cutoff counts bins"""
    cov = np.asarray(cov, np.int64)
    return make(name, res, [(len(cov) - 1) * res + extra], [cov], ratios=ratios, rounds=rounds)


# ------------------------------------------------------------------ bin counts at the chunk seam
SEAM_NB = (63, 64, 65, 127, 128, 129, 193)


def seam_cases():
    out = [det('nb1', [5], res=10, extra=5, ratios=(0.2, 0.0, 10)), det('nb2', [5, 5], res=10, extra=5, ratios=(0.2, 0.0, 10)),
           det('nb3 zero in the middle', [5, 0, 5], res=10, extra=5, ratios=(0.2, 0.0, 10), rounds=1),
           det('nb4 zero at bin 1', [5, 0, 5, 5], res=10, extra=9, ratios=(0.2, 0.0, 10), rounds=1),
           det('nb4 all high', [5, 1, 5, 5], res=10, extra=0, ratios=(0.2, 0.0, 10))]
    for nb in SEAM_NB:
        # a final counting run of exactly 3 bins (the cutoff) that reaches bin nb - 1: closed by the step past the last bin only
        cov = np.full(nb, H)
        cov[nb - 11:nb - 3] = 3
        cov[nb - 7] = 1
        out.append(det('final run reaches the last bin/nb%d' % nb, cov, ratios=(0.2, 0.0, 3), rounds=1))
        for s in (64, 128, 192):
            if nb >= s + 1:                                       # valley [s - 3, s - 1], the run behind it may be bin s alone
                cov = np.full(nb, H)
                v = [2, 3, 0, 1, 0, 2][:min(6, nb - 1 - (s - 3))]
                cov[s - 3:s - 3 + len(v)] = v
                out.append(det('leftmost zero is bin %d/nb%d' % (s - 1, nb), cov, rounds=1))
            if nb >= s + 5:
                cov = np.full(nb, H)
                cov[s - 3:s + 4] = [2, 3, 1, 0, 1, 0, 2]
                out.append(det('leftmost zero is bin %d/nb%d' % (s, nb), cov, rounds=1))
                cov = np.full(nb, H)
                cov[s - 3:s + 3] = [3, 2, 1, 1, 2, 3]
                out.append(det('first minimum is bin %d, bin %d ties/nb%d' % (s - 1, s, nb), cov, rounds=1))
            if nb >= s + 20:                                      # a counting run of exactly 8 bins (the cutoff) over the seam, a zero valley either side
                cov = np.full(nb, H)
                cov[s - 14:s - 4] = 3
                cov[s - 9] = 0
                cov[s + 4:s + 12] = 3
                cov[s + 6] = 0
                out.append(det('counting run spans bins %d-%d/nb%d' % (s - 4, s + 3, nb), cov, ratios=(0.2, 0.0, 8), rounds=1))
    for nb in (64, 128):                                          # an even count whose middle values are (3, 4): every lane stride of kth_smallest
        cov = prof((4, nb // 2 - 2), (3, nb // 2), 4, 4)
        out.append(det('median 3.5 at the cutoff/nb%d' % nb, cov, ratios=(1.0, 0.0, 2)))
    return out


# ------------------------------------------------------------------ median, coverage cutoff, region cutoff
def rule_cases():
    big, top = 2 ** 30, INT32_MAX
    out = [
        det('median 3.5, lower middle would hide the valley', [4, 3, 3, 9], ratios=(1.0, 0.0, 1)),
        det('median 3.5, odd neighbours', [3, 4, 0, 9], rounds=1),
        det('median 0.5 is examined', [5, 0, 0, 1]),
        det('median 0 with large values yields nothing', [9, 0, 0, 0, 9, 0, 7]),
        det('median 0 even count', [top, 0, 0, top, 0, 0]),
        det('all bins equal', [7] * 9),
        det('all bins equal at ratio 1', [7] * 9, ratios=(1.0, 0.0, 1)),
        det('odd count', [H, H, 1, H, H]),
        det('even count', [H, H, 1, H, H, H]),
        det('maximum 1', [1, 0, 1, 1, 1], rounds=1),
        det('maximum 2^30', [big, 5, big, big, 7]),
        det('maximum 2^31-1', [top, 3, top, top - 1, top]),
        det('maximum 2^31-1, half-integer median', [top, 3, top - 1, top]),
        det('maximum 2^31-1 over two chunks', prof((top, 40), 2 ** 28, (top - 1, 30), top), rounds=1),
        # coverage cutoff
        det('bin equal to the cutoff is high', prof((5, 3), 1, (5, 5))),
        det('bin one below the cutoff is low', prof((10, 3), 1, (10, 5))),
        det('15 * 0.2 against a bin of 3', prof((15, 3), 3, (15, 3))),
        det('50 * 0.14 against a bin of 7', prof((50, 3), 7, (50, 3)), ratios=(0.14, 0.0, 1)),
        # region cutoff: min_region_cutoff decides (ratio 0) / len * region_len_ratio decides (min 0)
        det('run equal to min_region_cutoff', prof((H, 3), 1, (H, 3), 0, (H, 2), 2, (H, 4)), res=10, extra=4, ratios=(0.2, 0.0, 30), rounds=1),
        det('run one bin below min_region_cutoff', prof((H, 3), 1, (H, 2), 2, (H, 2), 1, (H, 4)), res=10, extra=4, ratios=(0.2, 0.0, 30)),
        det('run equal to len * ratio', prof((H, 3), 1, (H, 3), 2, (H, 5)), res=10, extra=0, ratios=(0.2, 0.25, 0), rounds=1),
        det('run one bin below len * ratio', prof((H, 3), 1, (H, 2), 2, (H, 6)), res=10, extra=0, ratios=(0.2, 0.25, 0)),
        det('180 * 0.35 is below 63', prof((H, 7), 1, (H, 7), 2, (H, 5)), res=9, extra=0, ratios=(0.2, 0.35, 0)),
        det('50 * 0.14 is above 7', prof((H, 8), 0, (H, 7), 0, (H, 8), 3, (H, 25)), ratios=(0.2, 0.14, 0)),
    ]
    assert out[-4]['lens'] == [120] and out[-3]['lens'] == [120] and out[-2]['lens'] == [180] and out[-1]['lens'] == [50]
    return out


# ------------------------------------------------------------------ valleys (counting runs: 2 bins and more)
def valley_cases():
    r = (0.2, 0.0, 2)
    return [
        det('three runs, deepest valley second', prof((H, 3), [3, 2], (H, 3), [1, 3], (H, 3)), ratios=r),
        det('four runs, deepest valley third', prof((H, 3), 2, (H, 2), [3, 2], (H, 2), [1, 1], (H, 3)), ratios=r, rounds=1),
        det('short high run inside a valley', prof((H, 3), [3, H, 1, 2], (H, 3)), ratios=r),
        det('short high run first in a valley', prof((H, 3), [1, H, 3, H, 1], (H, 3)), ratios=r),
        det('tied minima inside a valley', prof((H, 3), [2, 1, 3, 1, 2], (H, 3)), ratios=r),
        det('tied candidates across valleys', prof((H, 3), [2, 1, 2], (H, 2), [1, 3], (H, 2), [3, 1], (H, 3)), ratios=r),
        det('zero valley with non-zero valleys', prof((H, 3), [1, 0, 1], (H, 2), [1, 1], (H, 2), [2, 0, 0], (H, 3)), ratios=r, rounds=1),
        det('several zeros in one valley', prof((H, 3), [1, 0, 1, 0, 0], (H, 3)), ratios=r),
        det('zeros and minima outside the outermost runs', prof([0, 1, H, 0], (H, 3), 2, (H, 3), [0, H, 0, 1]), ratios=r),
        det('zeros outside, zero inside', prof([0, H, 0], (H, 3), [2, 0], (H, 3), [1, 0, H]), ratios=r),
        det('exactly one counting run', prof([1, 1], (H, 4), [1, H, 0, H, 1]), ratios=r),
        det('ratio 0 makes one run', [5, 0, 5, 5, 0, 5], ratios=(0.0, 0.0, 1)),
        det('valley of one bin between runs of two', prof((H, 2), 0, (H, 2)), ratios=r),
    ]


# ------------------------------------------------------------------ breaking (res 10)
def break_cases():
    out = []
    # break at non-zero coverage, bp = 40: the closed ends of [lo, hi] against [bp, bp + res]
    pos = [50, 70, 51, 70, 5, 40, 5, 39, 45, 45, 12, 12, 0, 94, 60, 120, 41, 49, 52, 52]
    cov = prof((H, 4), 4, (H, 5))                                 # bin 4: (5, 40), (45, 45), (0, 94), (41, 49)
    out.append(make('non-zero break, closed ends', 10, [95], [cov], [pos], ratios=(0.25, 0.0, 20), rounds=1))
    # zero breaks: an end on a point, one below it, straddling pairs (those cannot have been counted at the point)
    pos = [5, 29, 5, 30, 30, 45, 29, 29, 30, 30, 12, 55, 40, 50, 0, 0]
    out.append(make('zero break, one point', 10, [68], [prof((H, 3), 0, (H, 3))], [pos], ratios=(0.2, 0.0, 20), rounds=1, uncounted=[(1, 2, 4, 5)]))
    pos = [20, 49, 19, 20, 50, 50, 20, 50, 5, 70, 49, 49, 0, 19, 30, 49, 60, 79]
    out.append(make('zero break, two points', 10, [79], [prof((H, 2), 0, (H, 2), 0, (H, 2))], [pos], ratios=(0.2, 0.0, 20), rounds=1,
                    uncounted=[(0, 1, 2, 3, 4)]))
    pos = [0, 9, 10, 10, 9, 10, 10, 29, 30, 49, 29, 30, 50, 69, 69, 70, 70, 89, 90, 125, 89, 89, 90, 90, 20, 29, 100, 200, 40, 48, 11, 91]
    out.append(make('zero break, five points', 10, [125], [prof(H, 0, H, 0, H, 0, H, 0, H, 0, (H, 3))], [pos], ratios=(0.2, 0.0, 10), rounds=1,
                    uncounted=[(1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 15)]))
    # 300 pairs (more than one 256-thread trip) whose survivors alternate between the children, every 7th is dropped; a zero break next to it
    pos = []
    for k in range(300):
        if k % 7 == 3:
            pos += [25 + k % 6, 31 + k % 19]                      # meets [30, 40]
        elif k % 2:
            pos += [41 + k % 20, 41 + k % 20 + k % 25]
        else:
            pos += [k % 13, k % 13 + k % 17]
    cov = prof((400, 3), 43, (400, 4))
    assert induced(8, 10, pos)[3] == 43
    pos2 = []
    for k in range(257):
        pos2 += [41 + k % 9, 41 + k % 9 + k % 30] if k % 2 else [k % 10, 10 + k % 20]
    out.append(make('300 pairs alternate between the children', 10, [75, 68], [cov, prof((400, 3), 0, (400, 3))], [pos, pos2], ratios=(0.2, 0.0, 20),
                    rounds=1))
    # a broken contig without pairs between two that have some; an unbroken one with pairs
    cz, cn = prof((H, 3), 0, (H, 3)), prof((H, 3), 2, (H, 3))
    out.append(make('a broken contig without pairs', 10, [65, 66, 67, 68], [cz, cn, prof((H, 7)), cz], [[1, 5, 40, 44], [], [3, 60], [41, 45, 2, 2]],
                    ratios=(0.2, 0.0, 20), rounds=1))
    out.append(make('no broken contig holds a pair', 10, [65, 66, 67], [cz, prof((H, 7)), cn], [[], [3, 60, 10, 20], []], ratios=(0.2, 0.0, 20), rounds=1))
    out.append(make('no pairs at all', 10, [65, 66], [cz, cn], ratios=(0.2, 0.0, 20), rounds=1))
    # lose_inner: len 225, runs of 3 bins count (22.5); round 1 cuts at 90 and 130 (zeros); the last child (len 95, runs of 1 bin count) is cut
    # at two zeros in round 2 — its inner children lose their pairs — and its own last child (len 55) at non-zero coverage in round 3
    cov = prof((H, 9), 0, (H, 3), [0, H, 0, H, 0, H, 1], (H, 3))
    pos = [5, 50, 100, 120, 140, 145, 165, 168, 180, 185, 185, 215, 200, 210, 201, 210, 181, 184, 60, 89, 220, 230]
    out.append(make('second and third round on a child that does not start its contig', 10, [225], [cov], [pos], ratios=(0.2, 0.1, 0), rounds=3))
    return out


# ------------------------------------------------------------------ more segments than one lap of the grid
def lap_case():
    """2112 contigs of 8-12 bins, every one broken in round 1 (by index % 3: at one zero, at non-zero coverage, at two zeros) and its
    last child again in round 2 (at non-zero coverage, as a piece that does not start its contig)"""
    lens, covs, poss = [], [], []
    for i in range(LAP_CONTIGS):
        nb, h = 8 + i % 5, 20 + i % 7
        kind = i % 3
        if kind == 0:
            cov = [h, h, 0, h, h, 1, h, h]
            pos = [i % 7, 12 + i % 5, 30, 30 + i % 9, 33, 47, 41, 62, 60 + i % 4, 75, 70, 70]
        elif kind == 1:
            cov = [h, h, 1, h, h, 2, h, h]
            pos = [i % 7, 12 + i % 5, 15, 33, 30, 30 + i % 9, 41, 62, 52 + i % 5, 58, 60 + i % 4, 75]
        else:
            cov = [h, 0, h, 0, h, 1, h, h]
            pos = [i % 7, 9, 20 + i % 10, 29, 40, 40 + i % 5, 45, 62, 60 + i % 4, 75]
        if i % 11 == 5:
            pos = pos[:2]                                         # some contigs hold a single pair, in their first child
        lens.append((nb - 1) * 10 + 3 + i % 7)
        covs.append(np.array(cov + [h] * (nb - 8), np.int64))
        poss.append(pos)
    return make('grid lap', 10, lens, covs, poss, ratios=(0.2, 0.0, 10), rounds=2)


def cases():
    out = seam_cases() + rule_cases() + valley_cases() + break_cases() + [lap_case()]
    assert len({c['name'] for c in out}) == len(out)
    return out


# ------------------------------------------------------------------ pass one
def pass_one_cases():
    res, lens = 10, [649, 95, 5, 1290]                            # 65, 10, 1 and 130 bins
    out = []

    def add(name, rows):
        a = np.array(rows, np.int32).reshape(-1, 4)
        out.append(dict(name=name, res=res, lens=list(lens), id1=a[:, 0].copy(), pos1=a[:, 1].copy(), id2=a[:, 2].copy(), pos2=a[:, 3].copy()))
    add('one record', [[1, 94, 1, 3]])
    add('64 identical records', [[0, 15, 0, 200]] * 64)
    add('64 records on 64 bins', [[0, 10 * k + 3, 0, 10 * k + 7] for k in range(64)])
    add('64 records on 64 bins of the second chunk', [[3, 10 * k + 9, 3, 10 * k] for k in range(64, 128)])
    for n in (63, 64, 65, 257):
        rng = np.random.default_rng(n)
        rows = []
        for k in range(n):
            c = int(rng.integers(0, len(lens)))
            L = lens[c]
            kind = k % 16
            p, q = int(rng.integers(0, L)), int(rng.integers(0, L))
            row = [c, p, c, q]
            if kind == 0:
                row = [c, p, c, p - p % res + res - 1]            # both ends in one bin
            elif kind == 1:
                row = [c, q, c, L]                                # hi in the last bin (position len)
            elif kind == 2:
                row = [c, L + 3 * res, c, p]                      # hi past the end, pos1 > pos2
            elif kind == 3:
                row = [-1, p, -1, q]
            elif kind == 4:
                row = [-2, p, -2, q]
            elif kind == 5:
                row = [c, p, (c + 1) % len(lens), q % 5]
            elif kind == 6:
                row = [-1, p, c, q]
            elif kind == 7:
                row = [c, max(p, q), c, min(p, q)]                # pos1 >= pos2
            elif kind == 8:
                row = [0, 630 + k % 19, 0, 645 + k % 30]          # round the 63|64 bin seam of contig 0, some past its end
            rows.append(row)
        add('%d mixed records' % n, rows)
    return out


# ------------------------------------------------------------------ hashes and the fixture's layout
def difference(cov):
    """the per-segment difference array whose inclusive scan is the coverage (what CorrectTable.absorb takes)"""
    return np.concatenate([np.diff(np.asarray(c, np.int64), prepend=0) for c in cov]).astype(np.int32)


def case_hash(case):
    h = hashlib.sha256()
    for key in sorted(case):
        v = case[key]
        if isinstance(v, np.ndarray):
            v = v.tolist()
        elif isinstance(v, list) and v and isinstance(v[0], np.ndarray):
            v = [x.tolist() for x in v]
        h.update(json.dumps([key, v]).encode())
    return h.hexdigest()


class Packer:
    """every integer list of the fixture in ONE flat int32 array (a member per list would cost more zip headers than data)"""

    def __init__(self):
        self.parts, self.ptr = [], [0]

    def add(self, values):
        a = np.asarray(values, np.int64).ravel()
        assert not len(a) or (a.min() >= -INT32_MAX - 1 and a.max() <= INT32_MAX)
        self.parts.append(a.astype(np.int32))
        self.ptr.append(self.ptr[-1] + len(a))
        return len(self.parts) - 1

    def arrays(self):
        return (np.concatenate(self.parts) if self.parts else np.zeros(0, np.int32)), np.array(self.ptr, np.int64)


ROUND_KEYS = ('bp_seg', 'bp_n', 'bp_pos', 'bp_cov')              # per detection: broken segments, points of each, positions, coverage of every point
STATE_KEYS = ('lens', 'nb', 'cov', 'np', 'pos')                   # per break: children in table order; cov and pos flat, nb bins / np pairs each


def load_fixture(path=GOLDEN):
    """{'cases': {name: {'hash', 'inputs': {...} or None, 'rounds': [{bp_*: int64 array, 'state': {...} or None}]}},
        'pass_one': {name: {'hash', 'nb', 'cov', 'np', 'pos'}}}"""
    with np.load(path, allow_pickle=False) as z:
        ints, ptr, meta = z['ints'].astype(np.int64), z['ptr'], json.loads(str(z['meta']))

    def get(k):
        return ints[ptr[k]:ptr[k + 1]]

    def thaw(node):
        if isinstance(node, dict):
            return {k: (v if k == 'hash' else get(v) if isinstance(v, int) else thaw(v)) for k, v in node.items()}
        if isinstance(node, list):
            return [thaw(v) for v in node]
        return node
    return thaw(meta)
