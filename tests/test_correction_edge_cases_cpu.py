"""tests/correction_edge_cases.py and tests/golden/correction_edges.npz without a GPU: the fixture belongs to the module (names, input
hashes), the reference reproduces it where its checkout exists, the restatement of tests/test_gpu_correction.py (ref_detect, ref_break) and
a Python port of the device walk (k_detect, kth_smallest, k_apply_diff of haphic_amd/csrc/hhx_correct.hip) equal it on every case, every
case reaches what its name says, and the cases bite: each wrong variant of the rules disagrees with the fixture on a named case."""
import importlib.util
import os

import numpy as np
import pytest

from tests import correction_edge_cases as cc
from tests.test_correction_cpu import REF, _load_reference
from tests.test_gpu_correction import ref_break, ref_detect, ref_pass_one

WAVE = 64
TOP = cc.INT32_MAX


@pytest.fixture(scope='module')
def fixture():
    return cc.load_fixture()


@pytest.fixture(scope='module')
def cases():
    return cc.cases()


def same_rounds(got, want):
    """'' or where two lists of rounds differ"""
    if len(got) != len(want):
        return '%d rounds for %d' % (len(got), len(want))
    for r, (a, b) in enumerate(zip(got, want)):
        for k in cc.ROUND_KEYS:
            if not np.array_equal(np.asarray(a[k], np.int64), b[k]):
                return 'round %d %s' % (r, k)
        if (a['state'] is None) != (b['state'] is None):
            return 'round %d state' % r
        if a['state'] is not None:
            for k in cc.STATE_KEYS:
                if not np.array_equal(np.asarray(a['state'][k], np.int64), b['state'][k]):
                    return 'round %d state %s' % (r, k)
    return ''


# ------------------------------------------------------------------ the models
def run_model(case, detect, brk):
    """the rounds of correct_assembly :1210-1243 with `detect` per contig and `brk` per broken contig, in the fixture's layout"""
    res, ratios = case['res'], case['ratios']
    segs = [(c.copy(), list(p), n, 0) for c, p, n in zip(case['cov'], case['pos'], case['lens'])]      # coverage, positions, length, start on its contig
    out = []
    for rnd in range(case['rounds'] + 1):
        found = [(s, detect(cov, n, res, *ratios)) for s, (cov, _p, n, _st) in enumerate(segs)]
        found = [(s, bp) for s, bp in found if bp]
        out.append({'bp_seg': [s for s, _b in found], 'bp_n': [len(b) for _s, b in found], 'bp_pos': [p for _s, b in found for p, _c in b],
                    'bp_cov': [c for _s, b in found for _p, c in b], 'state': None})
        if not found or rnd == case['rounds']:
            break
        new = []
        for s, bp in found:
            cov, pos, n, start = segs[s]
            bounds = [0] + [p for p, _c in bp] + [n]
            for t, (piece, kid) in enumerate(brk(cov, pos, bp, res, start != 0)):
                new.append((piece, kid, bounds[t + 1] - bounds[t], start + bounds[t]))
        segs = new
        out[-1]['state'] = {'lens': [n for _c, _p, n, _s in segs], 'nb': [len(c) for c, _p, _n, _s in segs],
                            'cov': [int(x) for c, _p, _n, _s in segs for x in c], 'np': [len(p) // 2 for _c, p, _n, _s in segs],
                            'pos': [x for _c, p, _n, _s in segs for x in p]}
    return out


def kth_smallest(c, k, top):
    """kth_smallest of hhx_correct.hip: the bins read as unsigned, the answer built bit by bit from `top` down"""
    u = c.astype(np.int64) & 0xffffffff
    r = 0
    for bit in range(top, -1, -1):
        t = r | (1 << bit)
        if int((u < t).sum()) <= k:
            r = t
    return r


def port_detect(cov, length, res, median_cov_ratio, region_len_ratio, min_region_cutoff, wrong=None):
    """k_detect for one segment, its walk in 64-bin chunks and the step past the last bin kept; `wrong` switches one rule"""
    c = np.asarray(cov, np.int64)
    nb = len(c)
    mx = int(c.max()) if nb else 0
    median = 0.0
    if nb > 0 and mx > 0:
        top = mx.bit_length() - 1
        if nb & 1:
            median = float(kth_smallest(c, nb // 2, top))
        elif wrong == 'median taken as the lower middle value':
            median = float(kth_smallest(c, nb // 2 - 1, top))
        else:
            median = (float(kth_smallest(c, nb // 2 - 1, top)) + float(kth_smallest(c, nb // 2, top))) / 2.0
    if median == 0.0:
        return None
    cov_cutoff = median * median_cov_ratio
    region_cutoff = max(float(min_region_cutoff), float(length) * region_len_ratio)
    less = (lambda a, b: a <= b) if wrong == 'last minimum instead of first' else (lambda a, b: a < b)
    run = n_counting = 0
    vz, vminb, vminv = -1, -1, TOP
    rz, rminb, rminv = -1, -1, TOP
    zeros, bestb, bestv = [], -1, TOP
    closing = nb if wrong == 'the open run not closed after the last bin' else nb + 1
    for base in range(0, closing, WAVE):
        mine = [int(c[base + lane]) if base + lane < nb else 0 for lane in range(WAVE)]
        for j in range(min(WAVE, closing - base)):
            i = base + j
            end = i == nb
            v = mine[j]
            high = not end and (float(v) > cov_cutoff if wrong == '> for >= at the coverage cutoff' else float(v) >= cov_cutoff)
            if high:
                run += 1
                if v == 0 and rz < 0:
                    rz = i
                if less(v, rminv):
                    rminv, rminb = v, i
                continue
            if run > 0:
                size = float(run * res)
                if size > region_cutoff if wrong == '> for >= at the region cutoff' else size >= region_cutoff:
                    if n_counting > 0 or wrong == 'leading zeros reported':
                        if vz >= 0:
                            zeros.append(vz)
                        elif vminb >= 0 and vminv < bestv:
                            bestv, bestb = vminv, vminb
                    n_counting += 1
                    vz, vminb, vminv = -1, -1, TOP
                else:
                    if vz < 0:
                        vz = rz
                    if rminb >= 0 and less(rminv, vminv):
                        vminv, vminb = rminv, rminb
                run, rz, rminb, rminv = 0, -1, -1, TOP
            if not end:
                if v == 0 and vz < 0:
                    vz = i
                if less(v, vminv):
                    vminv, vminb = v, i
    if zeros:
        return [(b * res, 0) for b in zeros]
    if bestb >= 0:
        return [(bestb * res, bestv)]
    return None


def port_scan(diff, carry=True):
    """k_apply_diff for one segment: a 64-lane Hillis-Steele scan per chunk and the carry across chunks, every partial sum inside int32"""
    nb = len(diff)
    cov = np.zeros(nb, np.int64)
    carried = 0
    for base in range(0, nb, WAVE):
        v = np.zeros(WAVE, np.int64)
        v[:min(WAVE, nb - base)] = diff[base:base + WAVE]
        o = 1
        while o < WAVE:
            v[o:] = v[o:] + v[:-o].copy()
            assert np.abs(v).max() <= TOP
            o <<= 1
        k = min(WAVE, nb - base)
        cov[base:base + k] = carried + v[:k]
        if carry:
            carried += int(v[WAVE - 1])
    return cov


def model_break(cov, pos, points, res, lose_inner=False, wrong=None):
    """ref_break with one rule switched"""
    zero = points[0][1] == 0
    bp = points[0][0]
    starts = [0] + [p for p, _c in points]
    kids = [[] for _ in starts]
    for k in range(len(pos) // 2):
        lo, hi = pos[2 * k], pos[2 * k + 1]
        left = lo < bp + res if wrong == 'lo < bp + res for lo <= bp + res' else lo <= bp + res
        right = hi > bp if wrong == 'hi > bp for hi >= bp' else hi >= bp
        if not zero and left and right:
            cov[lo // res:hi // res + 1] -= 1
            continue
        if wrong == 'an end on a break point filed under the left child':
            ci = max(t for t, s in enumerate(starts) if s < lo or t == 0)
            cj = max(t for t, s in enumerate(starts) if s < hi or t == 0)
        else:
            ci = max(t for t, s in enumerate(starts) if s <= lo)
            cj = max(t for t, s in enumerate(starts) if s <= hi)
        lost = lose_inner and ci < len(points) and wrong != 'lose_inner ignored'
        if ci == cj and not lost:
            kids[ci].extend((lo - starts[ci], hi - starts[ci]))
    return [(cov[s // res:starts[t + 1] // res] if t + 1 < len(starts) else cov[s // res:], kids[t]) for t, s in enumerate(starts)]


DETECT_VARIANTS = ('> for >= at the coverage cutoff', '> for >= at the region cutoff', 'last minimum instead of first',
                   'the open run not closed after the last bin', 'leading zeros reported', 'median taken as the lower middle value')
BREAK_VARIANTS = ('lo < bp + res for lo <= bp + res', 'hi > bp for hi >= bp', 'an end on a break point filed under the left child',
                  'lose_inner ignored')


# ------------------------------------------------------------------ the fixture belongs to the module
def test_fixture_matches_the_module(fixture, cases):
    assert list(fixture['cases']) == [c['name'] for c in cases]
    for c in cases:
        fx = fixture['cases'][c['name']]
        assert fx['hash'] == cc.case_hash(c), c['name']
        assert 1 <= len(fx['rounds']) <= c['rounds'] + 1
        if c['name'] == 'grid lap':
            assert fx['inputs'] is None                         # generated by the module, not stored
            continue
        assert np.array_equal(fx['inputs']['lens'], c['lens']) and np.array_equal(fx['inputs']['nb'], [len(v) for v in c['cov']])
        assert np.array_equal(fx['inputs']['cov'], np.concatenate(c['cov']))
        assert np.array_equal(fx['inputs']['np'], [len(p) // 2 for p in c['pos']]) and fx['inputs']['pos'].tolist() == [x for p in c['pos'] for x in p]
    p1 = cc.pass_one_cases()
    assert list(fixture['pass_one']) == [c['name'] for c in p1]
    for c in p1:
        assert fixture['pass_one'][c['name']]['hash'] == cc.case_hash(c), c['name']
    assert os.path.getsize(cc.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(cc.GOLDEN), 'build.npz'))


def test_coverage_never_goes_below_zero(fixture, cases):
    """the condition k_detect's unsigned reading rests on, on the injected tables and on the table after every round"""
    for c in cases:
        assert all(v.min() >= 0 for v in c['cov'])
        for rd in fixture['cases'][c['name']]['rounds']:
            if rd['state'] is not None and len(rd['state']['cov']):
                assert rd['state']['cov'].min() >= 0, c['name']


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_the_reference_reproduces_the_fixture(fixture, cases, monkeypatch):
    H = _load_reference(monkeypatch)
    spec = importlib.util.spec_from_file_location('make_golden_correction_edges', os.path.join(os.path.dirname(cc.GOLDEN),
                                                                                              'make_golden_correction_edges.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for c in cases:
        assert same_rounds(gen.reference_rounds(H, c), fixture['cases'][c['name']]['rounds']) == '', c['name']
    for c in cc.pass_one_cases():
        got, want = gen.reference_pass_one(H, c), fixture['pass_one'][c['name']]
        assert all(np.array_equal(got[k], want[k]) for k in ('nb', 'cov', 'np', 'pos')), c['name']


# ------------------------------------------------------------------ restatement and port against the fixture
def test_restatement_equals_the_fixture(fixture, cases):
    for c in cases:
        assert same_rounds(run_model(c, ref_detect, ref_break), fixture['cases'][c['name']]['rounds']) == '', c['name']


def test_port_of_the_device_walk_equals_the_fixture(fixture, cases):
    for c in cases:
        assert same_rounds(run_model(c, port_detect, model_break), fixture['cases'][c['name']]['rounds']) == '', c['name']


def test_port_of_the_scan_restores_every_coverage(cases):
    for c in cases:
        for cov in c['cov']:
            assert np.array_equal(port_scan(cc.difference([cov]).astype(np.int64)), cov), c['name']


def test_restatement_of_pass_one_equals_the_fixture(fixture):
    for c in cc.pass_one_cases():
        cov, pos = ref_pass_one(c['lens'], c['res'], c['id1'], c['pos1'], c['id2'], c['pos2'])
        want = fixture['pass_one'][c['name']]
        assert np.array_equal(np.concatenate(cov), want['cov']) and [x for p in pos for x in p] == want['pos'].tolist(), c['name']
        assert [len(p) // 2 for p in pos] == want['np'].tolist() and [len(v) for v in cov] == want['nb'].tolist()


# ------------------------------------------------------------------ every case reaches what its name says
def first_round(fixture, name):
    """[(position, coverage), ...] of the first detection of a one-contig case, None when nothing is found"""
    rd = fixture['cases'][name]['rounds'][0]
    return list(zip(rd['bp_pos'].tolist(), rd['bp_cov'].tolist())) or None


def test_seam_cases_reach_what_they_name(fixture, cases):
    names = [c['name'] for c in cases]
    nbs = {c['name']: len(c['cov'][0]) for c in cases}
    for nb in cc.SEAM_NB:
        name = 'final run reaches the last bin/nb%d' % nb
        c = cases[names.index(name)]
        assert nbs[name] == nb and (c['cov'][0][nb - 3:] == cc.H).all() and c['ratios'][2] == 3          # the run ends with the contig
        assert first_round(fixture, name) == [(nb - 7, 1)]
    assert {64, 128} <= set(cc.SEAM_NB)                           # nb % 64 == 0: the extra trip of the walk has lim == 1
    for s, sizes in ((64, (65, 127, 128, 129, 193)), (128, (129, 193)), (192, (193,))):
        for nb in sizes:
            assert first_round(fixture, 'leftmost zero is bin %d/nb%d' % (s - 1, nb)) == [(s - 1, 0)]
    for s, sizes in ((64, (127, 128, 129, 193)), (128, (193,))):
        for nb in sizes:
            assert first_round(fixture, 'leftmost zero is bin %d/nb%d' % (s, nb)) == [(s, 0)]
            name = 'first minimum is bin %d, bin %d ties/nb%d' % (s - 1, s, nb)
            cov = cases[names.index(name)]['cov'][0]
            assert cov[s - 1] == cov[s] == 1 and first_round(fixture, name) == [(s - 1, 1)]
            name = 'counting run spans bins %d-%d/nb%d' % (s - 4, s + 3, nb)
            cov = cases[names.index(name)]['cov'][0]
            assert (cov[s - 4:s + 4] == cc.H).all() and cov[s - 5] < 4 and cov[s + 4] < 4 and first_round(fixture, name) == [(s - 9, 0), (s + 6, 0)]
    for nb in (64, 128):
        name = 'median 3.5 at the cutoff/nb%d' % nb
        assert np.median(cases[names.index(name)]['cov'][0]) == 3.5 and first_round(fixture, name) == [(nb // 2 - 2, 3)]
    assert {nbs[n] for n in names if n != 'grid lap' and len(cases[names.index(n)]['lens']) == 1} >= {1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 193}
    assert first_round(fixture, 'nb1') is None and first_round(fixture, 'nb2') is None and first_round(fixture, 'nb4 all high') is None
    assert first_round(fixture, 'nb3 zero in the middle') == [(10, 0)] and first_round(fixture, 'nb4 zero at bin 1') == [(10, 0)]


RULES = {
    'median 3.5, lower middle would hide the valley': [(1, 3)], 'median 3.5, odd neighbours': [(2, 0)], 'median 0.5 is examined': [(1, 0)],
    'median 0 with large values yields nothing': None, 'median 0 even count': None, 'all bins equal': None, 'all bins equal at ratio 1': None,
    'odd count': [(2, 1)], 'even count': [(2, 1)], 'maximum 1': [(1, 0)], 'maximum 2^30': [(1, 5)], 'maximum 2^31-1': [(1, 3)],
    'maximum 2^31-1, half-integer median': [(1, 3)], 'maximum 2^31-1 over two chunks': [(40, 2 ** 28)],
    'bin equal to the cutoff is high': None, 'bin one below the cutoff is low': [(3, 1)], '15 * 0.2 against a bin of 3': None,
    '50 * 0.14 against a bin of 7': [(3, 7)],
    'run equal to min_region_cutoff': [(70, 0)], 'run one bin below min_region_cutoff': [(30, 1)], 'run equal to len * ratio': [(30, 1)],
    'run one bin below len * ratio': [(30, 1)], '180 * 0.35 is below 63': [(63, 1)], '50 * 0.14 is above 7': [(8, 0)],
    'three runs, deepest valley second': [(8, 1)], 'four runs, deepest valley third': [(10, 1)], 'short high run inside a valley': [(5, 1)],
    'short high run first in a valley': [(3, 1)], 'tied minima inside a valley': [(4, 1)], 'tied candidates across valleys': [(4, 1)],
    'zero valley with non-zero valleys': [(4, 0), (13, 0)], 'several zeros in one valley': [(4, 0)],
    'zeros and minima outside the outermost runs': [(7, 2)], 'zeros outside, zero inside': [(7, 0)], 'exactly one counting run': None,
    'ratio 0 makes one run': None, 'valley of one bin between runs of two': [(2, 0)],
}


def test_rule_cases_reach_what_they_name(fixture, cases):
    """the expectations above were worked out by hand from the rules; the fixture (the reference) agrees with every one"""
    by_name = {c['name']: c for c in cases}
    assert {c['name'] for c in cc.rule_cases() + cc.valley_cases()} == set(RULES)
    for name, want in RULES.items():
        assert first_round(fixture, name) == want, name
    med = {n: float(np.median(by_name[n]['cov'][0])) for n in RULES}
    assert med['median 3.5, odd neighbours'] == 3.5 and med['median 0.5 is examined'] == 0.5 and med['median 0 with large values yields nothing'] == 0
    assert med['median 0 even count'] == 0 and by_name['median 0 even count']['cov'][0].max() == TOP
    assert med['maximum 2^31-1, half-integer median'] == TOP - 0.5 and med['bin equal to the cutoff is high'] == 5 and med['15 * 0.2 against a bin of 3'] == 15
    assert by_name['maximum 1']['cov'][0].max() == 1 and by_name['maximum 2^30']['cov'][0].max() == 2 ** 30
    assert len(by_name['maximum 2^31-1 over two chunks']['cov'][0]) > WAVE
    assert by_name['180 * 0.35 is below 63']['lens'] == [180] and by_name['50 * 0.14 is above 7']['lens'] == [50]


def children(fixture, name, rnd):
    """[(length, coverage, positions), ...] of the table after round `rnd`"""
    st = fixture['cases'][name]['rounds'][rnd]['state']
    cp, pp = np.cumsum(np.r_[0, st['nb']]), 2 * np.cumsum(np.r_[0, st['np']])
    return [(int(n), st['cov'][a:b].tolist(), st['pos'][c:d].tolist()) for n, a, b, c, d in zip(st['lens'], cp[:-1], cp[1:], pp[:-1], pp[1:])]


def test_break_cases_reach_what_they_name(fixture, cases):
    by_name = {c['name']: c for c in cases}
    # non-zero break at 40: lo == 50 and hi == 40 are dropped, lo == 51 and hi == 39 survive
    assert first_round(fixture, 'non-zero break, closed ends') == [(40, 4)]
    left, right = children(fixture, 'non-zero break, closed ends', 0)
    assert left == (40, [cc.H - 2, cc.H - 2, cc.H - 2, cc.H - 2], [5, 39, 12, 12])
    assert right[0] == 55 and right[1][0] == 0 and right[2] == [11, 30, 20, 80, 12, 12]
    # zero breaks: an end on the point belongs to the child on the right, one below it to the one on the left
    a, b = children(fixture, 'zero break, one point', 0)
    assert a[2] == [5, 29, 29, 29, 0, 0] and b[2] == [0, 15, 0, 0, 10, 20]
    a, b, c = children(fixture, 'zero break, two points', 0)
    assert a[2] == [0, 19] and b[2] == [0, 29, 29, 29, 10, 29] and c[2] == [0, 0, 10, 29]
    kids = children(fixture, 'zero break, five points', 0)
    assert [k[0] for k in kids] == [10, 20, 20, 20, 20, 35] and [len(k[1]) for k in kids] == [1, 2, 2, 2, 2, 4]
    assert [k[2] for k in kids] == [[0, 9], [0, 0, 0, 19, 10, 19], [0, 19, 10, 18], [0, 19], [0, 19, 19, 19], [0, 35, 0, 0, 10, 110]]
    # 300 pairs: more than one trip of 256 threads, dropped pairs in between, file order inside each child
    c = by_name['300 pairs alternate between the children']
    assert len(c['pos'][0]) // 2 == 300 > 256 and len(c['pos'][1]) // 2 == 257
    a, b, d, e = children(fixture, '300 pairs alternate between the children', 0)
    pos = c['pos'][0]
    keep = [(pos[2 * k], pos[2 * k + 1]) for k in range(300) if k % 7 != 3]
    assert a[2] == [x for lo, hi in keep if hi < 30 for x in (lo, hi)] and b[2] == [x - 30 for lo, hi in keep if lo > 40 for x in (lo, hi)]
    assert len(a[2]) + len(b[2]) == 2 * len(keep) and min(len(a[2]), len(b[2])) > 200
    sides = [hi < 30 for lo, hi in keep]
    assert sum(x != y for x, y in zip(sides[:-1], sides[1:])) > 150                                       # the survivors do alternate
    assert len(d[2]) + len(e[2]) == 2 * 257
    # contigs without pairs
    st = fixture['cases']['a broken contig without pairs']['rounds'][0]
    assert st['bp_seg'].tolist() == [0, 1, 3] and st['state']['np'].tolist() == [1, 1, 0, 0, 1, 1]
    st = fixture['cases']['no broken contig holds a pair']['rounds'][0]
    assert st['bp_seg'].tolist() == [0, 2] and st['state']['np'].tolist() == [0, 0, 0, 0]
    assert sum(len(p) for p in by_name['no broken contig holds a pair']['pos']) > 0                      # the table holds pairs, the broken contigs none
    # lose_inner
    name = 'second and third round on a child that does not start its contig'
    r = fixture['cases'][name]['rounds']
    assert len(r) == 4 and [x['bp_seg'].tolist() for x in r] == [[0], [2], [2], []]
    assert list(zip(r[0]['bp_pos'], r[0]['bp_cov'])) == [(90, 0), (130, 0)] and list(zip(r[1]['bp_pos'], r[1]['bp_cov'])) == [(20, 0), (40, 0)]
    assert list(zip(r[2]['bp_pos'], r[2]['bp_cov'])) == [(20, 1)]
    assert [k[2] for k in children(fixture, name, 0)] == [[5, 50, 60, 89], [10, 30], [10, 15, 35, 38, 50, 55, 55, 85, 70, 80, 71, 80, 51, 54, 90, 100]]
    c1, c2, c3 = children(fixture, name, 1)
    assert c1[2] == [] and c2[2] == []                            # (10, 15) lies inside the first, (35, 38) inside the second: lost although both ends do
    assert c3[0] == 55 and c3[2] == [10, 15, 15, 45, 30, 40, 31, 40, 11, 14, 50, 60]                      # the last child keeps its pairs
    d1, d2 = children(fixture, name, 2)
    assert d1[2] == [] and d2[2] == [11, 20, 30, 40]             # (10, 15) and (11, 14) lost with the inner child; (15, 45) and (30, 40) meet [20, 30]
    assert d2[1][0] == 0                                          # the pair that made the break point's coverage is taken back


def test_lap_case_reaches_what_it_names(fixture, cases):
    c = cases[-1]
    assert c['name'] == 'grid lap' and len(c['lens']) == cc.LAP_CONTIGS > 2048 and c['res'] == 10
    nb = np.array([len(v) for v in c['cov']])
    assert nb.min() == 8 and nb.max() == 12 and 20_000 < nb.sum() < 30_000
    r = fixture['cases']['grid lap']['rounds']
    assert len(r) == 3
    assert r[0]['bp_seg'].tolist() == list(range(cc.LAP_CONTIGS))                                        # every contig is broken in round 1
    n0, cov0 = r[0]['bp_n'], r[0]['bp_cov'][np.cumsum(np.r_[0, r[0]['bp_n'][:-1]])]
    kind = np.arange(cc.LAP_CONTIGS) % 3
    assert (n0[kind == 2] == 2).all() and (n0[kind != 2] == 1).all() and (cov0[kind == 1] > 0).all() and (cov0[kind != 1] == 0).all()
    lap2 = np.arange(2048, cc.LAP_CONTIGS)
    assert (kind[lap2] != kind[lap2 - 2048]).all() and (nb[lap2] != nb[lap2 - 2048]).all()               # not the segments the first lap saw
    assert len(r[0]['state']['lens']) > 4224 and len(r[1]['bp_seg']) > 2048                               # round 2: detection and breaking lap
    assert (r[1]['bp_cov'] > 0).all() and len(r[1]['state']['lens']) == 2 * len(r[1]['bp_seg'])
    assert (r[1]['state']['np'][0::2] == 0).all() and r[1]['state']['np'][1::2].sum() > 1000             # inner children lose, last children keep
    assert len(r[2]['bp_seg']) == 0


def test_pass_one_cases_reach_what_they_name(fixture):
    p1 = {c['name']: c for c in cc.pass_one_cases()}
    assert [len(p1[n]['id1']) for n in ('one record', '63 mixed records', '64 mixed records', '65 mixed records', '257 mixed records')] == [1, 63, 64, 65, 257]
    c = p1['64 identical records']
    assert len(c['id1']) == WAVE and len({(a, p, b, q) for a, p, b, q in zip(c['id1'], c['pos1'], c['id2'], c['pos2'])}) == 1
    assert fixture['pass_one'][c['name']]['cov'][1:21].tolist() == [WAVE] * 20                           # one wave, one word per add
    for name, first in (('64 records on 64 bins', 0), ('64 records on 64 bins of the second chunk', 64)):
        c = p1[name]
        assert (c['pos1'] // c['res'] == c['pos2'] // c['res']).all() and sorted(c['pos1'] // c['res']) == list(range(first, first + WAVE))
    assert (p1['64 records on 64 bins of the second chunk']['pos1'] > p1['64 records on 64 bins of the second chunk']['pos2']).all()
    for n in (63, 64, 65, 257):
        c = p1['%d mixed records' % n]
        lens = np.array(c['lens'])
        same = (c['id1'] == c['id2']) & (c['id1'] >= 0)
        hi, L = np.maximum(c['pos1'], c['pos2'])[same], lens[c['id1'][same]]
        assert (c['id1'] == -1).any() and (c['id1'] == -2).any() and (c['id1'] != c['id2']).any()
        assert (c['pos1'][same] > c['pos2'][same]).any() and (c['pos1'][same] < c['pos2'][same]).any()
        assert (hi // c['res'] == L // c['res']).any() and (hi // c['res'] > L // c['res']).any()        # in the last bin, past the last bin
        assert (c['pos1'][same] // c['res'] == c['pos2'][same] // c['res']).any()
        assert fixture['pass_one'][c['name']]['np'].sum() == same.sum()


# ------------------------------------------------------------------ the cases bite
def disagreements(fixture, cases, detect, brk):
    """the cases (the grid lap aside) on which the model differs from the fixture"""
    return [c['name'] for c in cases if c['name'] != 'grid lap' and same_rounds(run_model(c, detect, brk), fixture['cases'][c['name']]['rounds'])]


CAUGHT_BY = {
    '> for >= at the coverage cutoff': 'bin equal to the cutoff is high',
    '> for >= at the region cutoff': 'final run reaches the last bin/nb63',
    'last minimum instead of first': 'first minimum is bin 63, bin 64 ties/nb127',
    'the open run not closed after the last bin': 'final run reaches the last bin/nb63',
    'leading zeros reported': 'zeros and minima outside the outermost runs',
    'median taken as the lower middle value': 'median 3.5 at the cutoff/nb64',
    'lo < bp + res for lo <= bp + res': 'non-zero break, closed ends',
    'hi > bp for hi >= bp': 'non-zero break, closed ends',
    'an end on a break point filed under the left child': 'zero break, one point',
    'lose_inner ignored': 'second and third round on a child that does not start its contig',
}


@pytest.mark.parametrize('wrong', DETECT_VARIANTS + BREAK_VARIANTS)
def test_every_wrong_variant_is_caught(fixture, cases, wrong):
    if wrong in DETECT_VARIANTS:
        got = disagreements(fixture, cases, lambda *a: port_detect(*a, wrong=wrong), model_break)
    else:
        got = disagreements(fixture, cases, port_detect, lambda *a: model_break(*a, wrong=wrong))
    assert CAUGHT_BY[wrong] in got, (wrong, got)


def test_a_dropped_carry_is_caught(cases):
    """the scan of k_apply_diff without its carry between 64-bin chunks: wrong on the first case with more than 64 bins, right below"""
    bad = [c['name'] for c in cases if any(not np.array_equal(port_scan(cc.difference([v]).astype(np.int64), carry=False), v) for v in c['cov'])]
    assert bad and bad[0] == 'final run reaches the last bin/nb65'
    assert all(max(len(v) for v in c['cov']) > WAVE for c in cases if c['name'] in bad)
