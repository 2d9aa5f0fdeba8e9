"""k_absorb_diff, k_apply_diff, k_detect, k_break_pairs and k_cov_push (haphic_amd/csrc/hhx_correct.hip) on the cases of
tests/correction_edge_cases.py against tests/golden/correction_edges.npz, the reference's own results: bin counts round the 64-bin chunk,
the rule edges of the detection, the closed-interval ends of the pair rules, more segments than one lap of the 2048-block grid.  Coverage
and pairs are injected exactly (CorrectTable.absorb).  Every comparison is integer equality; reads the fixture and the case module only."""
import numpy as np
import pytest

from tests import correction_edge_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.cases()
PASS_ONE = cc.pass_one_cases()


@pytest.fixture(scope='module')
def fixture():
    return cc.load_fixture()


@pytest.fixture(autouse=True)
def _knob_restored():
    from haphic_amd import _lib
    yield
    _lib.tune('correct_agg', None)


def table_state(table):
    """the table in the fixture's layout: lengths, bin counts, coverage (segment after segment), pair counts, positions"""
    off, nb, length, po = table.segments()
    flat = table.coverage()
    cov = np.concatenate([flat[o:o + k] for o, k in zip(off.tolist(), nb.tolist())]) if len(off) else flat[:0]
    return {'lens': length, 'nb': nb, 'cov': cov, 'np': np.diff(po), 'pos': table.pairs()}


def assert_state(got, want, where):
    for k in cc.STATE_KEYS:
        assert np.array_equal(np.asarray(got[k], np.int64), want[k]), where + (k,)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_rounds_against_the_reference(case, fixture):
    from haphic_amd import _lib
    want = fixture['cases'][case['name']]
    assert want['hash'] == cc.case_hash(case), 'the fixture was made from other inputs'
    res = case['res']
    table = _lib.CorrectTable(case['lens'], res)
    ctg = np.repeat(np.arange(len(case['lens']), dtype=np.int32), [len(p) // 2 for p in case['pos']])
    lo_hi = np.array([x for p in case['pos'] for x in p], np.int32)
    table.absorb(res, cc.difference(case['cov']), ctg, lo_hi)
    assert table.finalize() == len(ctg)
    # the injected table is the case: k_absorb_diff, the scan of k_apply_diff across its 64-bin carry, the sort by contig
    assert_state(table_state(table), {'lens': case['lens'], 'nb': [len(c) for c in case['cov']], 'cov': np.concatenate(case['cov']),
                                      'np': [len(p) // 2 for p in case['pos']], 'pos': lo_hi}, (case['name'], 'injected'))
    start = np.zeros(len(case['lens']), np.int64)                 # where a segment begins on its original contig
    length = np.array(case['lens'], np.int64)
    for rnd, rd in enumerate(want['rounds']):
        n_bp, bp_cov, bins = table.detect(*case['ratios'])
        seg = np.flatnonzero(n_bp)
        assert np.array_equal(seg, rd['bp_seg']), (case['name'], rnd)
        assert np.array_equal(n_bp[seg], rd['bp_n']), (case['name'], rnd)
        assert np.array_equal(bins.astype(np.int64) * res, rd['bp_pos']), (case['name'], rnd)
        assert np.array_equal(np.repeat(bp_cov[seg], n_bp[seg]), rd['bp_cov']), (case['name'], rnd)
        if rd['state'] is None:
            assert rnd == len(want['rounds']) - 1
            break
        bp_off = np.concatenate(([0], np.cumsum(n_bp[seg]))).astype(np.int64)
        bp_pos = bins.astype(np.int64) * res
        zero = (bp_cov[seg] == 0).astype(np.uint8) | (2 * (start[seg] != 0)).astype(np.uint8)
        table.break_(seg, bp_off, bp_pos, zero)
        assert_state(table_state(table), rd['state'], (case['name'], rnd))
        new_start, new_len = [], []
        for k, s in enumerate(seg.tolist()):
            bounds = [0] + bp_pos[bp_off[k]:bp_off[k + 1]].tolist() + [int(length[s])]
            new_start += [int(start[s]) + b for b in bounds[:-1]]
            new_len += [b - a for a, b in zip(bounds[:-1], bounds[1:])]
        start, length = np.array(new_start, np.int64), np.array(new_len, np.int64)
    table.destroy()


@pytest.mark.parametrize('agg', [0, 1])
@pytest.mark.parametrize('case', PASS_ONE, ids=[c['name'] for c in PASS_ONE])
def test_pass_one_against_the_reference(case, agg, fixture):
    from haphic_amd import _lib
    want = fixture['pass_one'][case['name']]
    assert want['hash'] == cc.case_hash(case), 'the fixture was made from other inputs'
    _lib.tune('correct_agg', agg)
    table = _lib.CorrectTable(case['lens'], case['res'])
    table.push(case['id1'], case['pos1'], case['id2'], case['pos2'])
    assert table.finalize() == int(want['np'].sum())
    got = table_state(table)
    assert np.array_equal(got['lens'], case['lens'])
    for k in ('nb', 'cov', 'np', 'pos'):
        assert np.array_equal(np.asarray(got[k], np.int64), want[k]), (case['name'], agg, k)
    table.destroy()
