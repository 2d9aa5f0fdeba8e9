"""Host side of the assembly correction (haphic_amd/correct.py, patch.CORRECTION_SEAMS): no GPU needed."""
import copy
import os
import random
import sys
import types

import pytest

REF = '/root/reference/scripts'


def _fake_reference():
    from haphic_amd import patch
    H = types.ModuleType('HapHiC_cluster_stand_in')
    for table in (patch.SEAMS, patch.CONTAINER_SEAMS, patch.OPTIONAL, patch.CORRECTION_SEAMS):
        for name in table:
            setattr(H, name, (lambda n: lambda *a, **k: ('original', n))(name))
    H.run = lambda *a, **k: 'ran'
    return H


def test_patch_binds_and_restores_every_correction_seam():
    from haphic_amd import correct, patch
    H = _fake_reference()
    originals = {name: getattr(H, name) for name in patch.CORRECTION_SEAMS}
    assert len(originals) == 8
    saved = patch.patch_reference(H, ingest=True)
    try:
        for name, (cite, fn) in patch.CORRECTION_SEAMS.items():
            assert cite.startswith('HapHiC_cluster.py:') and fn is getattr(correct, name)
            bound = getattr(H, name)
            assert bound is not originals[name]
            assert getattr(bound, '__wrapped__', bound) is fn, name
        # plain dicts (what the reference's own pass one returns) go back to the reference's functions
        assert H.detect_break_points({}, {}, None) == ('original', 'detect_break_points')
        assert H.break_and_update_ctgs({}, {}, {}, {}, {}, {}, {}, {}, set(), None) == ('original', 'break_and_update_ctgs')
    finally:
        patch.unpatch_reference(H, saved)
    for name in patch.CORRECTION_SEAMS:
        assert getattr(H, name) is originals[name], name


def test_keep_reference_ingest_leaves_correction_alone():
    from haphic_amd import patch
    H = _fake_reference()
    originals = {name: getattr(H, name) for name in patch.CORRECTION_SEAMS}
    saved = patch.patch_reference(H, ingest=False)
    try:
        for name in patch.CORRECTION_SEAMS:
            assert getattr(H, name) is originals[name]
    finally:
        patch.unpatch_reference(H, saved)


def _load_reference(monkeypatch):
    """the reference module with the interval stand-in of tests/golden/make_golden_correction.py for `portion`; the stand-in modules and
    the import leave sys.modules with the test"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_correction', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                                                                        'make_golden_correction.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}),
                        ('portion', {'closed': lambda a, b: gen.Iv([(a, b)]), 'empty': lambda: gen.Iv()})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        monkeypatch.setitem(sys.modules, name, m)
    monkeypatch.delitem(sys.modules, 'HapHiC_cluster', raising=False)
    monkeypatch.syspath_prepend(REF)
    import HapHiC_cluster as H
    monkeypatch.setitem(sys.modules, 'HapHiC_cluster', H)      # restored (dropped) when the test ends
    return H


def _bind_stand_in(monkeypatch):
    import haphic_amd
    from haphic_amd import cluster, correct, patch
    from tests import correction_fixture
    lib = correction_fixture.stand_in_lib()
    monkeypatch.setattr(haphic_amd, '_lib', lib)
    for mod in (cluster, correct):
        monkeypatch.setattr(mod, '_lib', lib)
    monkeypatch.setattr(patch, '_lib', lib, raising=False)
    return lib


def test_mirrors_against_the_reference_fixture(tmp_path, monkeypatch):
    """tests/golden/correction.npz through the mirrors with the numpy stand-in for the library: pass one, every round (break points, the table
    after the break), the host bookkeeping (final_break_* dicts, corrected contig table, corrected_ctgs.txt) and pass two of both variants"""
    from tests import correction_fixture
    _bind_stand_in(monkeypatch)
    correction_fixture.check_against_mirrors(correction_fixture.load(), str(tmp_path))


def _tree(d):
    out = {}
    for root, _dirs, files in os.walk(d):
        for f in files:
            if not f.endswith(('.log', '.pdf', '.png')):         # logs carry times, matplotlib stamps a creation date
                p = os.path.join(root, f)
                out[os.path.relpath(p, d)] = os.readlink(p) if os.path.islink(p) else open(p, 'rb').read()
    return out


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
@pytest.mark.parametrize('extra', [[], ['--bin_size', '20'], ['--quick_view']])
def test_whole_run_with_correction_patched_and_unpatched(tmp_path, monkeypatch, extra):
    """HapHiC_cluster.run() with --correct_nrounds 2, untouched and with every seam re-bound: identical file trees"""
    import pickle
    from haphic_amd import correct, patch
    from tests import correction_fixture
    H = _load_reference(monkeypatch)
    correction_fixture.write_inputs(correction_fixture.load(), str(tmp_path))
    monkeypatch.setattr(H, 'dot_product_mkl', lambda a, b, **k: (a @ b).tocsc(), raising=False)
    monkeypatch.setattr(H, 'INTEL_MKL', True, raising=False)

    def run(sub):
        d = tmp_path / sub
        d.mkdir()
        monkeypatch.chdir(d)
        monkeypatch.setattr(sys, 'argv', ['haphic', '../asm.fa', '../hic.pairs', '3', '--min_inflation', '1.2', '--max_inflation', '2.0',
                                          '--inflation_step', '0.4', '--Nx', '100', '--flank', '20', '--correct_nrounds', '2'] + extra)
        H.run(H.parse_arguments())
        return _tree(str(d))
    want = run('ref')
    _bind_stand_in(monkeypatch)
    thawed = []
    real_thaw = correct.CorrectionSession.thaw
    monkeypatch.setattr(correct.CorrectionSession, 'thaw', lambda self: (thawed.append(1), real_thaw(self))[1])
    saved = patch.patch_reference(H)
    try:
        got = run('ours')
    finally:
        patch.unpatch_reference(H, saved)
    assert not thawed, 'correct_assembly made the correction tables thaw'
    assert sorted(want) == sorted(got)
    assert {'corrected_asm.fa', 'corrected_ctgs.txt', 'alignments.bed', 'HT_links.pkl'} <= set(want) and want['corrected_ctgs.txt']
    if '--quick_view' not in extra:
        assert {'paired_links.clm', 'full_links.pkl'} <= set(want) and any(k.startswith('inflation_') for k in want)
    for k in want:
        if k.endswith('.pkl'):
            a, b = pickle.loads(want[k]), pickle.loads(got[k])
            assert type(a) is type(b) and list(a.items()) == list(b.items()), 'pickle differs: ' + k
        else:
            assert want[k] == got[k], 'file differs: ' + k


def _count_gatc(seq, RE):
    return seq.count(RE) + 1


def test_bookkeeping_by_hand():
    """two rounds on one contig: c (100 bp) -> c:1-40, c:41-100; then c:41-100 -> c:41-70, c:71-100"""
    from haphic_amd import correct
    args = types.SimpleNamespace(RE='GATC')
    seq = ''.join(random.Random(1).choice('ACGT') for _ in range(100))
    fa = {'a': ['AC', 2, 1], 'c': [seq, 100, _count_gatc(seq, 'GATC')], 'z': ['GG', 2, 1]}
    depth = {'a': (0, 9), 'c': (1, 30), 'z': (0, 4)}
    unbroken = set(fa)
    source, fpos, ffrag = {'c': 'c'}, {'c': [0]}, {'c': ['c']}
    kids = correct.update_bookkeeping({'c': [(40, 3)]}, source, fpos, ffrag, fa, depth, unbroken, args, count_re=_count_gatc)
    assert kids == {'c': ['c:1-40', 'c:41-100']}
    assert list(fa) == ['a', 'z', 'c:1-40', 'c:41-100'] and fa['c:41-100'] == [seq[40:], 60, _count_gatc(seq[40:], 'GATC')]
    assert ffrag == {'c': ['c:41-100', 'c:1-40']} and fpos == {'c': [40, 0]}
    assert list(depth) == ['a', 'z', 'c:1-40', 'c:41-100'] and depth['c:1-40'] == (1, 30)
    unbroken -= {'c'}
    kids = correct.update_bookkeeping({'c:41-100': [(30, 0)]}, source, fpos, ffrag, fa, depth, unbroken, args, count_re=_count_gatc)
    assert kids == {'c:41-100': ['c:41-70', 'c:71-100']}
    assert ffrag == {'c': ['c:71-100', 'c:41-70', 'c:1-40']} and fpos == {'c': [70, 40, 0]}
    assert fa['c:71-100'][0] == seq[70:] and fa['c:41-70'][:2] == [seq[40:70], 30]
    assert source == {'c': 'c', 'c:1-40': 'c', 'c:41-100': 'c', 'c:41-70': 'c', 'c:71-100': 'c'}
    sources, off, pos, new = correct._remap_tables(list(fa), fpos, ffrag)
    assert sources == ['a', 'z', 'c'] and off.tolist() == [0, 1, 2, 5]
    assert pos.tolist() == [0, 0, 0, 40, 70] and new.tolist() == [0, 1, 2, 3, 4]


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_bookkeeping_against_the_reference_function(monkeypatch):
    """break_and_update_ctgs(last_round=True) of the reference touches the dicts alone (:1151 :1176 :1188): three rounds of random
    break points through it and through update_bookkeeping, all seven dicts equal in content and order after every round"""
    H = _load_reference(monkeypatch)
    from haphic_amd import correct
    rng = random.Random(7)
    res = 10
    args = types.SimpleNamespace(RE='GATC', correct_resolution=res)
    for with_depth in (True, False):
        fa = {}
        for k in range(30):
            seq = ''.join(rng.choice('ACGT') for _ in range(rng.randrange(200, 900)))
            fa['ctg%d' % k] = [seq, len(seq), H.count_RE_sites(seq, 'GATC')]
        depth = {n: (k % 2, 10 + k) for k, n in enumerate(fa)} if with_depth else {}
        state = [dict(fa=copy.deepcopy(fa), depth=dict(depth), unbroken=set(fa), source={}, fpos={}, ffrag={}) for _ in range(2)]
        for rnd in range(3):
            cur = state[0]['fa']
            cand = [n for n in cur if rnd == 0 or n not in state[0]['unbroken']]
            bp = {}
            for n in cand:
                if rng.random() < 0.5 and cur[n][1] > 6 * res:
                    k = rng.choice((1, 1, 2, 3))
                    pts = sorted(rng.sample(range(1, cur[n][1] // res), k))
                    bp[n] = [(p * res, 0 if k > 1 else rng.choice((0, 4))) for p in pts]
            assert bp
            for st in state:
                if rnd == 0:
                    for n in bp:
                        st['source'][n], st['fpos'][n], st['ffrag'][n] = n, [0], [n]
            a, b = state
            H.break_and_update_ctgs(bp, None, None, a['source'], a['fpos'], a['ffrag'], a['fa'], a['depth'], a['unbroken'], args, True)
            kids = correct.update_bookkeeping(bp, b['source'], b['fpos'], b['ffrag'], b['fa'], b['depth'], b['unbroken'], args,
                                              count_re=H.count_RE_sites)
            for st in state:
                st['unbroken'] -= set(bp)
            for key in ('fa', 'depth', 'source', 'fpos', 'ffrag'):
                assert a[key] == b[key] and list(a[key]) == list(b[key]), (rnd, key)
            assert list(kids) == list(bp) and all(set(v) <= set(b['fa']) for v in kids.values())
