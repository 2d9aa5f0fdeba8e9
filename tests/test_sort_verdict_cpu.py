"""The verdict of `haphic sort` (fast sorting or ALLHiC) on the CPU: the host engine of tests/sort_verdict_cases.py and the mirror of
haphic_amd/sort.py with that engine against tests/golden/sort_verdict.npz — the reference's own verdicts, log lines and sums — and, where the
checkout exists, against the reference's function itself; the opt-in binding of patch.patch_sort and the wrapper's flag."""
import os
import sys
import types

import numpy as np
import pytest

from haphic_amd import patch, sort
from tests import sort_cases
from tests import sort_verdict_cases as vc

HAVE_REF = os.path.isfile(os.path.join(sort_cases.REFERENCE_SCRIPTS, 'HapHiC_sort.py'))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason='needs the reference checkout (dev container only)')
CASES = [c.name for c in vc.cases()]


@pytest.fixture(scope='module')
def fx():
    return vc.Fixture()


def test_fixture_covers_the_corpus(fx):
    fx.self_check()


@pytest.mark.parametrize('case', CASES)
def test_stand_in_equals_the_golden_sums(fx, case):
    c = fx.case(case)
    lens = [c.lens[ctg] for ctg, _ in c.fast]
    assert np.array_equal(vc.stand_in(vc.values_of(c), lens), fx.sums(case))


def counting_engine(calls):
    def engine(value, lengths, r0, r1):
        calls.append((len(value), r0, r1))
        return vc.stand_in(value, lengths, r0, r1)
    return engine


@pytest.mark.parametrize('case', CASES)
def test_mirror_with_the_stand_in_gives_the_golden_verdict_and_log_line(fx, case, tmp_path):
    calls = []
    S = vc.fake_module()
    S.compare_fast_sort_and_allhic = sort.bind_verdict(S, counting_engine(calls))
    verdict, lines = vc.run_verdict(S, fx.case(case), tmp_path)
    assert verdict is fx.verdict(case) and lines == [fx.log(case)]
    n = len(fx.case(case).lens)
    want = {'ratio': [], 'first': [(n, 0, 1)], 'later': [(n, 0, 1), (n, 1, n - 1)], 'none': [(n, 0, 1), (n, 1, n - 1)]}[fx.outcome(case)]
    assert calls == (want[:1] if n == 2 else want)        # rotation 0 alone first, the rest in one call, nothing past the ratio rule


def test_mirror_hands_back_without_the_checkout(tmp_path):
    """one contig, a contig missing from the ALLHiC tour, a longer ALLHiC tour, lengths that are no ints, an engine that raises: the original"""
    handed = []
    S = vc.fake_module()
    S.compare_fast_sort_and_allhic = lambda prefix, fa_dict: handed.append(prefix) or 'original'
    calls = []
    mirror = sort.bind_verdict(S, counting_engine(calls))

    def run(case, fa=None):
        cwd = os.getcwd()
        os.chdir(str(tmp_path))
        try:
            fa_dict = vc.write_tours(case, case.name)
            fa_dict.update(fa or {})
            return mirror(case.name, fa_dict)
        finally:
            os.chdir(cwd)
    assert run(vc.Case('one', [(0, '+')], [(0, '+')], [5])) == 'original'
    assert run(vc.Case('missing', [(0, '+'), (1, '+'), (2, '-')], [(0, '+'), (1, '+'), (3, '-')], [5, 5, 5, 5])) == 'original'
    assert run(vc.Case('longer', [(0, '+'), (1, '+')], [(0, '+'), (1, '+'), (2, '-')], [5, 5, 5])) == 'original'
    assert run(vc.Case('floats', [(0, '+'), (1, '+')], [(1, '+'), (0, '+')], [5, 5]), {vc.ctg_name(0): 5.0}) == 'original'
    assert run(vc.Case('negative', [(0, '+'), (1, '+')], [(1, '+'), (0, '+')], [5, 5]), {vc.ctg_name(0): -5}) == 'original'
    assert run(vc.Case('huge', [(0, '+'), (1, '+')], [(1, '+'), (0, '+')], [1 << 61, 1 << 61])) == 'original'
    assert calls == [] and handed == ['one', 'missing', 'longer', 'floats', 'negative', 'huge']

    def refusing(value, lengths, r0, r1):
        raise sort.VerdictUnsupported('too many contigs')
    mirror = sort.bind_verdict(S, refusing)                # `run` reads the name at call time
    assert run(vc.Case('refused', [(0, '+'), (1, '+')], [(1, '+'), (0, '+')], [5, 5])) == 'original' and handed[-1] == 'refused'


# ------------------------------------------------------------------ against the reference's own function
@pytest.fixture(scope='module')
def modules():
    plain = sort_cases.load_reference_sort(name='_haphic_sort_reference_verdict_plain')
    ours = sort_cases.load_reference_sort(name='_haphic_sort_reference_verdict_patched')
    calls = []
    saved = patch.patch_sort(ours, engine=sort_cases.NumpyEngine, verdict=True, verdict_engine=counting_engine(calls))
    return plain, ours, calls, saved


@needs_ref
@pytest.mark.parametrize('case', [n for n in CASES if n != 'n1025'])        # the reference takes most of a minute there: the golden file holds it
def test_mirror_equals_the_reference_function(modules, fx, case, tmp_path):
    plain, ours, calls, _saved = modules
    del calls[:]
    want = vc.run_verdict(plain, fx.case(case), tmp_path)
    got = vc.run_verdict(ours, fx.case(case), tmp_path)
    assert got == want and got[0] is want[0]
    assert want[0] is fx.verdict(case) and want[1][-1] == fx.log(case)
    assert (calls == []) == (fx.outcome(case) == 'ratio')


def _outcome_of(S, case, tmp_path):
    try:
        return vc.run_verdict(S, case, tmp_path)
    except Exception as e:                                 # noqa: BLE001  (whatever the reference raises is the specification)
        return type(e), str(e)


@needs_ref
def test_handed_back_calls_behave_as_the_original(modules, tmp_path):
    plain, ours, calls, _saved = modules
    del calls[:]
    one = vc.Case('one', [(0, '+')], [(0, '+')], [5])
    missing = vc.Case('missing', [(0, '+'), (1, '+'), (2, '-')], [(0, '+'), (1, '+'), (3, '-')], [5, 5, 5, 5])
    for case in (one, missing):
        want, got = _outcome_of(plain, case, tmp_path), _outcome_of(ours, case, tmp_path)
        assert isinstance(want[0], type) and issubclass(want[0], Exception) and got[0] is want[0] and got[1] == want[1], case.name
    assert calls == []
    refused = []

    def refusing(value, lengths, r0, r1):
        refused.append(len(value))
        raise sort.VerdictUnsupported('too many contigs')
    theirs = sort_cases.load_reference_sort(name='_haphic_sort_reference_verdict_refusing')
    patch.patch_sort(theirs, engine=sort_cases.NumpyEngine, verdict=True, verdict_engine=refusing)
    case = vc.Fixture().case('shuffled_n65')
    want, got = vc.run_verdict(plain, case, tmp_path), vc.run_verdict(theirs, case, tmp_path)
    assert refused == [65] and got[0] is want[0] and got[1][-1] == want[1][-1]


# ------------------------------------------------------------------ binding
def _bare_module():
    S = vc.fake_module('sort_verdict_bare')
    for name in patch.SORT_SEAMS:
        setattr(S, name, (lambda name: lambda *a, **k: name)(name))
    S.Pool = object
    return S


def test_patch_sort_leaves_the_verdict_alone_by_default():
    S = _bare_module()
    original = S.compare_fast_sort_and_allhic
    saved = patch.patch_sort(S, engine=sort_cases.NumpyEngine)
    assert S.compare_fast_sort_and_allhic is original and 'compare_fast_sort_and_allhic' not in saved
    assert set(saved) == set(patch.SORT_SEAMS) | {'Pool'}
    assert 'compare_fast_sort_and_allhic' not in patch.SORT_SEAMS and patch.SORT_VERDICT_SEAMS == {'compare_fast_sort_and_allhic': 'HapHiC_sort.py:645-724'}


def test_patch_sort_binds_the_verdict_on_request_and_unpatch_restores_it(fx, tmp_path):
    S = _bare_module()
    original = S.compare_fast_sort_and_allhic
    calls = []
    saved = patch.patch_sort(S, engine=sort_cases.NumpyEngine, verdict=True, verdict_engine=counting_engine(calls))
    assert S.compare_fast_sort_and_allhic is not original and S.compare_fast_sort_and_allhic.__wrapped__ is original
    assert saved['compare_fast_sort_and_allhic'] is original
    verdict, lines = vc.run_verdict(S, fx.case('rot_1'), tmp_path)
    assert verdict is False and lines == [fx.log('rot_1')] and calls == [(8, 0, 1), (8, 1, 7)]
    patch.unpatch_reference(S, saved)
    assert S.compare_fast_sort_and_allhic is original and S.Pool is object


def test_wrapper_strips_the_flag(monkeypatch, tmp_path):
    """`python -m haphic_amd sort --keep-reference-verdict ...`: the flag decides patch_sort's `verdict` and never reaches the reference's parser"""
    from haphic_amd import __main__ as cli
    from haphic_amd import _lib
    (tmp_path / 'HapHiC_cluster.py').write_text('')
    seen = {}
    fake = types.ModuleType('HapHiC_sort')
    fake.parse_arguments = lambda: seen.setdefault('argv', list(sys.argv))
    fake.run = lambda args, log: seen.setdefault('log', log)
    monkeypatch.setitem(sys.modules, 'HapHiC_sort', fake)
    monkeypatch.setattr(_lib, 'load', lambda: types.SimpleNamespace(hhx_set_device=lambda d: 0))
    monkeypatch.setattr(patch, 'patch_sort', lambda S, **kw: seen.setdefault('kw', []).append(kw))
    monkeypatch.setattr(sys, 'argv', list(sys.argv))
    monkeypatch.setattr(sys, 'path', list(sys.path))
    monkeypatch.setattr(sort, 'DEVICE', None)
    rest = ['asm.fa', 'HT_links.pkl', 'split_clms', 'group1.txt']
    assert cli.main(['sort', '--reference', str(tmp_path), '--keep-reference-verdict'] + rest) == 0
    assert seen['argv'] == ['haphic sort'] + rest and seen['kw'] == [{'verdict': False}]
    seen.pop('argv')
    assert cli.main(['sort', '--reference', str(tmp_path)] + rest) == 0
    assert seen['argv'] == ['haphic sort'] + rest and seen['kw'][-1] == {'verdict': True}
    assert '--keep-reference-verdict' in cli.__doc__
