"""Stage 2 of --remove_allelic_links (links between non-maximum matches :621-667) without a GPU:
  * allelic.lsap_small — the step-by-step restatement of scipy's solver, the CPU oracle of the device solver — equals
    scipy.optimize.linear_sum_assignment on exhaustive small matrices and random ones with ties (tests/allelic_stage2_cases.py);
  * the mirror hands stage 2 to an engine that offers `nonmax_keys` (what the real engine's device form looks like to it), falls through to the
    host form on NotImplemented, and to the reference's own function on None."""
import numpy as np
import pytest

from tests import allelic_cases, allelic_stage2_cases as s2
from tests.test_allelic_cases_cpu import CASES, _call, check_verdict, frozen_groups, golden, mirror   # noqa: F401 (golden, mirror: fixtures)


@pytest.mark.parametrize('name', list(s2.families()))
def test_lsap_small_equals_scipy(name):
    from haphic_amd import allelic
    matrices, want = s2.families()[name], s2.family_answers()[name]
    for k, m in enumerate(matrices):
        got = allelic.lsap_small(-m)
        assert np.array_equal(got, want[k]), (name, k, m.tolist(), got.tolist(), want[k].tolist())


def test_lsap_small_wide_counts():
    from haphic_amd import allelic
    matrices = s2.wide_counts(n=200)
    want = s2.scipy_col4row(matrices)
    assert int(matrices.max()) > 2 ** 39
    for k, m in enumerate(matrices):
        assert np.array_equal(allelic.lsap_small(-m), want[k]), k


def test_families_are_the_stated_ones():
    fam = s2.families()
    assert sum(len(m) for m in fam.values()) == 3 + 81 + 19683 + 65536 + 22500
    assert {m.shape[1] for m in fam.values()} == set(range(1, 9))
    # ties are the rule: most matrices have several optimal assignments of different shape — scipy's choice is what is pinned
    m = fam['random 6x6 below 2']
    assert (m.sum(axis=(1, 2)) > 6).mean() > 0.9


def _engine(mirror, answer):  # noqa: F811
    """binds the mirror's library to an engine whose nonmax_keys records the call and answers with the host function ('host function') or `answer`"""
    calls = []

    class Engine(allelic_cases.Ingest):
        def nonmax_keys(self, si, sj, scnt, groups, names, ctg_rank, stats=None):
            calls.append(len(si))
            if answer == 'host function':
                return mirror.allelic.nonmax_keys(si, sj, scnt, groups, names, ctg_rank, stats)
            return answer
    mirror.lib.Ingest = Engine
    return Engine, calls


@pytest.mark.parametrize('name', ['p2', 'p4'])
def test_mirror_takes_the_engines_stage_2(mirror, golden, name):  # noqa: F811
    case = CASES[name]
    Engine, calls = _engine(mirror, 'host function')
    groups = frozen_groups(golden, case) if case.ploidy > 2 else None
    got = allelic_cases.run_mirror(case, mirror.cluster, mirror.allelic, groups=groups)
    assert isinstance(got['session'].ing, Engine) and len(calls) == 1 and calls[0] > 0
    check_verdict(got, golden, case, mirror.cluster)
    st = mirror.allelic.STATS
    assert st['stage2_engine'] == 'device' and st['stage2_keys'] == int(golden[name + '_nonmax'].sum()) and st['group_pairs'] > 0
    assert not mirror.containers.THAW_LOG


def test_mirror_without_the_method_keeps_the_host_form(mirror, golden):  # noqa: F811
    case = CASES['p2']
    got = allelic_cases.run_mirror(case, mirror.cluster, mirror.allelic)
    check_verdict(got, golden, case, mirror.cluster)
    assert mirror.allelic.STATS['stage2_engine'] == 'host'


def test_not_implemented_falls_through_to_the_host_form(mirror, golden):  # noqa: F811
    case = CASES['p4']
    _Engine, calls = _engine(mirror, NotImplemented)
    got = allelic_cases.run_mirror(case, mirror.cluster, mirror.allelic, groups=frozen_groups(golden, case))
    assert len(calls) == 1
    check_verdict(got, golden, case, mirror.cluster)
    st = mirror.allelic.STATS
    assert st['stage2_engine'] == 'host' and st['stage2_keys'] == int(golden['p4_nonmax'].sum()) and st['assignments'] > 0
    assert not mirror.containers.THAW_LOG


def test_none_goes_to_the_original(mirror):  # noqa: F811
    """an `assert` of :652-659 would fail somewhere: the reference's own function raises it"""
    _Engine, calls = _engine(mirror, None)
    out, original_calls, kw = _call(mirror, CASES['p2'], lambda kw: None)
    assert len(calls) == 1 and out == {'from the original'} and len(original_calls) == 1
    assert len(kw['full_link_dict']) == 5053                     # nothing was dropped before the hand-over


def test_real_engine_is_told_by_its_type_and_the_environment(monkeypatch):
    """the device form is for the library's own Ingest; HAPHIC_ALLELIC_STAGE2 turns it on and off"""
    from haphic_amd import _lib, allelic
    real = object.__new__(_lib.Ingest)                           # no handle behind it: only its type is looked at
    real.h = None
    monkeypatch.setenv('HAPHIC_ALLELIC_STAGE2', 'device')
    assert allelic._stage2(real) == (allelic.nonmax_keys_device, 'device')
    monkeypatch.setenv('HAPHIC_ALLELIC_STAGE2', 'host')
    assert allelic._stage2(real) == (allelic.nonmax_keys, 'host')
    monkeypatch.delenv('HAPHIC_ALLELIC_STAGE2')
    assert allelic._stage2(real)[1] == allelic.STAGE2_DEFAULT and allelic.STAGE2_DEFAULT in ('device', 'host')
    assert allelic._stage2(object()) == (allelic.nonmax_keys, 'host')
