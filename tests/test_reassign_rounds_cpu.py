"""CPU: the rounds of `haphic reassign` (HapHiC_reassign.py run_reassignment :266-427) and the agglomerative step's group-pair sums.
  * the numpy engine of tests/reassign_cases.py against tests/golden/reassign_rounds.npz, which the reference's own functions wrote: every case,
    every call (the rescue round included): groups, group_RE values, the four counts; the pair sums and their first positions.  This pins the
    engine the GPU test at 2 100 groups leans on;
  * the engine's two summation modes on quotient lists where they differ;
  * where the reference checkout is present: the round loop of run() :855-880 and the agglomerative step through
    patch_reassign(R, rounds=True, engine=NumpyReassign) against the unpatched functions on a fresh random job: dicts (with their key order), log
    lines and files equal."""
import copy
import logging
import os
import sys
import types

import numpy as np
import pytest

from tests import reassign_cases as rc

REF = '/root/reference/scripts'
CASES = rc.load_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_numpy_engine_against_the_reference_rounds(name):
    case = CASES[name]
    engine = rc.NumpyReassign(case['fi'], case['fj'], case['links'], len(case['group0']), case['group0'], len(case['group_re0']))
    out = rc.run_job(case, engine)
    assert len(out) == len(case['nrounds']) >= 3
    for k, (nround, group, group_re, counts) in enumerate(out):
        assert (group == case['groups'][k]).all(), (name, nround)
        assert (group_re == case['group_res'][k]).all(), (name, nround)
        assert counts.tolist() == case['counts'][k].tolist(), (name, nround)
        assert counts.sum() == len(case['order'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_numpy_engine_pair_sums(name):
    case = CASES[name]
    engine = rc.NumpyReassign(case['fi'], case['fj'], case['links'], len(case['group0']), case['group0'], len(case['group_re0']))
    rc.check_pair_sums(case, *engine.pair_sums(case['agg_member'], case['agg_group'], len(case['agg_names'])))


def test_the_two_sums_differ_where_the_test_says_they_do():
    values = rc.compensation_quotients()
    assert rc.python_sum(values, 0) != rc.python_sum(values, 1)
    assert rc.python_sum(values, 1 if sys.version_info >= (3, 12) else 0) == sum(values)


def _reference():
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import HapHiC_reassign as R
    return R


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _whole_job(R, d, nclusters, tmp):
    """run() :855-896 through the names R holds, in directory tmp -> what it leaves behind"""
    lines = _Lines()
    R.logger.addHandler(lines)
    level = R.logger.level
    R.logger.setLevel(logging.INFO)
    here = os.getcwd()
    os.makedirs(tmp)
    os.chdir(tmp)
    try:
        rc.drive_rounds(R, d)
        os.mkdir('reassigned_groups')
        group_ctg_dict, group_hiconf_RE_dict = R.stat_clusters(d['ctg_group_dict'], d['fa_dict'], d['grouped_ctgs'])
        new_ctg_group_dict, new_group_ctg_dict, new_old_group_dict = R.clusters_output(group_ctg_dict, d['fa_dict'], 'reassigned')
        assert nclusters < len(new_group_ctg_dict)
        os.mkdir('hc_groups')
        hc = R.agglomerative_hierarchical_clustering(d['full_link_dict'], d['grouped_ctgs'], new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict,
                                                     nclusters, normalize_by_nlinks=False)
        txt = open('hc_groups/group_group_links.txt', 'rb').read()
    finally:
        os.chdir(here)
        R.logger.removeHandler(lines)
        R.logger.setLevel(level)
    return dict(ctg_group=list(d['ctg_group_dict'].items()), group_re=list(d['group_RE_dict'].items()), lines=lines.lines, txt=txt,
                hc=sorted(sorted(v) for v in hc.values()))


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
@pytest.mark.parametrize('spec', [dict(seed=501, n_groups=8, max_links=50, p_in=0.35, p_out=0.04, ungrouped=0.25),
                                  dict(seed=502, n_groups=6, max_links=3, p_in=0.3, p_out=0.05, ungrouped=0.5)], ids=['dense', 'ties'])
def test_seams_against_the_unpatched_reference(spec, tmp_path):
    from haphic_amd import patch, reassign
    R = _reference()
    fi, fj, links, group, ctg_re, ctg_len = rc.build_case(**spec)
    group_re = np.ones(spec['n_groups'], np.int64)
    np.add.at(group_re, group[group >= 0], ctg_re[group >= 0] - 1)
    few_links = spec['max_links'] < 10
    case = dict(fi=fi, fj=fj, links=links, group0=group, group_re0=group_re, ctg_re=ctg_re, ctg_len=ctg_len,
                order=np.argsort(-ctg_len, kind='stable').astype(np.int32), gfa=np.bool_(few_links), max_ctg_len=np.float64(80), min_RE_sites=np.int64(25),
                min_links=np.float64(1 if few_links else 25), min_link_density=np.float64(0.0001), min_density_ratio=np.float64(1.5 if few_links else 4),
                ambiguous_cutoff=np.float64(1.5 if few_links else 0.6), min_group_len=np.float64(0 if few_links else 1.5))
    theirs = _whole_job(R, rc.case_dicts(case), 2, str(tmp_path / 'theirs'))
    assert theirs['lines'][-3].startswith('[result::additional_rescue]') and 'rescued: 0, reassigned: 0' not in theirs['lines'][1]
    saved = patch.patch_reassign(R, rounds=True, engine=rc.NumpyReassign)
    try:
        assert set(saved) == {'parse_link_dict', 'split_clm_file', 'run_reassignment', 'agglomerative_hierarchical_clustering'}
        d = rc.case_dicts(case)
        ours = _whole_job(R, d, 2, str(tmp_path / 'ours'))
        tables = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
        assert type(tables[0]) is reassign.RoundTable and type(tables[1]) is reassign.RoundTable
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)
    assert ours == theirs


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_thaw_before_the_first_round_is_the_reference_result(tmp_path):
    from haphic_amd import patch
    R = _reference()
    d = rc.case_dicts(CASES['defaults'])
    theirs = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
    saved = patch.patch_reassign(R, rounds=True, engine=rc.NumpyReassign)
    try:
        ours = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
        again = R.parse_link_dict(d['full_link_dict'], d['ctg_group_dict'])
        assert [(c, list(inner.items())) for c, inner in ours[0].items()] == [(c, list(inner.items())) for c, inner in theirs[0].items()]
        assert list(ours[1].items()) == list(theirs[1].items())
        assert type(ours[0]).__name__ == 'Thawed' and ours[0].default_factory is dict and ours[1].default_factory is set
        rc.call_round(R, d, again, 1)
        with pytest.raises(RuntimeError, match='on the device'):
            again[0]['c000']
        with pytest.raises(RuntimeError, match='on the device'):
            len(again[1])
    finally:
        for name, fn in saved.items():
            setattr(R, name, fn)
    assert copy.copy(ours[0]) == theirs[0]
