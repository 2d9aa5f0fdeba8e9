#!/usr/bin/env python3
"""Generate tests/golden/reassign_rounds.npz by running the REFERENCE's own run_reassignment :266-427 (the round loop of run() :865-880) and
agglomerative_hierarchical_clustering :489-560 of HapHiC_reassign.py on small synthetic jobs.

Run in the dev container only (needs /root/reference):
    PYTHONHASHSEED=0 python tests/golden/make_golden_reassign_rounds.py
Every case records its inputs as arrays, the state after every call of run_reassignment, and the agglomerative step's group-pair sums, file
and distance matrix.  The numpy engine of tests/reassign_cases.py is run beside the reference, call by call and contig by contig (the
reference's DEBUG lines), and must agree; what the cases have to contain between them (ISSUE list below, COVERAGE) is asserted from it."""
import logging
import os
import re
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}),
                    ('portion', {'closed': None, 'empty': None})):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
sys.path.insert(0, '/root/reference/scripts')
import HapHiC_reassign as R  # noqa: E402

from tests import reassign_cases as rc  # noqa: E402

COVERAGE = ('consistent', 'rescued', 'reassigned', 'not_rescued', 'nr_re', 'nr_links', 'nr_ambiguous', 'nr_density', 'nr_ratio', 'cascade',
            'tie_by_first', 'tie_by_move', 'zero_and_back', 'dismissal', 'gfa_on', 'gfa_off', 'too_long_to_move', 'converged', 'not_converged')

DEBUG_CODES = (('too few RE sites', rc.NR_RE), ('too few Hi-C links,', rc.NR_LINKS), ('(ambiguous', rc.NR_AMBIGUOUS),
               ('too low Hi-C links density', rc.NR_DENSITY), ('too low density ratio', rc.NR_RATIO), ('is consistent', rc.CONSISTENT),
               ('is rescued', rc.RESCUED), ('is reassigned', rc.REASSIGNED))

DEFAULT = dict(n_groups=7, max_links=60, p_in=0.35, p_out=0.04, ungrouped=0.2, min_links=25, min_link_density=0.0001, ambiguous_cutoff=0.6,
               min_density_ratio=4, gfa=None, min_group_len=0, max_ctg_len=10000, nclusters=3)
CASES = (('defaults', dict(seed=11)),
         ('ties_gfa', dict(seed=12, n_groups=12, max_links=3, p_in=0.30, p_out=0.02, ungrouped=0.6, min_links=1, ambiguous_cutoff=1.5,
                           min_density_ratio=1.2, gfa='x', nclusters=2)),
         ('dismissal', dict(seed=13, n_groups=9, max_links=40, p_in=0.40, p_out=0.03, min_links=10, min_link_density=0.01, min_density_ratio=2,
                            min_group_len=2.2, max_ctg_len=60, nclusters=2)),
         ('restless', dict(seed=101, n_groups=4, max_links=2, p_in=0.10, p_out=0.10, min_links=1, ambiguous_cutoff=1.5, min_density_ratio=0.5,
                           nclusters=2)))


class Capture(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.debug, self.info = [], []

    def emit(self, record):
        (self.debug if record.levelno == logging.DEBUG else self.info).append(record.getMessage())


def run_case(name, seen, seed, n_groups, max_links, p_in, p_out, ungrouped, min_links, min_link_density, ambiguous_cutoff, min_density_ratio, gfa,
             min_group_len, max_ctg_len, nclusters):
    fi, fj, links, group, ctg_re, ctg_len = rc.build_case(seed, n_groups, max_links, p_in, p_out, ungrouped)
    n_ctg = len(group)
    names = ['c%03d' % k for k in range(n_ctg)]
    gnames = ['g%d' % g for g in range(n_groups)]
    min_RE_sites = 25
    full_link_dict = {(names[i], names[j]): int(v) for i, j, v in zip(fi.tolist(), fj.tolist(), links.tolist())}
    fa_dict = {names[k]: [None, int(ctg_len[k]), int(ctg_re[k])] for k in range(n_ctg)}
    RE_site_dict = {names[k]: int(ctg_re[k]) for k in range(n_ctg)}
    order = np.argsort(-ctg_len, kind='stable').astype(np.int32)
    sorted_ctg_list = [(names[k], int(ctg_len[k])) for k in order.tolist()]
    ctg_group_dict, group_RE_dict = {}, {g: 1 for g in gnames}
    for k in np.argsort(group, kind='stable').tolist():                 # as parse_clusters :144-167 fills them: group by group
        if group[k] >= 0:
            ctg_group_dict[names[k]] = gnames[group[k]]
            group_RE_dict[gnames[group[k]]] += int(ctg_re[k]) - 1
    grouped_ctgs = R.add_ungrouped_ctgs(fa_dict, ctg_group_dict)
    group_re0 = np.array([group_RE_dict[g] for g in gnames], np.int64)
    gid = {g: k for k, g in enumerate(gnames)}
    gid['ungrouped'] = -1

    case = dict(fi=fi, fj=fj, links=links, group0=group, group_re0=group_re0, ctg_re=ctg_re, ctg_len=ctg_len, order=order,
                min_RE_sites=np.int64(min_RE_sites), min_links=np.float64(min_links), min_link_density=np.float64(min_link_density),
                min_density_ratio=np.float64(min_density_ratio), ambiguous_cutoff=np.float64(ambiguous_cutoff), gfa=np.bool_(bool(gfa)),
                min_group_len=np.float64(min_group_len), max_ctg_len=np.float64(max_ctg_len))

    cap = Capture()
    R.logger.addHandler(cap)
    R.logger.setLevel(logging.DEBUG)
    R.logger.propagate = False
    ctg_group_link_dict, linked_ctg_dict = R.parse_link_dict(full_link_dict, ctg_group_dict)
    engine = rc.NumpyReassign(fi, fj, links, n_ctg, group, n_groups)
    e_group, e_re = group.copy(), group_re0.copy()
    flags = rc.case_flags(case)
    rounds, groups, res, counts, info = [], [], [], [], []

    def call(nround):
        cap.debug.clear()
        # the engine first: the frozen judgement of every contig, then its own walk
        dismissed = rc.case_dismissed(case, e_group) if nround > 1 else None
        if dismissed is not None and dismissed.any():
            seen.add('dismissal')
        args = (float(min_links), min_link_density, float(min_density_ratio), float(ambiguous_cutoff), nround == 0, bool(gfa), 0)
        probe = rc.NumpyReassign([], [], [], n_ctg, e_group, n_groups)
        probe.sum, probe.stamp = engine.sum.copy(), engine.stamp.copy()
        f_group = e_group.copy()
        if dismissed is not None:
            f_group[np.isin(f_group, np.flatnonzero(dismissed))] = -1
            probe.sum[:, np.flatnonzero(dismissed)] = 0
        frozen = [probe.judge(c, f_group, e_re, ctg_re, flags, *args) for c in order.tolist()]
        e_counts = engine.round(e_group, e_re, ctg_re, order, flags, dismissed, *args)
        R.run_reassignment(sorted_ctg_list, ctg_group_link_dict, ctg_group_dict, full_link_dict, linked_ctg_dict, fa_dict, RE_site_dict, gfa,
                           group_RE_dict, max_ctg_len, min_RE_sites, min_links, min_link_density, min_density_ratio, ambiguous_cutoff,
                           min_group_len, set(), nround)
        g_now = np.array([gid[ctg_group_dict[c]] for c in names], np.int32)
        re_now = np.array([group_RE_dict[g] for g in gnames], np.int64)
        line = cap.info[-1]
        c_now = np.array([int(x) for x in re.search(r'consistent: (\d+), rescued: (\d+), reassigned: (\d+), not rescued: (\d+)', line).groups()], np.int64)
        verdicts = [next(code for text, code in DEBUG_CODES if text in msg) for msg in cap.debug]
        # a contig without a non-zero cell: "too few RE sites" (no inner dict) or, once a dismissal has inserted zeros, "too few Hi-C links"
        same = lambda v: rc.NR_RE if v == rc.NR_LINKS else v            # noqa: E731
        assert [same(v) for v in verdicts] == [same(v) for v in engine.last_verdicts.tolist()], (name, nround)
        assert (g_now == e_group).all() and (re_now == e_re).all() and (c_now == e_counts).all(), (name, nround)
        for v, (fv, _t) in zip(verdicts, frozen):
            if v != fv:
                seen.add('cascade')
        for code, key in ((rc.NR_RE, 'nr_re'), (rc.NR_LINKS, 'nr_links'), (rc.NR_AMBIGUOUS, 'nr_ambiguous'), (rc.NR_DENSITY, 'nr_density'),
                          (rc.NR_RATIO, 'nr_ratio')):
            if code in verdicts:
                seen.add(key)
        for k, key in enumerate(('consistent', 'rescued', 'reassigned', 'not_rescued')):
            if c_now[k]:
                seen.add(key)
        rounds.append(nround); groups.append(g_now); res.append(re_now); counts.append(c_now); info.append(line)

    last_round = None
    converged = False
    for n in range(5):                                                   # run() :865-880
        call(n + 1)
        if n > 0 and last_round == ctg_group_dict:
            converged = True
            break
        last_round = ctg_group_dict.copy()
    seen.add('converged' if converged else 'not_converged')
    call(0)
    seen.update(engine.events)
    seen.add('gfa_on' if gfa else 'gfa_off')
    R.logger.removeHandler(cap)
    R.logger.setLevel(logging.WARNING)
    case.update(nrounds=np.array(rounds, np.int32), groups=np.array(groups, np.int32), group_res=np.array(res, np.int64),
                counts=np.array(counts, np.int64), info=np.array(info))

    # ---- the agglomerative step as run() :882-896 reaches it
    here = os.getcwd()
    recorded = {}

    class Recorder(R.AgglomerativeClustering):
        def fit_predict(self, X, y=None):
            recorded['matrix'] = np.array(X, np.float64)
            return super().fit_predict(X, y)
    real = R.AgglomerativeClustering
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.mkdir('reassigned_groups')
            group_ctg_dict, group_hiconf_RE_dict = R.stat_clusters(ctg_group_dict, fa_dict, grouped_ctgs)
            new_ctg_group_dict, new_group_ctg_dict, new_old_group_dict = R.clusters_output(group_ctg_dict, fa_dict, 'reassigned')
            assert nclusters < len(new_group_ctg_dict), (name, len(new_group_ctg_dict), counts)
            new_names = list(new_old_group_dict)
            nid = {g: k for k, g in enumerate(new_names)}
            first = {}
            for pos, ((a, b), v) in enumerate(full_link_dict.items()):   # :496-508, only to note where each pair is first met
                if a in grouped_ctgs and b in grouped_ctgs and a in new_ctg_group_dict and b in new_ctg_group_dict:
                    ga, gb = new_ctg_group_dict[a], new_ctg_group_dict[b]
                    if ga != gb:
                        first.setdefault(tuple(sorted([ga, gb])), pos)
            os.mkdir('hc_groups')
            R.AgglomerativeClustering = Recorder
            hc = R.agglomerative_hierarchical_clustering(full_link_dict, grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict,
                                                         nclusters)
            txt = open('hc_groups/group_group_links.txt', 'rb').read()
        finally:
            R.AgglomerativeClustering = real
            os.chdir(here)
    rows = [line.split('\t') for line in txt.decode().splitlines()[1:]]
    assert [(r[0], r[1]) for r in rows] == list(first), name
    case.update(agg_member=np.array([c in grouped_ctgs for c in names], np.uint8),
                agg_group=np.array([nid.get(new_ctg_group_dict.get(c), -1) for c in names], np.int32),
                agg_names=np.array(new_names), agg_hiconf_re=np.array([group_hiconf_RE_dict[new_old_group_dict[g]] for g in new_names], np.int64),
                agg_pairs=np.array([(nid[r[0]], nid[r[1]], int(r[2]), first[(r[0], r[1])]) for r in rows], np.int64).reshape(-1, 4),
                agg_txt=np.frombuffer(txt, np.uint8), agg_matrix=recorded['matrix'], agg_nclusters=np.int64(nclusters),
                agg_clusters=np.array([sorted(nid[g] for g in hc[k]) + [-1] * (len(new_names) - len(hc[k])) for k in sorted(hc)], np.int32))
    print('%-10s calls %s  counts %s  pairs %d' % (name, rounds, counts[0].tolist(), len(rows)))
    return case


def main():
    seen = set()
    out = {}
    for name, spec in CASES:
        for field, value in run_case(name, seen, **dict(DEFAULT, **spec)).items():
            out['%s/%s' % (name, field)] = value
    missing = [c for c in COVERAGE if c not in seen]
    assert not missing, 'the cases do not contain: %s' % missing
    path = os.path.join(HERE, 'reassign_rounds.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
