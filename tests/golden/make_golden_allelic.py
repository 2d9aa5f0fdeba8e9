#!/usr/bin/env python3
"""tests/golden/allelic.npz: the REFERENCE's remove_allelic_HiC_links :474-692 on the cases of tests/allelic_cases.py.

Run in the dev container only (it imports the reference at run time, as make_golden.py does):
    python tests/golden/make_golden_allelic.py
Per case: parse_alignments* -> (normalize_by_nlinks) -> remove_allelic_HiC_links of the reference, with a profile hook that reads the
function's own locals when it returns (inter_allele_dict, unique_allele_groups, nonmax_ctg_pair_set).  Frozen, as integers / masks / float64:
the concordance ratio of every eligible key, the stage-1 keys, the allele groups as id arrays, which keys of full / flank_link_dict left
(dict order), remaining_frags, the items of full_links.pkl and the dict_to_matrix index map.  Data only."""
import os
import sys
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
import HapHiC_cluster as H  # noqa: E402

H.logger.setLevel('WARNING')

from tests import allelic_cases  # noqa: E402


def gen_case(case, out):
    t = case.name + '_'
    fa, args = case.fa_dict(), case.args()
    full, flank, frag_link, coord, c2f = case.parse(H)
    if case.normalize:
        H.normalize_by_nlinks(flank, frag_link)
    cid = {n: k for k, n in enumerate(case.names)}
    fid = {n: k for k, n in enumerate(case.frag_names)}
    pre_full, pre_flank = list(full), list(flank)
    assert list(coord) == pre_full
    # cal_concordance_ratio of every eligible key: the collapsed entries hold it, the others are evaluated as :589-591 does
    eligible = np.zeros(len(pre_full), bool)
    ratio = np.full(len(pre_full), -1.0)
    for k, key in enumerate(pre_full):
        data = coord[key]
        if isinstance(data, list):
            eligible[k], ratio[k] = True, data[0]
        elif len(data) >= args.min_read_pairs * 2:
            eligible[k] = True
            ratio[k] = H.cal_concordance_ratio(data, min(fa[key[0]][1], fa[key[1]][1]), args.nwindows)
    grabbed = {}

    def hook(frame, event, arg):
        if event == 'return' and frame.f_code.co_name == 'remove_allelic_HiC_links':
            loc = frame.f_locals
            grabbed.update(inter=list(loc['inter_allele_dict']), groups=sorted(loc['unique_allele_groups']), nonmax=set(loc['nonmax_ctg_pair_set']))
    sys.setprofile(hook)
    try:
        remaining = H.remove_allelic_HiC_links(fa, coord, full, args, flank, set(case.filtered), c2f)
    finally:
        sys.setprofile(None)
    stage1 = set(grabbed['inter'])
    groups = grabbed['groups']
    mat, fidx = H.dict_to_matrix(flank, remaining, dense_matrix=False, add_self_loops=True)
    out.update({
        t + 'checksum': np.int64(case.checksum), t + 'n_ctg': np.int64(len(case.names)), t + 'n_frag': np.int64(len(case.frag_names)),
        t + 'full_i': np.array([cid[a] for a, _ in pre_full], np.int32), t + 'full_j': np.array([cid[b] for _, b in pre_full], np.int32),
        t + 'flank_i': np.array([fid[a] for a, _ in pre_flank], np.int32), t + 'flank_j': np.array([fid[b] for _, b in pre_flank], np.int32),
        t + 'eligible': eligible, t + 'ratio': ratio,
        t + 'stage1': np.array([k in stage1 for k in pre_full], bool),
        t + 'nonmax': np.array([k in grabbed['nonmax'] for k in pre_full], bool),
        t + 'group_ptr': np.cumsum([0] + [len(g) for g in groups]).astype(np.int64),
        t + 'group_ctg': np.array([cid[c] for g in groups for c in g], np.int32),
        t + 'full_removed': np.array([k not in full for k in pre_full], bool),
        t + 'flank_removed': np.array([k not in flank for k in pre_flank], bool),
        t + 'remaining': np.array([f in remaining for f in case.frag_names], bool),
        t + 'pkl_i': np.array([cid[a] for a, _ in full], np.int32), t + 'pkl_j': np.array([cid[b] for _, b in full], np.int32),
        t + 'pkl_cnt': np.array(list(full.values()), np.int64),
        t + 'frag_index': np.array([fidx.get(f, -1) for f in case.frag_names], np.int32),
        t + 'matrix_nnz': np.int64(mat.nnz),
    })
    if case.normalize:
        out[t + 'flank_val'] = np.array(list(flank.values()), np.float64)
    print('allelic case', case.name, 'ctgs', len(case.names), 'frags', len(case.frag_names), 'pairs', len(case.id1), 'keys', len(pre_full),
          'eligible', int(eligible.sum()), 'stage 1', len(stage1), 'groups', len(groups), 'non-max', len(grabbed['nonmax']),
          'full removed', int(out[t + 'full_removed'].sum()), 'flank removed', int(out[t + 'flank_removed'].sum()), 'of', len(pre_flank),
          'fragments kept', len(remaining), 'of', len(case.filtered))


if __name__ == '__main__':
    out = {'cases': np.array([c.name for c in allelic_cases.cases()])}
    for case in allelic_cases.cases():
        gen_case(case, out)
    path = os.path.join(HERE, 'allelic.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
