#!/usr/bin/env python3
"""tests/golden/statistics.npz: the REFERENCE's output_statistics :2279-2478 on the cases of tests/statistics_cases.py.

Run in the dev container only (it imports the reference at run time, as make_golden.py does):
    python tests/golden/make_golden_statistics.py
Per case: fa_dict, full_link_dict and result_clusters_list as plain Python objects through the reference's function in a scratch directory; frozen
are the inputs (names, lengths, RE sites, keys and counts in dict order, the clusters of every inflation) and the bytes of the four
*_statistics.txt files of every inflation.  Data only.  The interpreter that runs this decides how sum() :2376 adds (plainly up to CPython 3.11):
`sum_mode` records it."""
import os
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
import HapHiC_cluster as H  # noqa: E402

H.logger.setLevel('WARNING')

from tests import statistics_cases  # noqa: E402

TITLES = ('RE_site_threshold', 'Link_threshold', 'Link_density_threshold', 'Link_density_ratio_threshold')


def gen_case(case, out):
    t = case.name + '_'
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for label, _clusters in case.sets:
                os.mkdir('inflation_{}'.format(label))
            H.output_statistics(case.fa_dict(), case.link_dict(), case.result_clusters_list())
            for label, _clusters in case.sets:
                for title in TITLES:
                    with open('inflation_{}/{}_statistics.txt'.format(label, title), 'rb') as f:
                        out['{}file_{}_{}'.format(t, label, title)] = np.frombuffer(f.read(), np.uint8)
        finally:
            os.chdir(here)
    out.update({
        t + 'names': np.array(case.names), t + 'lengths': case.lengths, t + 're_sites': case.re_sites,
        t + 'fi': case.fi, t + 'fj': case.fj, t + 'cnt': case.cnt, t + 'handle': np.bool_(case.handle),
        t + 'labels': np.array([label for label, _c in case.sets]),
    })
    for label, clusters in case.sets:
        out['{}cluster_ptr_{}'.format(t, label)] = np.cumsum([0] + [len(c) for c in clusters]).astype(np.int64)
        out['{}cluster_ctg_{}'.format(t, label)] = np.array([c for cluster in clusters for c in cluster], np.int32)
    print('statistics case', case.name, 'contigs', case.n_ctg, 'keys', len(case.fi), 'sets', [(label, len(c)) for label, c in case.sets])


if __name__ == '__main__':
    cases = statistics_cases.fixture_cases()
    out = {'cases': np.array([c.name for c in cases]), 'sum_mode': np.int64(1 if sys.version_info >= (3, 12) else 0)}
    for case in cases:
        gen_case(case, out)
    path = os.path.join(HERE, 'statistics.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
