"""Writes tests/golden/sort_heads.npz from the reference's own get_sub_HT_dict (scripts/HapHiC_sort.py:117-143).

    python tests/golden/make_golden_sort_heads.py [path/to/HapHiC/scripts]

Every case of tests/sort_heads_cases.py: the table (names in order of first appearance, the two name ids and the value of every key in file order)
and, per group extracted from it, the contigs as given, the items of sub_HT_dict in insertion order (i, j, w) and HT_index_dict in insertion order
(index_names, index_values), all of them as the unmodified function returns them on the dict the case's pickle loads into.  Data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import sort_cases as sc              # noqa: E402
from tests import sort_heads_cases as hc        # noqa: E402


def strings(values):
    return np.array(list(values), np.str_) if len(values) else np.empty(0, '<U1')


def main(scripts=sc.REFERENCE_SCRIPTS):
    S = sc.load_reference_sort(scripts, name='_haphic_sort_reference_golden_heads')
    out = {'cases': strings([c.name for c in hc.cases()])}
    for case in hc.cases():
        table = hc.table_of(case)
        i, j, value, names = hc.table_arrays(case.items)
        out[case.name + '/names'], out[case.name + '/ti'], out[case.name + '/tj'], out[case.name + '/tv'] = strings(names), i, j, value
        out[case.name + '/n_groups'] = np.int64(len(case.groups))
        for g, ctgs in enumerate(case.groups):
            sub, index = S.get_sub_HT_dict(list(ctgs), table)
            keys = np.array(list(sub.keys()), np.int32).reshape(-1, 2)
            values = list(sub.values())
            p = '{}/{}/'.format(case.name, g)
            out[p + 'ctgs'] = strings(ctgs)
            out[p + 'i'], out[p + 'j'] = keys[:, 0], keys[:, 1]
            out[p + 'w'] = np.array(values, np.float64 if case.kind == 'float' else np.int64).reshape(len(values))
            out[p + 'index_names'], out[p + 'index_values'] = strings(list(index)), np.array(list(index.values()), np.int32).reshape(len(index))
            assert len(table) == len(case.items)                      # the look-ups added nothing (`in` before [])
    np.savez_compressed(hc.GOLDEN, **out)
    size = os.path.getsize(hc.GOLDEN)
    print('{}: {} cases, {} bytes'.format(hc.GOLDEN, len(hc.cases()), size))
    assert size < 1 << 20


if __name__ == '__main__':
    main(*sys.argv[1:2])
