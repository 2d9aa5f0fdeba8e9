#!/usr/bin/env python3
"""tests/golden/link_pickles.npz: the bytes of full_links.pkl and HT_links.pkl as the reference's own code writes them for one tiny input —
a .pairs text of a few hundred read pairs over 14 contigs read by pairs_generator_inter_ctgs :1562-1583, parse_alignments_for_ctgs :1596-1655,
output_pickle :710-715 (run() :2872-2931).  Data only.  It pins the reference's dialect: FRAME, MEMOIZE after every key, the keys' names written
as literals again (they are the str objects of the line that made the key) and BINGET only where two keys share one object.

    python tests/golden/make_golden_link_pickles.py            (needs the reference checkout)"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules.setdefault(name, m)
sys.path.insert(0, os.environ.get('HAPHIC_REFERENCE_SCRIPTS', '/root/reference/scripts'))
import HapHiC_cluster as H  # noqa: E402

H.logger.setLevel('WARNING')


def main():
    rng = np.random.default_rng(11)
    names = ['utg%06dl' % (k * 37 + 1) for k in range(14)]
    length = rng.integers(40_000, 400_000, len(names))
    fa_dict = {n: [None, int(l), int(l) // 400] for n, l in zip(names, length)}
    lines = ['## pairs format v1.0\n']
    for k in range(420):
        a, b = rng.integers(0, len(names), 2)
        lines.append('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, names[a], rng.integers(1, length[a]), names[b], rng.integers(1, length[b])))
    args = types.SimpleNamespace(flank=20, remove_allelic_links=0, remove_concentrated_links=False, max_read_pairs=200, nwindows=50)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with open('hic.pairs', 'w') as f:
                f.writelines(lines)
            aln = H.pairs_generator_inter_ctgs('hic.pairs', 'pairs')
            full, _flank, HT, _clm, _frag_link, _coord = H.parse_alignments_for_ctgs(aln, fa_dict, args, {n: fa_dict[n][1] for n in names}, set(names),
                                                                                     'int32', 'int32')
            H.output_pickle(HT, 'HT_link_dict', 'HT_links.pkl')
            H.output_pickle(full, 'full_link_dict', 'full_links.pkl')
            out = {n: np.frombuffer(open(n + '.pkl', 'rb').read(), np.uint8) for n in ('full_links', 'HT_links')}
        finally:
            os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, 'link_pickles.npz'), **out)
    print({k: v.size for k, v in out.items()})


if __name__ == '__main__':
    main()
