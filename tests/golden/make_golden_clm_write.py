#!/usr/bin/env python3
"""Writes tests/golden/clm_write.npz from the reference's own update_clm_dict and output_clm (scripts/HapHiC_cluster.py:376-401).

    python tests/golden/make_golden_clm_write.py path/to/HapHiC/scripts     (or HAPHIC_REFERENCE_SCRIPTS; needs the reference checkout)

For every case of tests/clm_write_cases.py the read pairs go through the four statements of parse_alignments_for_ctgs that feed the
CLM file (:1629-1633 and :1643: the two ends sorted by contig name, the 0-based coordinates handed to update_clm_dict) into a
clm_dict of the array type determine_int_type :116-147 chooses for the contig lengths, and output_clm writes paired_links.clm in a
temporary directory.  The fixture keeps the inputs of every case and the file: its bytes, or, above clm_write_cases.GOLDEN_TEXT_MAX,
its SHA-256 and length alone.  Data only."""
import hashlib
import os
import sys
import tempfile
import types
from array import array
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import clm_write_cases as cw      # noqa: E402


def load_reference():
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
    scripts = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('HAPHIC_REFERENCE_SCRIPTS')
    if not scripts or not os.path.exists(os.path.join(scripts, 'HapHiC_cluster.py')):
        sys.exit('usage: make_golden_clm_write.py path/to/HapHiC/scripts   (or HAPHIC_REFERENCE_SCRIPTS)')
    sys.path.insert(0, scripts)
    import HapHiC_cluster as H
    H.logger.setLevel('WARNING')
    return H


def reference_text(H, case):
    fa_dict = {n: [None, int(ln), 0] for n, ln in zip(case.names, case.lengths.tolist())}
    ctg_len_dict = {n: v[1] for n, v in fa_dict.items()}
    _pos_type, dist_type = H.determine_int_type(fa_dict)
    clm_dict = defaultdict(lambda: array('i')) if dist_type == 'int32' else defaultdict(lambda: array('l'))        # :1617-1620
    nm = case.names
    for a, x, b, y in zip(case.id1.tolist(), case.p1.tolist(), case.id2.tolist(), case.p2.tolist()):
        ref, pos, mref, mpos = nm[a], x, nm[b], y
        (ctg_i, coord_i), (ctg_j, coord_j) = sorted(((ref, pos + 1), (mref, mpos + 1)))                              # :1629
        ctg_name_pair = (ctg_i, ctg_j)
        len_i, len_j = ctg_len_dict[ctg_i], ctg_len_dict[ctg_j]
        H.update_clm_dict(clm_dict, ctg_name_pair, len_i, len_j, coord_i - 1, coord_j - 1)                            # :1643
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            H.output_clm(clm_dict)
            return open('paired_links.clm', 'rb').read()
        finally:
            os.chdir(cwd)


def main():
    H = load_reference()
    cases = [cw.case(n) for n in cw.GOLDEN_CASES]
    texts = [reference_text(H, c) for c in cases]
    kept = [len(t) <= cw.GOLDEN_TEXT_MAX for t in texts]
    # few arrays: case k owns names / lengths name_off[k]:name_off[k + 1], read pairs pair_off[k]:pair_off[k + 1], cuts cut_off[k]:cut_off[k + 1]
    # and, where text_kept[k], the next text_len[k] bytes of text
    out = {'case_names': np.array([c.name for c in cases]),
           'names': np.array([n for c in cases for n in c.names], dtype=str), 'lengths': np.concatenate([c.lengths for c in cases]),
           'name_off': np.cumsum([0] + [len(c.names) for c in cases]).astype(np.int64),
           'pairs': np.concatenate([np.stack([c.id1, c.p1, c.id2, c.p2], axis=1).astype(np.int64) for c in cases]),
           'pair_off': np.cumsum([0] + [len(c.id1) for c in cases]).astype(np.int64),
           'cuts': np.array([x for c in cases for x in c.cuts], np.int64), 'cut_off': np.cumsum([0] + [len(c.cuts) for c in cases]).astype(np.int64),
           'text_len': np.array([len(t) for t in texts], np.int64), 'text_sha256': np.array([hashlib.sha256(t).hexdigest() for t in texts]),
           'text_kept': np.array(kept, np.bool_), 'text': np.frombuffer(b''.join(t for t, k in zip(texts, kept) if k), np.uint8)}
    path = os.path.join(HERE, 'clm_write.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases,', sum(kept), 'with their bytes')


if __name__ == '__main__':
    main()
