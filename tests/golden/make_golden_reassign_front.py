"""Writes tests/golden/reassign_front.npz from the reference's own parse_fasta (scripts/HapHiC_cluster.py:87-113).

    python tests/golden/make_golden_reassign_front.py [path/to/HapHiC/scripts]

For every FASTA case of tests/reassign_front_cases.py, both keep_letter_case values and every RE string of RES the fixture keeps the reference's
fa_dict as names, lengths and RE sites + 1, and the sequences of the small cases — or the name of the exception the reference raised.  Data only;
layout: reassign_front_cases.golden()."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

from tests import reassign_front_cases as fc      # noqa: E402
from make_golden_build import load_reference_build      # noqa: E402


def main():
    scripts = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/scripts'
    parse_fasta = load_reference_build(scripts).parse_fasta
    cases, raises, has_seq, names, name_off, ints, int_off, blobs = [], [], [], [], [0], [], [0], []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'asm.fa')
        for case, text, _refused in fc.fasta_cases():
            with open(path, 'wb') as f:
                f.write(text)
            cases.append(case)
            try:
                got = {(keep, RE): parse_fasta(path, RE=RE, keep_letter_case=keep) for keep in (False, True) for RE in fc.RES}
            except Exception as e:      # noqa: BLE001 — whatever the reference raises is the record
                raises.append(type(e).__name__)
                has_seq.append(False)
                continue
            raises.append('')
            small = sum(v[1] for v in got[(False, fc.RES[0])].values()) <= fc.SMALL
            has_seq.append(small)
            for keep in (False, True):
                first = got[(keep, fc.RES[0])]
                for RE in fc.RES:
                    d = got[(keep, RE)]
                    assert list(d) == list(first) and [v[:2] for v in d.values()] == [v[:2] for v in first.values()]
                names += list(first)
                name_off.append(len(names))
                ints += [v[1] for v in first.values()]
                for RE in fc.RES:
                    ints += [v[2] for v in got[(keep, RE)].values()]
                int_off.append(len(ints))
                if small:
                    blobs.append(''.join(v[0] for v in first.values()).encode('ascii'))
    out = {'cases': np.array(cases), 'raises': np.array(raises), 'has_seq': np.array(has_seq, np.bool_), 'names': np.array(names, dtype=str),
           'name_off': np.array(name_off, np.int64), 'ints': np.array(ints, np.int64), 'int_off': np.array(int_off, np.int64),
           'blob': np.frombuffer(b''.join(blobs), np.uint8), 'blob_off': np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)}
    path = os.path.join(ROOT, 'tests', 'golden', 'reassign_front.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases,', sum(1 for r in raises if r), 'raise')


if __name__ == '__main__':
    main()
