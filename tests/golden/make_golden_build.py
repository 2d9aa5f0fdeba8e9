"""Writes tests/golden/build.npz from the reference's own `haphic build` (scripts/HapHiC_build.py, parse_fasta of scripts/HapHiC_cluster.py:87-113).

    python tests/golden/make_golden_build.py [path/to/HapHiC/scripts]

For every case of tests/build_cases.py the fixture keeps the inputs (FASTA bytes, tour file names and bytes, corrected_ctgs lines, arguments), the
reference's fa_dict for both keep_letter_case values (names, lengths, RE sites + 1, one sequence blob) and the bytes of scaffolds.fa, scaffolds.agp
and scaffolds.raw.agp that its run() wrote — or the name of the exception it raised.  Data only; layout: build_cases.golden()."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import build_cases as bc      # noqa: E402


def load_reference_build(scripts, name='_haphic_build_reference_private'):
    """HapHiC_build.py under a private module name (a cached `HapHiC_build` may carry the product's seams); pysam / portion stubbed when absent"""
    for mod, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        try:
            __import__(mod)
        except ImportError:
            m = types.ModuleType(mod)
            m.__dict__.update(attrs)
            sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, 'HapHiC_build.py'))
    module = importlib.util.module_from_spec(spec)
    sys.path.insert(0, scripts)
    try:
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(scripts)
    return module


def run_reference(B, case):
    """-> ({keep_letter_case: fa_dict or None}, {file: bytes} or the name of the exception run() raised)"""
    with tempfile.TemporaryDirectory() as tmp:
        args = case.write(tmp)
        fa = {}
        for keep in (False, True):
            try:
                fa[keep] = B.parse_fasta(args.fasta, keep_letter_case=keep)
            except Exception:
                fa[keep] = None
        work = os.path.join(tmp, 'run')
        os.mkdir(work)
        try:
            bc.run_in(work, lambda: B.run(args))
        except Exception as e:
            return fa, type(e).__name__
        return fa, bc.read_outputs(work)


def main():
    scripts = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/scripts'
    B = load_reference_build(scripts)
    cases = bc.cases()
    blobs, in_blobs, ctg_names, ctg_name_off, ints, int_off = [], [], [], [0], [], [0]
    raises, fa_ok, tour_names, tour_off, corrected, numbers = [], [], [], [0], [], []
    for c in cases:
        fa, result = run_reference(B, c)
        in_blobs += [c.fasta] + [data for _f, data in c.tours]
        tour_names += [f for f, _data in c.tours]
        tour_off.append(len(tour_names))
        corrected.append(bc.NO_CORRECTED if c.corrected is None else '\n'.join(c.corrected))
        numbers.append([c.Ns, c.max_width, int(c.sort_by_input), int(c.keep_letter_case)])
        fa_ok.append(fa[False] is not None)
        for keep in (False, True):
            if fa[False] is None:
                continue
            d = fa[keep]
            ctg_names += list(d)
            ctg_name_off.append(len(ctg_names))
            ints += [v[1] for v in d.values()] + [v[2] for v in d.values()]
            int_off.append(len(ints))
            blobs.append(''.join(v[0] for v in d.values()).encode('ascii'))
        raises.append(result if isinstance(result, str) else '')
        if not isinstance(result, str):
            blobs += [result[f] for f in bc.OUTPUTS]
    out = {'case_names': np.array([c.name for c in cases]), 'raises': np.array(raises), 'fa_ok': np.array(fa_ok, np.bool_),
           'blob': np.frombuffer(b''.join(blobs), np.uint8), 'blob_off': np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64),
           'ctg_names': np.array(ctg_names, dtype=str), 'ctg_name_off': np.array(ctg_name_off, np.int64),
           'ints': np.array(ints, np.int64), 'int_off': np.array(int_off, np.int64),
           'in_blob': np.frombuffer(b''.join(in_blobs), np.uint8), 'in_off': np.cumsum([0] + [len(b) for b in in_blobs]).astype(np.int64),
           'tour_names': np.array(tour_names, dtype=str), 'tour_off': np.array(tour_off, np.int64), 'corrected': np.array(corrected, dtype=str),
           'args': np.array(numbers, np.int64)}
    path = os.path.join(ROOT, 'tests', 'golden', 'build.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases,', sum(1 for r in raises if r), 'raise')


if __name__ == '__main__':
    main()
