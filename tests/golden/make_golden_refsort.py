"""Writes tests/golden/refsort.npz from the reference's own `haphic refsort` (scripts/HapHiC_refsort.py).

    python tests/golden/make_golden_refsort.py [path/to/HapHiC/scripts]

For every case of tests/refsort_cases.py the fixture keeps the inputs (AGP, PAF and FASTA texts) and what the reference's functions gave when called
as run() :398-409 calls them: the parse_paf dict (as nested lists in insertion order), stdout, the INFO lines of order_and_orient_groups, the text of
scaffolds.refsort.fa — or the name of the exception raised.  One run() per case is checked against those pieces.  Data only, as two JSON texts;
layout: refsort_cases.golden()."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import build_cases as bc      # noqa: E402
from tests import refsort_cases as rc    # noqa: E402


def load_reference_refsort(scripts, name='_haphic_refsort_reference_private'):
    """HapHiC_refsort.py under a private module name (a cached `HapHiC_refsort` may carry the product's seams); pysam stubbed when absent, and
    where `portion` is absent (or stubbed empty by another loader) the module's `closed` is the package's interval stand-in"""
    for mod, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        try:
            __import__(mod)
        except ImportError:
            m = types.ModuleType(mod)
            m.__dict__.update(attrs)
            sys.modules[mod] = m
        if getattr(sys.modules[mod], '__file__', None) is None:      # a stand-in another loader left: it may lack a name the imports ask for
            for k, v in attrs.items():
                sys.modules[mod].__dict__.setdefault(k, v)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, 'HapHiC_refsort.py'))
    module = importlib.util.module_from_spec(spec)
    sys.path.insert(0, scripts)
    try:
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(scripts)
    if getattr(sys.modules['portion'], '__file__', None) is None:        # a stand-in of this or another loader, whatever it holds
        from haphic_amd import intervals
        module.closed = intervals.closed
    return module


def run_whole(F, case):
    """run() itself -> (stdout, scaffolds.refsort.fa or None) or the name of the exception"""
    with tempfile.TemporaryDirectory() as tmp:
        args = case.write(tmp)
        work = os.path.join(tmp, 'run')
        os.mkdir(work)
        stdout = io.StringIO()
        try:
            with contextlib.redirect_stdout(stdout):
                bc.run_in(work, lambda: F.run(args))
        except Exception as e:
            return type(e).__name__
        fa = os.path.join(work, args.fout)
        return stdout.getvalue(), open(fa, 'rb').read().decode('ascii') if args.fasta else None


def main():
    scripts = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/scripts'
    F = load_reference_refsort(scripts)
    cases = rc.cases()
    records, inputs = {}, {}
    for c in cases:
        with tempfile.TemporaryDirectory() as tmp:
            rec = rc.run_reference(F, c, tmp)
        whole = run_whole(F, c)
        assert whole == (rec['raises'] if rec['raises'] else (rec['stdout'], rec['fa'])), c.name
        records[c.name] = rec
        inputs[c.name] = [c.agp.decode('ascii'), c.paf.decode('ascii'), None if c.fasta is None else c.fasta.decode('ascii')]
        print(c.name, rec['raises'] or '{} log lines, {} bytes of stdout, {} of FASTA'.format(len(rec['log']), len(rec['stdout']), len(rec['fa'] or '')))
    path = os.path.join(ROOT, 'tests', 'golden', 'refsort.npz')
    np.savez_compressed(path, records=np.frombuffer(json.dumps(records).encode('ascii'), np.uint8),
                        inputs=np.frombuffer(json.dumps(inputs).encode('ascii'), np.uint8))
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases,', sum(1 for r in records.values() if r['raises']), 'raise')


if __name__ == '__main__':
    main()
