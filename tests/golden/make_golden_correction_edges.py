"""Dev container only (needs the reference checkout): tests/golden/correction_edges.npz — the reference's OWN detect_break_points and
break_and_update_ctgs (through correct_assembly, both spied per round) and parse_pairs_for_correction on every case of
tests/correction_edge_cases.py.  `portion` is not installed here: the interval stand-in of make_golden_correction.py is used.

Per case: every detection (one more than the breaking rounds) and the table after every break (lengths, coverage and position lists of
the children, in the order of ctg_cov_dict), the hash of the case's inputs and — except for the grid-lap case, which the module
generates — the inputs themselves.

    python tests/golden/make_golden_correction_edges.py [reference scripts dir]
"""
import importlib.util
import json
import os
import sys
import tempfile
import types
from array import array
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import correction_edge_cases as cc  # noqa: E402
from tests.test_correction_cpu import REF  # noqa: E402

_spec = importlib.util.spec_from_file_location('make_golden_correction', os.path.join(HERE, 'make_golden_correction.py'))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)
Iv, load_reference = _gen.Iv, _gen.load_reference                 # the interval stand-in for `portion` and the import that binds it

STORED_INPUTS_MAX_BINS = 2000                                     # larger cases keep their inputs in the module


def child_names(parent, unbroken, points, length):
    """:1122-1165: the children of `parent` (length bp) cut at `points`"""
    raw, shift = parent, 0
    if not unbroken:
        raw, pos_range = parent.rsplit(':', 1)
        shift = int(pos_range.split('-')[0]) - 1
    bounds = [0] + list(points) + [length]
    return ['%s:%d-%d' % (raw, a + 1 + shift, b + shift) for a, b in zip(bounds[:-1], bounds[1:])]


def reference_rounds(H, case):
    """correct_assembly(cov_dict, pos_dict, fa_dict, {}, args) on the case's tables, from a temporary directory and a generated FASTA ->
    [{'bp_seg', 'bp_n', 'bp_pos', 'bp_cov', 'state': {'lens', 'nb', 'cov', 'np', 'pos'} or None}, ...] as lists of int"""
    names = ['c%d' % k for k in range(len(case['lens']))]
    res = case['res']
    args = types.SimpleNamespace(correct_resolution=res, correct_nrounds=case['rounds'] + 1, median_cov_ratio=case['ratios'][0],
                                 region_len_ratio=case['ratios'][1], min_region_cutoff=case['ratios'][2], RE='GATC', quick_view=False, gfa=None,
                                 fasta='asm.fa')
    rounds = []
    real_detect, real_break = H.detect_break_points, H.break_and_update_ctgs
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with open('asm.fa', 'w') as f:
                for n, l in zip(names, case['lens']):
                    f.write('>%s\n%s\n' % (n, 'ACGT' * (l // 4) + 'ACGT'[:l % 4]))
            fa_dict = H.parse_fasta('asm.fa', RE='GATC')
            assert [v[1] for v in fa_dict.values()] == case['lens']
            cov_d = {n: np.array(c, np.int32) for n, c in zip(names, case['cov'])}
            pos_d = defaultdict(lambda: array('i'))
            for n, p in zip(names, case['pos']):
                if p:
                    pos_d[n] = array('i', p)

            def spy(cd, fd, a):
                got = real_detect(cd, fd, a)
                order = list(cd)
                assert [order.index(c) for c in got] == sorted(order.index(c) for c in got)
                rounds.append({'bp_seg': [order.index(c) for c in got], 'bp_n': [len(v) for v in got.values()],
                               'bp_pos': [int(p) for v in got.values() for p, _c in v], 'bp_cov': [int(c) for v in got.values() for _p, c in v],
                               'state': None})
                return got

            def spy_break(bp, link_pos, cov, *rest, **kw):
                last = rest[7] if len(rest) > 7 else kw.get('last_round', False)
                fd, unbroken = rest[3], rest[5]
                want = [n for c, v in bp.items() for n in child_names(c, c in unbroken, [p for p, _c in v], fd[c][1])]
                real_break(bp, link_pos, cov, *rest, **kw)
                if last:
                    return
                assert list(cov) == want, (list(cov)[:4], want[:4])
                pos = [list(link_pos[c]) if c in link_pos else [] for c in cov]
                rounds[-1]['state'] = {'lens': [fd[c][1] for c in cov], 'nb': [len(v) for v in cov.values()],
                                       'cov': [int(x) for v in cov.values() for x in v.tolist()], 'np': [len(p) // 2 for p in pos],
                                       'pos': [x for p in pos for x in p]}
            H.detect_break_points, H.break_and_update_ctgs = spy, spy_break
            try:
                H.correct_assembly(cov_d, pos_d, fa_dict, {}, args)
            finally:
                H.detect_break_points, H.break_and_update_ctgs = real_detect, real_break
        finally:
            os.chdir(cwd)
    return rounds


def reference_pass_one(H, case):
    """parse_pairs_for_correction on the records written as a .pairs file -> {'nb', 'cov', 'np', 'pos'} per contig of the FASTA, in its order"""
    names = ['c%d' % k for k in range(len(case['lens']))]
    other = {-1: 'elsewhere', -2: 'filtered'}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with open('hic.pairs', 'w') as f:
                f.write('## pairs format v1.0\n')
                for k, (a, p, b, q) in enumerate(zip(case['id1'].tolist(), case['pos1'].tolist(), case['id2'].tolist(), case['pos2'].tolist())):
                    f.write('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, other.get(a) or names[a], p + 1, other.get(b) or names[b], q + 1))
            fa_dict = {n: ['', int(l), 1] for n, l in zip(names, case['lens'])}
            args = types.SimpleNamespace(alignments='hic.pairs', aln_format='pairs', correct_resolution=case['res'])
            cov_d, pos_d = H.parse_pairs_for_correction(fa_dict, args)
        finally:
            os.chdir(cwd)
    assert list(cov_d) == names
    pos = [list(pos_d[n]) if n in pos_d else [] for n in names]
    return {'nb': [len(cov_d[n]) for n in names], 'cov': [int(x) for n in names for x in cov_d[n].tolist()], 'np': [len(p) // 2 for p in pos],
            'pos': [x for p in pos for x in p]}


def stored_inputs(case):
    if sum(len(c) for c in case['cov']) > STORED_INPUTS_MAX_BINS:
        return None
    return {'lens': case['lens'], 'nb': [len(c) for c in case['cov']], 'cov': [int(x) for c in case['cov'] for x in c.tolist()],
            'np': [len(p) // 2 for p in case['pos']], 'pos': [x for p in case['pos'] for x in p]}


def build(H):
    pk = cc.Packer()

    def freeze(node):
        if isinstance(node, dict):
            return {k: (v if k == 'hash' else freeze(v)) for k, v in node.items()}
        if isinstance(node, list) and (not node or isinstance(node[0], (int, np.integer))):
            return pk.add(node)
        if isinstance(node, list):
            return [freeze(v) for v in node]
        return node
    meta = {'cases': {}, 'pass_one': {}}
    for case in cc.cases():
        rounds = reference_rounds(H, case)
        meta['cases'][case['name']] = freeze({'hash': cc.case_hash(case), 'inputs': stored_inputs(case), 'rounds': rounds})
    for case in cc.pass_one_cases():
        meta['pass_one'][case['name']] = freeze(dict(reference_pass_one(H, case), hash=cc.case_hash(case)))
    ints, ptr = pk.arrays()
    return {'ints': ints, 'ptr': ptr, 'meta': np.array(json.dumps(meta))}


def main():
    H = load_reference(sys.argv[1] if len(sys.argv) > 1 else REF)
    out = build(H)
    path = os.path.join(HERE, 'correction_edges.npz')
    np.savez_compressed(path, **out)
    fx = cc.load_fixture(path)
    print(path, os.path.getsize(path), 'bytes;', len(fx['cases']), 'cases,', len(fx['pass_one']), 'pass-one cases,', len(out['ints']), 'integers')


if __name__ == '__main__':
    main()
