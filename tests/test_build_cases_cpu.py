"""`haphic build` without a GPU: the mirrors of haphic_amd/scaffolds.py over the numpy engine of tests/build_cases.py give the reference's bytes
(tests/golden/build.npz: scaffolds.fa, scaffolds.agp, scaffolds.raw.agp and fa_dict of the reference's own run on every case), the FastaTable
semantics, the refusals, the command line, and — where the reference checkout is present — HapHiC_build.run() with and without patch_build."""
import os
import types

import numpy as np
import pytest

from haphic_amd import containers, scaffolds
from tests import build_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/scripts'
Z = np.load(os.path.join(HERE, 'golden', 'build.npz'))
GOLDEN = bc.golden(Z)
CASES = bc.cases()
SERVED = [c for c in CASES if not c.refused]


def test_the_generator_still_gives_the_recorded_inputs():
    recorded = bc.golden_inputs(Z)
    assert [c.name for c in recorded] == [c.name for c in CASES]
    for a, b in zip(recorded, CASES):
        assert (a.fasta, a.tours, a.corrected, a.Ns, a.max_width, a.sort_by_input, a.keep_letter_case) == \
               (b.fasta, b.tours, b.corrected, b.Ns, b.max_width, b.sort_by_input, b.keep_letter_case), a.name
    assert os.path.getsize(os.path.join(HERE, 'golden', 'build.npz')) < 1 << 20


def test_the_cases_reach_what_they_are_meant_to():
    """slab seams of the smallest slab inside a header, on a '\\n', inside a gap and inside a piece; pieces and gaps at every offset of a 16-byte store"""
    fa = GOLDEN['emit/offsets_one_line']['files']['scaffolds.fa']
    first = fa.split(b'\n')[1]                                # 20 reversed pieces of 17 joined by 100 N
    assert len(first) == 20 * 17 + 19 * 100
    start = fa.index(first)
    assert {(start + k * 117) % 16 for k in range(20)} == set(range(16)) and {(start + 17 + k * 117) % 16 for k in range(19)} == set(range(16))
    kinds = set()
    for name in ('emit/offsets_one_line', 'emit/offsets_w60', 'emit/offsets_w7_ns1'):
        fa = GOLDEN[name]['files']['scaffolds.fa']
        for seam in range(bc.SLAB_MIN, len(fa), bc.SLAB_MIN):
            line_start = fa.rfind(b'\n', 0, seam) + 1
            if fa[line_start:line_start + 1] == b'>' and seam > line_start:
                kinds.add('header')
            elif fa[seam - 1:seam] == b'\n' or fa[seam:seam + 1] == b'\n':
                kinds.add('newline')
            elif fa[seam - 1:seam + 1] == b'NN':
                kinds.add('gap')
            else:
                kinds.add('piece')
    assert kinds == {'header', 'newline', 'gap', 'piece'}


@pytest.mark.parametrize('case', SERVED, ids=repr)
def test_numpy_engine_gives_the_reference_fa_dict(case):
    for keep in (False, True):
        names, lengths, re_sites, seq = GOLDEN[case.name]['fa_dict'][keep]
        table = scaffolds.parse_fasta(case.fasta, keep_letter_case=keep, _engine=bc.NumpyFasta)
        assert isinstance(table, containers.FastaTable) and table.frozen
        assert table.names == names and table.lengths.tolist() == lengths.tolist() and table.engine.sequences().tobytes() == seq
        off = np.concatenate([[0], np.cumsum(lengths)]).tolist()
        want = {n: [seq[off[k]:off[k + 1]].decode(), int(lengths[k]), int(re_sites[k])] for k, n in enumerate(names)}
        assert list(table) == names and table.frozen
        got = dict(table.items())                              # thaws
        assert not table.frozen and got == want and list(got) == names


@pytest.mark.parametrize('case', SERVED, ids=repr)
def test_numpy_engine_gives_the_reference_files(case, tmp_path):
    files, table = bc.run_mirrors(case, str(tmp_path), bc.NumpyFasta, scaffolds.parse_fasta, scaffolds.build_final_scaffolds)
    assert table.frozen, 'build_final_scaffolds thawed the table'
    for f in bc.OUTPUTS:
        assert files[f] == GOLDEN[case.name]['files'][f], f


def test_fasta_table_semantics():
    table = scaffolds.parse_fasta(b'>a x\nacgatc\nGATC\n>b\n\n>c\nNNgatcN\n', _engine=bc.NumpyFasta)
    before = len(containers.THAW_LOG)
    assert len(table) == 3 and bool(table) and 'a' in table and 'b' in table and 'zz' not in table and list(table) == ['a', 'b', 'c']
    assert table.index_of('c') == 2 and table.index_of('nope') == -1 and table.lengths.tolist() == [10, 0, 7]
    assert table.frozen and len(containers.THAW_LOG) == before
    assert table['a'] == ['ACGATCGATC', 10, 3]                 # thaws: two GATC + the pseudo-count
    assert not table.frozen and type(table) is containers.ThawedFasta and isinstance(table, dict)
    assert dict(table) == {'a': ['ACGATCGATC', 10, 3], 'b': ['', 0, 1], 'c': ['NNGATCN', 7, 2]}
    assert len(containers.THAW_LOG) == before + 1
    table['d'] = ['A', 1, 1]
    del table['a']
    assert list(table) == ['b', 'c', 'd'] and not table.frozen
    for touch in (lambda t: t.values(), lambda t: t.get('a'), lambda t: t.pop('b'), lambda t: t.__setitem__('q', [])):
        t = scaffolds.parse_fasta(b'>a\nAC\n>b\nGT\n', _engine=bc.NumpyFasta)
        touch(t)
        assert not t.frozen


# ------------------------------------------------------------------ what is not served goes to the reference's own function
def _args(**kw):
    base = dict(Ns=100, max_width=60, sort_by_input=False, keep_letter_case=False, prefix='scaffolds')
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize('name', ['refuse/high_byte', 'refuse/sequence_first', 'refuse/duplicate_names'])
def test_a_refused_fasta_goes_to_the_original_parse_fasta(name, tmp_path):
    case = next(c for c in CASES if c.name == name)
    path = str(tmp_path / 'asm.fa')
    with open(path, 'wb') as f:
        f.write(case.fasta)
    calls = []

    def original(fasta, RE, keep_letter_case, logger):
        calls.append((fasta, RE, keep_letter_case))
        return 'theirs'
    assert scaffolds.parse_fasta(path, 'AAGCTT', True, _original=original, _engine=bc.NumpyFasta) == 'theirs'
    assert calls == [(path, 'AAGCTT', True)]
    with pytest.raises(bc.NumpyFasta.Unsupported):
        scaffolds.parse_fasta(path, _engine=bc.NumpyFasta)


def test_unserved_builds_go_to_the_original_function(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    table = scaffolds.parse_fasta(b'>a\nACGT\n>b:1-2\nGG\n', _engine=bc.NumpyFasta)
    tour_dict = {'g': [('a', '-')]}

    def original(*a):
        return ('theirs',) + a[4:]
    for args in (_args(max_width=0), _args(max_width=-3), _args(Ns=-1)):
        assert scaffolds.build_final_scaffolds(tour_dict, table, {'a'}, set(), args, _original=original) == ('theirs', args)
        assert table.frozen and os.listdir(str(tmp_path)) == []
    # a corrected contig whose name does not read name:start-end: the assertion / ValueError is the reference's to raise
    for bad in ({'a'}, {'b:1-2', 'a'}):
        assert scaffolds.build_final_scaffolds(tour_dict, table, {'a'}, bad, _args(), _original=original)[0] == 'theirs'
    table2 = scaffolds.parse_fasta(b'>a\nACGT\n>b:1-2-3\nGG\n', _engine=bc.NumpyFasta)
    assert scaffolds.build_final_scaffolds(tour_dict, table2, {'a'}, {'b:1-2-3'}, _args(), _original=original)[0] == 'theirs'
    assert os.listdir(str(tmp_path)) == []
    plain = dict(table.items())                                   # a thawed table, and a plain dict
    assert scaffolds.build_final_scaffolds(tour_dict, table, {'a'}, set(), _args(), _original=original)[0] == 'theirs'
    assert scaffolds.build_final_scaffolds(tour_dict, plain, {'a'}, set(), _args(), _original=original)[0] == 'theirs'
    assert os.listdir(str(tmp_path)) == []


def test_patch_build_binds_and_returns_the_originals():
    from haphic_amd import patch
    import logging
    B = types.SimpleNamespace(parse_fasta=lambda *a, **k: 'pf', build_final_scaffolds=lambda *a: 'bfs', logger=logging.getLogger('t'))
    originals = (B.parse_fasta, B.build_final_scaffolds)
    saved = patch.patch_build(B, engine=bc.NumpyFasta)
    assert set(saved) == set(patch.BUILD_SEAMS) == {'parse_fasta', 'build_final_scaffolds'}
    assert (saved['parse_fasta'], saved['build_final_scaffolds']) == originals
    assert B.parse_fasta.__wrapped__ is scaffolds.parse_fasta and B.build_final_scaffolds.__wrapped__ is scaffolds.build_final_scaffolds
    assert B.build_final_scaffolds({}, {}, set(), set(), _args()) == 'bfs'          # a plain dict: the original's


# ------------------------------------------------------------------ the reference's run() around the mirrors
def _load_reference():
    from tests.golden.make_golden_build import load_reference_build
    return load_reference_build(REF, '_haphic_build_reference_for_test')


def _run(B, case, directory):
    os.makedirs(directory)
    args = case.write(directory)
    work = os.path.join(directory, 'run')
    os.mkdir(work)
    try:
        bc.run_in(work, lambda: B.run(args))
    except Exception as e:
        return type(e).__name__
    return bc.read_outputs(work)


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_reference_run_with_and_without_the_seams(tmp_path):
    from haphic_amd import patch
    B = _load_reference()
    theirs = {c.name: _run(B, c, str(tmp_path / 'theirs' / str(k))) for k, c in enumerate(CASES)}
    saved = patch.patch_build(B, engine=bc.NumpyFasta)
    try:
        ours = {c.name: _run(B, c, str(tmp_path / 'ours' / str(k))) for k, c in enumerate(CASES)}
    finally:
        for name, fn in saved.items():
            setattr(B, name, fn)
    for c in CASES:
        assert ours[c.name] == theirs[c.name], c.name
        if not c.refused:
            assert theirs[c.name] == GOLDEN[c.name]['files'], c.name
    assert theirs['refuse/sequence_first'] == 'UnboundLocalError' and theirs['refuse/max_width_0'] == 'ValueError'


# ------------------------------------------------------------------ the command line
def run_main(argv):
    from haphic_amd import __main__ as cli
    with pytest.raises(SystemExit) as e:
        cli.main(list(argv))
    return str(e.value)


def test_build_is_a_command_now(monkeypatch):
    monkeypatch.delenv('HAPHIC_REFERENCE', raising=False)
    assert 'HapHiC checkout not found' in run_main(['build', '--reference', '/nonexistent'])
    assert '--gpus is a flag of the "cluster" step only' in run_main(['build', '--gpus', '2'])
    msg = run_main(['pipeline'])
    assert 'steps only' in msg and all('"%s"' % s in msg for s in ('cluster', 'plot', 'reassign', 'sort', 'build'))
    from haphic_amd import __main__ as cli
    assert 'python -m haphic_amd build' in cli.__doc__ and '--keep-reference-build' in cli.__doc__
