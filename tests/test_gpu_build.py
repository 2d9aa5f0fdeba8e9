"""`haphic build` on the device (csrc/hhx_fasta.hip behind _lib.Fasta): the reader and the writer against the reference's bytes of
tests/golden/build.npz on every case of tests/build_cases.py, with the default and the smallest slab, and against the numpy engine (pinned to the
same fixture by tests/test_build_cases_cpu.py) on a generated genome of about 2 MB."""
import os

import numpy as np
import pytest

from haphic_amd import _lib, containers, scaffolds
from tests import build_cases as bc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = bc.golden(np.load(os.path.join(HERE, 'golden', 'build.npz')))
CASES = bc.cases()
SERVED = [c for c in CASES if not c.refused]


@pytest.fixture(autouse=True)
def default_slab():
    yield
    _lib.tune('fasta_slab', None)


@pytest.fixture(scope='module')
def genome():
    """the case and the bytes the numpy engine writes for it"""
    import tempfile
    case = bc.genome_case()
    with tempfile.TemporaryDirectory() as tmp:
        files, _table = bc.run_mirrors(case, tmp, bc.NumpyFasta, scaffolds.parse_fasta, scaffolds.build_final_scaffolds)
    return case, files


@pytest.mark.parametrize('case', SERVED, ids=repr)
def test_reader_gives_the_reference_fa_dict(case, tmp_path):
    path = str(tmp_path / 'asm.fa')
    with open(path, 'wb') as f:
        f.write(case.fasta)
    for keep in (False, True):
        names, lengths, re_sites, seq = GOLDEN[case.name]['fa_dict'][keep]
        for source in (case.fasta, path):
            fa = _lib.Fasta(source, keep_letter_case=keep)
            assert fa.names() == names and fa.seq_len.tolist() == lengths.tolist() and fa.sequences().tobytes() == seq
            assert fa.seq_off.tolist() == (np.cumsum(lengths) - lengths).tolist()
            fa.close()
        table = scaffolds.parse_fasta(path, keep_letter_case=keep)
        assert table.frozen and list(table) == names
        off = np.concatenate([[0], np.cumsum(lengths)]).tolist()
        assert dict(table.items()) == {n: [seq[off[k]:off[k + 1]].decode(), int(lengths[k]), int(re_sites[k])] for k, n in enumerate(names)}
        assert not table.frozen


@pytest.mark.parametrize('slab', [None, bc.SLAB_MIN], ids=['default_slab', 'min_slab'])
@pytest.mark.parametrize('case', SERVED, ids=repr)
def test_mirrors_write_the_reference_files(case, slab, tmp_path):
    _lib.tune('fasta_slab', slab)
    files, table = bc.run_mirrors(case, str(tmp_path), _lib.Fasta, scaffolds.parse_fasta, scaffolds.build_final_scaffolds)
    assert isinstance(table, containers.FastaTable) and table.frozen
    for f in bc.OUTPUTS:
        assert files[f] == GOLDEN[case.name]['files'][f], f


@pytest.mark.parametrize('slab', [None, bc.SLAB_MIN], ids=['default_slab', 'min_slab'])
def test_generated_genome_equals_the_numpy_engine(genome, slab, tmp_path):
    case, want = genome
    _lib.tune('fasta_slab', slab)
    files, _table = bc.run_mirrors(case, str(tmp_path), _lib.Fasta, scaffolds.parse_fasta, scaffolds.build_final_scaffolds,
                                   source='bytes' if slab is None else 'path')
    assert len(files['scaffolds.fa']) > 2 << 20
    for f in bc.OUTPUTS:
        assert files[f] == want[f], f


def test_reader_on_the_generated_genome(genome):
    case, _want = genome
    theirs = bc.NumpyFasta(case.fasta, keep_letter_case=True)
    ours = _lib.Fasta(case.fasta, keep_letter_case=True)
    assert ours.names() == theirs.names() and ours.seq_len.tolist() == theirs.seq_len.tolist()
    assert ours.sequences().tobytes() == theirs.sequences().tobytes()
    sites = [b'GATC', b'AAGCTT']
    assert ours.re_counts(sites).tolist() == theirs.re_counts(sites).tolist()


def test_refusals_are_unsupported_and_leave_no_file(tmp_path):
    for name in ('refuse/high_byte', 'refuse/sequence_first'):
        case = next(c for c in CASES if c.name == name)
        path = str(tmp_path / 'bad.fa')
        with open(path, 'wb') as f:
            f.write(case.fasta)
        for source in (case.fasta, path):
            with pytest.raises(_lib.Fasta.Unsupported):
                _lib.Fasta(source)
        assert scaffolds.parse_fasta(path, _original=lambda *a: 'theirs') == 'theirs'
    dup = next(c for c in CASES if c.name == 'refuse/duplicate_names')
    assert scaffolds.parse_fasta(dup.fasta, _original=lambda *a: 'theirs') == 'theirs'
    with pytest.raises(_lib.Fasta.Unsupported):
        _lib.Fasta(str(tmp_path))                              # no regular file
    with pytest.raises(RuntimeError):
        _lib.Fasta(str(tmp_path / 'missing.fa'))
    fa = _lib.Fasta(b'>a\nACGT\n>b\nGG\n')
    out = str(tmp_path / 'out.fa')
    for Ns, width in ((100, 0), (100, -1), (-1, 60)):
        with pytest.raises(_lib.Fasta.Unsupported):
            fa.emit(out, ['g'], [0, 2], [0, 1], [1, 0], Ns, width)
        assert not os.path.exists(out)
    with pytest.raises(RuntimeError):                            # a contig the table does not have
        fa.emit(out, ['g'], [0, 1], [2], [0], 100, 60)
    assert not os.path.exists(out)
    assert fa.emit(out, ['g', 'e'], [0, 2, 2], [0, 1], [1, 0], 2, 3) == len(b'>g\nACG\nTNN\nGG\n>e\n')
    assert open(out, 'rb').read() == b'>g\nACG\nTNN\nGG\n>e\n'
    assert fa.emit(out, [], [0], [], [], 2, 3) == 0 and open(out, 'rb').read() == b''
    empty = _lib.Fasta(b'')
    assert empty.n_ctg == 0 and empty.names() == [] and empty.sequences().size == 0


def test_null_handles():
    L = _lib.load()
    n = _lib.C.c_int64(0)
    assert L.hhx_fasta_counts(None, _lib.C.byref(n), None, None) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_fasta_table(None, None, None, None, None) != 0 and L.hhx_fasta_sequences(None, None) != 0
    assert L.hhx_fasta_emit(None, b'x', 0, None, None, None, None, None, 0, 60, None) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_fasta_close(None) == 0


def test_the_knob_is_clamped_and_unknown_knobs_are_refused(tmp_path):
    case = next(c for c in CASES if c.name == 'emit/offsets_w60')
    for k, slab in enumerate((1, 0, -5, 1000, 1 << 40)):               # below the minimum, no multiple of 16, above the maximum
        _lib.tune('fasta_slab', slab)
        files, _table = bc.run_mirrors(case, str(tmp_path / str(k)), _lib.Fasta, scaffolds.parse_fasta, scaffolds.build_final_scaffolds)
        assert files == GOLDEN[case.name]['files'], slab
    _lib.tune('fasta_slab', None)
    with pytest.raises(RuntimeError, match='unknown knob'):
        _lib.tune('fasta_slabs', 1)
