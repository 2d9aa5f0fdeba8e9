"""`haphic cluster --gpus N --correct_nrounds 2` on the one GPU of a test box: N ranks over the host transport share BOTH passes over the
alignment file, and every file of the job — the corrected FASTA, alignments.bed, the link files, every inflation_*/ file — is byte-identical
to the one-rank run of the same seam sequence (tests/ranks_correction_job.py: the sequence run() drives, the reference checkout is not needed).
The per-rank record (HAPHIC_RANKS_RECORD) shows who parsed what: every rank a share of the lines, in pass one and in pass two."""
import filecmp
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB = os.path.join(ROOT, 'tests', 'ranks_correction_job.py')
STEP_S = 150                     # each rank's process: timeout -k 10 STEP_S

pytestmark = pytest.mark.gpu


def _bgzip(data, block=4000):
    from tests.bam_fixture import bgzf_block
    return b''.join(bgzf_block(data[k:k + block]) for k in range(0, len(data), block)) + bgzf_block(b'')


def _inputs(tmp_path, fmt, text=None):
    """asm.fa and the alignment file (the fixture's own, or `text`) under tmp_path; returns (fasta, pairs, number of lines)"""
    from tests import correction_fixture
    correction_fixture.write_inputs(correction_fixture.load(), str(tmp_path))
    plain = str(tmp_path / 'hic.pairs')
    if text is not None:
        with open(plain, 'wb') as f:
            f.write(text)
    with open(plain, 'rb') as f:
        data = f.read()
    pairs = plain
    if fmt != 'pairs':
        pairs = plain + '.gz'
        with open(pairs, 'wb') as f:
            f.write(_bgzip(data))
    return str(tmp_path / 'asm.fa'), pairs, len(data.splitlines())


def _run(case, fasta, pairs, fmt, tmp_path, world):
    """one job of `world` ranks (fresh child processes, each under its own time limit); returns (work directory, per-rank records)"""
    from haphic_amd import ranks
    workdir, recdir = str(tmp_path / ('w%d' % world)), str(tmp_path / ('rec%d' % world))
    os.makedirs(workdir)
    os.makedirs(recdir)
    cmd = ['timeout', '-k', '10', str(STEP_S), sys.executable, JOB, case, fasta, pairs, fmt, workdir]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), HAPHIC_TABLE_PIECE='5000', HAPHIC_RANKS_RECORD=recdir)
    env.pop('MASTER_PORT', None)
    rc = ranks.launch(cmd, world, host_transport=True, env=env)
    assert rc == 0, 'world {} job failed with status {}'.format(world, rc)
    records = []
    for r in range(world):
        with open(os.path.join(recdir, 'rank%d.json' % r)) as f:
            records.append(json.load(f))
    return workdir, records


def _files(d):
    out = []
    for base, _dirs, names in os.walk(d):
        out += [os.path.relpath(os.path.join(base, n), d) for n in names]
    return sorted(out)


def _same_tree(a, b):
    fa, fb = _files(a), _files(b)
    assert fa == fb
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f + ' differs'


def _lines_of(records, phase):
    """per rank: the lines it parsed in `phase` (0 when it took no part)"""
    out = []
    for rec in records:
        rows = [p for p in rec['phases'] if p['phase'] == phase]
        assert len(rows) <= 1, (phase, rec)
        out.append(rows[0]['lines'] if rows else 0)
    return out


def _check_shares(records, n_lines, every_rank):
    for phase in ('correct_pass1', 'ingest'):
        lines = _lines_of(records, phase)
        print(phase, 'lines per rank', lines, 'of', n_lines)
        assert sum(lines) == n_lines, (phase, lines, n_lines)
        if every_rank:
            assert all(k > 0 for k in lines[1:]), (phase, lines)
    for rec in records[1:]:
        sent = [p for p in rec['phases'] if p['phase'] == 'correct_pass1']
        assert sent and sent[0]['bytes_sent'] > 0                    # at least its difference array went to rank 0


def _broken(workdir):
    with open(os.path.join(workdir, 'broken.txt')) as f:
        return int(f.read())


@pytest.mark.parametrize('fmt', ['pairs', 'bgzipped_pairs'])
@pytest.mark.parametrize('case', ['ctg', 'bins'])
def test_n_ranks_with_correction_write_the_files_of_one(tmp_path, case, fmt):
    fasta, pairs, n_lines = _inputs(tmp_path, fmt)
    one, _rec = _run(case, fasta, pairs, fmt, tmp_path, 1)
    assert _broken(one) > 0, 'the fixture has planted chimeras'
    names = _files(one)
    assert {'corrected_asm.fa', 'corrected_ctgs.txt', 'alignments.bed', 'HT_links.pkl', 'full_links.pkl', 'paired_links.clm'} <= set(names)
    assert any(n.startswith('inflation_') for n in names)
    assert os.path.getsize(os.path.join(one, 'alignments.bed')) > 0 and os.path.getsize(os.path.join(one, 'corrected_ctgs.txt')) > 0
    for world in (2, 3):
        d, records = _run(case, fasta, pairs, fmt, tmp_path, world)
        _same_tree(one, d)
        _check_shares(records, n_lines, every_rank=True)


def test_nothing_to_break_takes_the_ordinary_generators(tmp_path):
    fasta, pairs, n_lines = _inputs(tmp_path, 'pairs')
    one, _rec = _run('nobreak', fasta, pairs, 'pairs', tmp_path, 1)
    assert _broken(one) == 0 and os.path.getsize(os.path.join(one, 'corrected_ctgs.txt')) == 0
    d, records = _run('nobreak', fasta, pairs, 'pairs', tmp_path, 2)
    _same_tree(one, d)
    _check_shares(records, n_lines, every_rank=True)


def test_more_ranks_than_lines(tmp_path):
    from tests import correction_fixture
    nm = correction_fixture.load()['names']
    text = ('r0\t%s\t101\t%s\t2001\t+\t-\nr1\t%s\t3001\t%s\t9001\t+\t-\nr2\t%s\t501\t%s\t701\t+\t-\n' % (nm[0], nm[1], nm[2], nm[2], nm[1], nm[3])).encode()
    fasta, pairs, n_lines = _inputs(tmp_path, 'pairs', text)
    assert n_lines == 3
    one, _rec = _run('tiny', fasta, pairs, 'pairs', tmp_path, 1)
    d, records = _run('tiny', fasta, pairs, 'pairs', tmp_path, 5)
    _same_tree(one, d)
    _check_shares(records, n_lines, every_rank=False)
    assert sum(1 for k in _lines_of(records, 'correct_pass1') if k == 0) >= 2          # ranks that own an empty range
