"""The correction phases of a multi-rank job without a GPU (the twin of tests/test_gpu_ranks_correction.py): world sizes 2 and 3 over gloo,
`_lib` the numpy stand-in (tests/ranks_correction_host_job.py).  Pass one — the phase `correct_pass1`, every rank's table absorbed in rank
order — must give the coverage and the position lists tests/golden/correction.npz pins for the reference; pass two — the remap tables
broadcast with the ingest spec, every rank converting its own lines — must give the whole file's converted pairs in file order."""
import json
import os
import sys

import numpy as np
import pytest

from haphic_amd import ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB = os.path.join(ROOT, 'tests', 'ranks_correction_host_job.py')


def _convert(names, cid, fpos, ffrag, i, x):
    """convert_ctg :1405-1411, then `ref not in fa_dict`"""
    if i < 0 or i >= len(names):
        return -1, x
    n = names[i]
    if n in ffrag:
        for p, f in zip(fpos[n], ffrag[n]):                      # descending break positions
            if x - p >= 0:
                return cid[f], x - p
    return cid[n], x


@pytest.mark.parametrize('world', [2, 3])
def test_both_passes_shared_over_gloo(tmp_path, world):
    from tests import correction_fixture
    fx = correction_fixture.load()
    correction_fixture.write_inputs(fx, str(tmp_path))
    pairs, out = str(tmp_path / 'hic.pairs'), str(tmp_path / 'out.json')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), HAPHIC_TABLE_PIECE='5000')
    env.pop('MASTER_PORT', None)
    rc = ranks.launch(['timeout', '-k', '10', '240', sys.executable, JOB, pairs, out], world, host_transport=True, env=env)
    assert rc == 0
    with open(out) as f:
        got = json.load(f)
    names = fx['names']
    # ---- pass one against the reference's fixture
    assert [n for n, _v in got['cov']] == names
    for k, (n, v) in enumerate(got['cov']):
        assert v == fx['cov_flat'][fx['cov_ptr'][k]:fx['cov_ptr'][k + 1]].tolist(), n
    at = {n: k for k, n in enumerate(fx['meta']['pos_keys'])}
    assert sorted(n for n, _v in got['pos']) == sorted(at)
    for n, v in got['pos']:
        assert v == fx['pos_flat'][fx['pos_ptr'][at[n]]:fx['pos_ptr'][at[n] + 1]].tolist(), n
    # ---- pass two against the conversion of the whole stream
    cid = {n: k for k, n in enumerate(got['corrected'])}
    assert got['src_names'] == [n for n in names if n not in got['fpos']] + list(got['fpos'])
    sid = {n: k for k, n in enumerate(names)}
    want = []
    for a, p, b, q in zip(fx['id1'].tolist(), fx['pos1'].tolist(), fx['id2'].tolist(), fx['pos2'].tolist()):
        i, x = _convert(names, cid, got['fpos'], got['ffrag'], a, p)
        j, y = _convert(names, cid, got['fpos'], got['ffrag'], b, q)
        if i >= 0 and j >= 0:
            want.append([i, x, j, y])
    assert len(want) > 30_000 and sid
    assert got['pass_two'] == want
    # ---- every rank parsed its share of the lines, in both phases
    with open(pairs, 'rb') as f:
        n_lines = len(f.read().splitlines())
    records = [got['record']]
    for r in range(1, world):
        with open('%s.rank%d' % (out, r)) as f:
            records.append(json.load(f))
    for phase in ('correct_pass1', 'ingest'):
        lines = [sum(p['lines'] for p in rec if p['phase'] == phase) for rec in records]
        assert sum(lines) == n_lines and all(k > 0 for k in lines), (phase, lines)
    sent = [p['bytes_sent'] for rec in records[1:] for p in rec if p['phase'] == 'correct_pass1']
    assert len(sent) == world - 1 and all(b > 0 for b in sent)


def test_correct_spec_and_ingest_spec_carry_what_a_worker_needs(tmp_path):
    from haphic_amd import cluster, correct
    p = tmp_path / 'x.pairs'
    p.write_bytes(b'r\ta\t1\tb\t2\n')
    text = cluster.PairsText(str(p), 'pairs', False, chunk_bytes=1234, bed_path=None)
    spec = ranks.correct_spec(text, ['a', 'b'], [np.int64(10), 20], np.int32(500))
    assert spec == {'path': str(p), 'format': 'pairs', 'names': ['a', 'b'], 'lens': [10, 20], 'resolution': 500, 'chunk_bytes': 1234}
    assert ranks.ingest_spec(text, ['a', 'b'], False)['remap'] is None
    fixed = correct.CorrectedPairsText(str(p), 'pairs', True, {'a': [40, 0]}, {'a': ['a:41-100', 'a:1-40']})
    fixed.remap_tables = tuple(np.asarray(t, np.int32) for t in correct._remap_tables(['b', 'a:1-40', 'a:41-100'], fixed._break_pos, fixed._break_frag)[1:])
    spec = ranks.ingest_spec(fixed, ['b', 'a'], False)
    assert spec['names'] == ['b', 'a'] and spec['inter_only'] is True
    assert spec['remap'] == ([0, 1, 3], [0, 0, 40], [0, 1, 2])
