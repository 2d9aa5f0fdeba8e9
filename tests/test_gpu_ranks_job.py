"""`haphic cluster --gpus N` on the one GPU of a test box: N ranks over the host transport, every file byte-identical to the one-rank run of
the same seam sequence (tests/ranks_job.py), cluster files equal to the reference's goldens; and the ranged text reader
(hhx_text_reader_open_range) handing out every line of a plain or BGZF file once, in order, for N = 1..16."""
import filecmp
import os
import pickle
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB = os.path.join(ROOT, 'tests', 'ranks_job.py')
STEP_S = 150                     # each rank's process: timeout -k 10 STEP_S


def _bgzip(data, block=4000):
    """BGZF of `data` in blocks of `block` bytes of text (+ the EOF block)"""
    from tests.bam_fixture import bgzf_block
    return b''.join(bgzf_block(data[k:k + block]) for k in range(0, len(data), block)) + bgzf_block(b'')


def _run(case, pairs, fmt, workdir, world, chunk_mb=None):
    from haphic_amd import ranks
    os.makedirs(workdir)
    cmd = ['timeout', '-k', '10', str(STEP_S), sys.executable, JOB, case, pairs, fmt, workdir]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('MASTER_PORT', None)
    if chunk_mb:
        env['HAPHIC_TEXT_CHUNK_MB'] = str(chunk_mb)
    rc = ranks.launch(cmd, world, host_transport=True, env=env)
    assert rc == 0, 'world {} job failed with status {}'.format(world, rc)


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


def _check_golden(case, d):
    from tests.conftest import load_golden
    g = load_golden({'toy': 'pipeline_toy.npz', 'c1': 'pipeline_c1.npz'}.get(case, 'pipeline_bins.npz'))
    for infl in g['inflations']:
        infl = str(infl)
        sub = os.path.join(d, 'inflation_' + infl)
        with open(os.path.join(sub, 'mcl_inflation_{}.clusters.txt'.format(infl))) as f:
            assert f.read() == str(g['clusters_txt_' + infl])
        groups = sorted(x for x in os.listdir(sub) if x.startswith('group'))
        assert groups == [str(x) for x in g['group_files_' + infl]]


@pytest.mark.gpu
@pytest.mark.parametrize('case,fmt,worlds', [('toy', 'pairs', (2, 3, 8)), ('toy', 'bgzipped_pairs', (3,)), ('bins', 'pairs', (2, 3)),
                                             ('bins_allelic', 'pairs', (3,)), ('c1', 'pairs', (2, 3)), ('c1', 'bgzipped_pairs', (2,))])
def test_n_ranks_write_the_files_of_one(tmp_path, case, fmt, worlds):
    from tests import ranks_job
    text = ranks_job.pairs_text(case)
    golden = case != 'bins_allelic' and (case != 'c1' or ranks_job.fixture('c1')[0]['same_pairs'])
    pairs = str(tmp_path / ('in.pairs' + ('.gz' if fmt != 'pairs' else '')))
    with open(pairs, 'wb') as f:
        f.write(text if fmt == 'pairs' else _bgzip(text))
    one = str(tmp_path / 'w1')
    _run(case, pairs, fmt, one, 1)
    assert os.path.getsize(os.path.join(one, 'alignments.bed')) > 0
    if golden:
        _check_golden(case, one)
    for world in worlds:
        d = str(tmp_path / ('w%d' % world))
        _run(case, pairs, fmt, d, world, chunk_mb=1 if case == 'c1' else None)     # c1: ~50 MB of text, several chunks on every rank
        _same_tree(one, d)
    if case == 'bins_allelic':
        with open(os.path.join(one, 'thawed.pkl'), 'rb') as f:
            assert pickle.load(f)['c2f']                 # the allelic path was reached


@pytest.mark.gpu
def test_ranged_reader_hands_out_every_line_once(tmp_path):
    from haphic_amd import _lib, ranks
    from tests import ranks_job
    _lib.check(_lib.load().hhx_set_device(0))
    text = ranks_job.pairs_text('toy')[:300_000]
    text = text[:text.rfind(b'\n') + 1] + b'x' * 9000 + b'\t1\n' + b'tail\twithout\tnewline'
    _check_shares(tmp_path, 'a', text, block=4000)
    # empty ranges: a line longer than a range (ranks inside it get nothing), more ranks than lines, a range without a block start
    _check_shares(tmp_path, 'long', b'y' * 50_000 + b'\tz\n' + b'r\ta\t1\tb\t2\n' * 3, block=20_000, want_empty=True)
    _check_shares(tmp_path, 'few', b'a\t1\nb\t2\n', block=4000, want_empty=True)
    _check_shares(tmp_path, 'empty', b'', block=4000)


def _check_shares(tmp_path, name, text, block, want_empty=False):
    import ctypes
    from haphic_amd import _lib, ranks
    plain, gz = str(tmp_path / (name + '.pairs')), str(tmp_path / (name + '.pairs.gz'))
    with open(plain, 'wb') as f:
        f.write(text)
    with open(gz, 'wb') as f:
        f.write(_bgzip(text, block))
    for path, bgzf in ((plain, False), (gz, True)):
        size = os.path.getsize(path)
        for world in range(1, 17):
            shares = []
            for b, e in ranks.byte_ranges(size, world):
                r = _lib.TextReader(path, 64 << 10, threads=2, bgzf=bgzf, byte_range=(b, e))
                try:
                    shares.append(b''.join(ctypes.string_at(h, n) for h, n in r))
                finally:
                    r.close()
            assert b''.join(shares) == text, (path, world)
            assert all(not s or s.endswith(b'\n') for s in shares[:-1]), (path, world)
            if not bgzf:
                assert shares == [text[lo:hi] for lo, hi in (ranks.owned_range(text, b, e) for b, e in ranks.byte_ranges(size, world))]
            if want_empty and world == 16:
                assert any(not s for s in shares), (path, 'no empty range')


@pytest.mark.gpu
def test_bgzf_cap_from_the_isize_trailers(tmp_path):
    """a small BGZF file that inflates far more than 12 x, with a line longer than 12 x the file: the pinned buffers are sized from the
    ISIZE trailers (an assumed 12 x ratio made this 'a line is longer than a chunk')"""
    import ctypes
    from haphic_amd import _lib
    _lib.check(_lib.load().hhx_set_device(0))
    text = b'r\t' + b'a' * 600_000 + b'\t1\tb\t2\n' + b'r\ta\t1\tb\t2\n' * 1000
    gz = tmp_path / 'dense.pairs.gz'
    gz.write_bytes(_bgzip(text, 60_000))
    assert len(text) > 12 * gz.stat().st_size + (256 << 10)
    r = _lib.TextReader(str(gz), 1 << 20, threads=2, bgzf=True)
    try:
        assert b''.join(ctypes.string_at(h, n) for h, n in r) == text
    finally:
        r.close()


def _sink_roundtrip(tmp_path, name, pieces, deferred, budget, base=0):
    """write `pieces` (sizes in bytes) of a known pattern through a byte sink from device memory; returns (file bytes, expected bytes)"""
    import ctypes
    import torch
    from haphic_amd import _lib
    from haphic_amd.sharded import HipEngine
    _lib.check(_lib.load().hhx_set_device(0))
    eng = HipEngine('cuda:0')
    path = str(tmp_path / name)
    prefix = bytes(range(256)) * (base // 256) + bytes(base % 256)
    with open(path, 'wb') as f:
        f.write(prefix)                                   # a deferred sink must not truncate what the ranks before it wrote
    sink = _lib.ByteSink(path, hbm_budget_bytes=budget, expected_bytes=64 << 20, deferred=deferred)
    want = []
    for k, n in enumerate(pieces):
        dev = ctypes.c_void_p()
        _lib.check(_lib.load().hhx_byte_sink_reserve(sink.h, n, ctypes.byref(dev)))
        src = (torch.arange(n, dtype=torch.int64, device='cuda:0') * (2 * k + 1) % 251).to(torch.uint8)
        eng.view(dev.value, n, '|u1', torch.uint8).copy_(src)
        torch.cuda.synchronize()
        _lib.check(_lib.load().hhx_byte_sink_commit(sink.h, dev, n))
        want.append(src.cpu().numpy().tobytes())
        del src
    if deferred:
        sink.set_base(base)
    sink.close()
    _lib.files_join()
    with open(path, 'rb') as f:
        got = f.read()
    import glob
    assert not glob.glob(path + '.part.*'), 'a part file was left behind'
    return got, prefix + b''.join(want)


@pytest.mark.gpu
def test_deferred_sink_spills_past_its_budget_and_places_at_base(tmp_path):
    """300 MB through a deferred sink with a budget of two 64 MB slabs: the parked ranges spill to the part file (in order), which set_base
    copies into place at a nonzero offset in front of the ranges still parked"""
    got, want = _sink_roundtrip(tmp_path, 'spill.bed', [40 << 20] * 7 + [12345], deferred=True, budget=128 << 20, base=1_000_003)
    assert len(got) == len(want) and got == want


@pytest.mark.gpu
@pytest.mark.parametrize('deferred', [False, True])
def test_sink_gives_a_piece_larger_than_a_slab_its_own(tmp_path, deferred):
    """a chunk whose BED outgrows the slabs (sized from a guess): a slab of its own, between ordinary pieces, not a failure"""
    got, want = _sink_roundtrip(tmp_path, 'big.bed', [3 << 20, 100 << 20, 5 << 20, 70 << 20, 1 << 20], deferred=deferred, budget=1 << 30,
                                base=4096 if deferred else 0)
    assert len(got) == len(want) and got == want
