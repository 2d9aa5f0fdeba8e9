"""paired_links.clm as the device writes it (hhx_ingest_write_clm, ingest_write_clm_fd in csrc/hhx_pairs.hip; FileSink in csrc/hhx_filesink.h)
against the contract of tests/clm_write_cases.py, at the chunk, block, digit and piece seams its corpus constructs.  The counters of the
library ("clm_chunks", "clm_blocks_direct", "sink_pieces") must read what the host mirror predicts: the test that names a seam also proves
that the run went through it."""
import logging
import os

import numpy as np
import pytest

from haphic_amd import _lib, cluster
from tests import clm_write_cases as cw

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_knobs():
    _lib.profile_enable(True)
    yield
    _lib.tune('clm_chunk', None)
    _lib.tune('sink_piece', None)
    _lib.profile_enable(False)


def _ingest(c):
    ing = _lib.Ingest(c.table, cw.FLANK)
    ing.keep_pairs()
    for part in c.pushes():
        ing.push(*part)
    ing.finalize()
    return ing


def _write(c, ing, path, clm_chunk=None, sink_piece=None):
    """one file in place under the two knobs -> its bytes; lines, bytes and the three counters checked against the file and the mirror"""
    _lib.tune('clm_chunk', clm_chunk)
    _lib.tune('sink_piece', sink_piece)
    _lib.profile_reset()
    lines, nbytes = ing.write_clm(str(path), c.names)
    seen = {k: _lib.profile_counter(k) for k in cw.COUNTERS}
    got = open(path, 'rb').read()
    print('%s clm_chunk=%s sink_piece=%s: %d bytes, %s' % (c.name, clm_chunk, sink_piece, len(got), seen))
    assert got == c.text, cw.first_difference(c, got, clm_chunk)
    assert nbytes == len(got) == os.path.getsize(path) and lines == got.count(b'\n')
    assert seen == cw.counters(c.plan(clm_chunk, sink_piece))
    return got


@pytest.mark.parametrize('name', cw.CASE_NAMES)
def test_every_case_against_the_contract(tmp_path, name):
    c = cw.case(name)
    ing = _ingest(c)
    _write(c, ing, tmp_path / 'x.clm')
    if not c.text:
        assert ing.write_clm(str(tmp_path / 'e.clm'), c.names) == (0, 0)
    ing.destroy()


@pytest.mark.parametrize('name', cw.CHUNK_SWEEP_CASES)
def test_clm_chunk_sweep(tmp_path, name):
    """every "clm_chunk" gives the file of the default: one contig pair per chunk (4: each larger than the chunk), cuts on the equality (8 and the
    value tests/test_clm_write_cases_cpu.py proves), chunks with their own line bits (1024)"""
    c = cw.case(name)
    ing = _ingest(c)
    for v in cw.chunk_settings(name):
        _write(c, ing, tmp_path / 'x.clm', clm_chunk=v)
    _write(c, ing, tmp_path / 'x.clm', clm_chunk=1)                    # clamped to 4
    ing.destroy()


@pytest.mark.parametrize('name', cw.PIECE_SWEEP_CASES)
def test_sink_piece_sweep(tmp_path, name):
    """every "sink_piece" gives the same file: more pieces than pinned buffers (4096), a piece as long as the file, and, with "clm_chunk" 1024,
    chunks shorter and longer than a piece, every one at its own offset of the file"""
    c = cw.case(name)
    ing = _ingest(c)
    for v in cw.piece_settings(name):
        _write(c, ing, tmp_path / 'x.clm', sink_piece=v)
        _write(c, ing, tmp_path / 'x.clm', clm_chunk=1024, sink_piece=v)
    _write(c, ing, tmp_path / 'x.clm', sink_piece=len(c.text) - 1)     # one byte in a piece of its own
    _write(c, ing, tmp_path / 'x.clm', sink_piece=1)                   # clamped to 4096
    ing.destroy()


@pytest.mark.parametrize('drop_pairs', [False, True])
def test_queued_equals_in_place(tmp_path, drop_pairs):
    """hhx_ingest_write_clm_async: the same writer on the library's file-writer thread (its own stream and pool arena), several chunks and pieces"""
    c = cw.case('random')
    ing = _ingest(c)
    _lib.tune('clm_chunk', cw.equality_chunk('random') * 8)
    _lib.tune('sink_piece', 4096 * 3)
    assert cw.case('random').plan(cw.equality_chunk('random') * 8)['n_chunks'] >= 3
    ing.write_clm(str(tmp_path / 'a.clm'), c.names)
    ing.write_clm_async(str(tmp_path / 'b.clm'), c.names, drop_pairs=drop_pairs)
    _lib.files_join()
    assert (tmp_path / 'a.clm').read_bytes() == (tmp_path / 'b.clm').read_bytes() == c.text
    if drop_pairs:
        with pytest.raises(RuntimeError, match='released'):
            ing.fetch_ht_order()
        with pytest.raises(RuntimeError, match='released'):
            ing.write_clm(str(tmp_path / 'c.clm'), c.names)
    else:
        assert len(ing.fetch_ht_order()) == len(c.want['full_i'])
        assert ing.write_clm(str(tmp_path / 'c.clm'), c.names) == (c.text.count(b'\n'), len(c.text))
    ing.destroy()


@pytest.mark.parametrize('name', cw.REFUSED_NAMES)
def test_position_beyond_the_contig_is_refused(tmp_path, name):
    """the ingest takes such a read pair (the reference does not look at it either); the CLM writer refuses the stream, in place and, on the
    caller's thread and before the file exists, queued"""
    c = cw.case(name)
    ing = _ingest(c)
    assert ing.n_full == len(c.want['full_i'])
    with pytest.raises(RuntimeError, match='beyond the end'):
        ing.write_clm(str(tmp_path / 'x.clm'), c.names)
    with pytest.raises(RuntimeError, match='beyond the end'):
        ing.write_clm_async(str(tmp_path / 'q.clm'), c.names)
    _lib.files_join()
    assert not os.path.exists(tmp_path / 'q.clm')
    ing.destroy()


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append((record.levelname, record.getMessage()))


@pytest.mark.parametrize('name', cw.REFUSED_NAMES)
def test_refused_stream_takes_the_host_loop(tmp_path, monkeypatch, name):
    """cluster.output_clm on the frozen clm_dict of parse_alignments_for_ctgs: the refusal is logged and the reference's loop writes the file,
    negative distances included"""
    from tests.test_seam_containers import _args
    monkeypatch.chdir(tmp_path)
    c = cw.case(name)
    fa_dict = {nm: [None, int(ln), int(ln) // 256 + 1] for nm, ln in zip(c.names, c.lengths.tolist())}
    aln = cluster.IdArrays(c.names, c.id1, c.p1.astype(np.int32), c.id2, c.p2.astype(np.int32))
    out = cluster.parse_alignments_for_ctgs(aln, fa_dict, _args(), {n: v[1] for n, v in fa_dict.items()}, set(fa_dict), 'int32', 'int32')
    clm = out[3]
    assert clm.frozen
    seen = _Lines()
    cluster.logger.addHandler(seen)
    level = cluster.logger.level
    cluster.logger.setLevel(logging.INFO)
    try:
        cluster.output_clm(clm)
        cluster._lib.files_join()
    finally:
        cluster.logger.removeHandler(seen)
        cluster.logger.setLevel(level)
    warned = [m for lv, m in seen.lines if lv == 'WARNING']
    assert len(warned) == 1 and 'written by the host loop' in warned[0] and 'beyond the end' in warned[0]
    assert open('paired_links.clm', 'rb').read() == c.text
    assert (b'-898 -898' in c.text) == (name == 'beyond_negative')


def test_split_contigs_at_a_small_chunk(tmp_path, monkeypatch):
    """bins mode (parse_alignments, the COMBINED side records): the frozen clm_dict's file at "clm_chunk" 8 == the thawed dict's host loop"""
    from tests.test_seam_containers import _args, _case, _s5
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('HAPHIC_SYNC_FILES', '1')                        # in place: the counters below are this file's
    gen, fa_dict, aln = _case(n_pairs=3000, seed=17, split=True)
    args = _args(remove_allelic_links=2, max_read_pairs=40)
    out = _s5(fa_dict, aln, args, split=True)
    ref = _s5(fa_dict, aln, args, split=True)
    assert out[3].frozen and any('_bin' in a for a, _b in out[6][next(iter(out[6]))])
    _lib.tune('clm_chunk', 8)
    _lib.profile_reset()
    cluster.output_clm(out[3])
    cluster._lib.files_join()
    chunks = _lib.profile_counter('clm_chunks')
    os.rename('paired_links.clm', 'a.clm')
    ref[3]._thaw()
    cluster.output_clm(ref[3])
    want = open('paired_links.clm', 'rb').read()
    assert open('a.clm', 'rb').read() == want and len(want) > 1000
    kept = [len(v) // 4 for v in ref[3].values() if len(v) >= 8]
    assert chunks == cw.plan([(0, 0, n, np.zeros((4, n), np.int64)) for n in kept], np.zeros(1, np.int64), 8)['n_chunks'] >= 3
