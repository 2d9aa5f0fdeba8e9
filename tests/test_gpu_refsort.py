"""`haphic refsort` on the device: the jobs of tests/refsort_cases.py through the library against what the reference gave (tests/golden/refsort.npz),
and the three kernels — csrc/hhx_paf.hip behind _lib.Paf, hhx_lis_sums, hhx_fasta_emit_segments — against the numpy restatements of
tests/refsort_cases.py (pinned to the same fixture by tests/test_refsort_cpu.py) at the seams of their blocks, chunks, stores and slabs."""
import os

import numpy as np
import pytest

from haphic_amd import _lib, refsort, scaffolds
from tests import build_cases as bc
from tests import refsort_cases as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = rc.golden(np.load(os.path.join(HERE, 'golden', 'refsort.npz')))
CASES = rc.cases()
SERVED = [c for c in CASES if c.served]
BLOCK = 4096                   # TX_BLOCK of csrc/hhx_textscan.h


@pytest.fixture(autouse=True)
def default_knobs():
    yield
    _lib.tune('fasta_slab', None)
    _lib.tune('sort_verdict_lds_n', None)


# ------------------------------------------------------------------ the jobs
@pytest.mark.parametrize('source, slab', [('path', None), ('bytes', bc.SLAB_MIN)], ids=['path_default_slab', 'bytes_min_slab'])
@pytest.mark.parametrize('case', SERVED, ids=repr)
def test_jobs_give_the_reference_results_on_the_device(case, source, slab, tmp_path):
    _lib.tune('fasta_slab', slab)
    refsort.STATS.clear()
    rec = rc.run_mirrors(case, str(tmp_path), _lib, refsort, scaffolds, paf_source=source)
    assert rec == GOLDEN[case.name]
    assert refsort.STATS['parse_paf'] == 'device'
    if not rec['raises']:
        assert refsort.STATS['order_and_orient_groups'] == 'device'


# ------------------------------------------------------------------ the PAF reader
def same_table(text, source=None):
    want, got = rc.NumpyPaf(text), _lib.Paf(text if source is None else source)
    assert got.names() == want.names() and (got.n_rec, got.n_names) == (want.n_rec, want.n_names)
    for k in ('query', 'target', 'query_start', 'query_end', 'target_start', 'target_end', 'mapq', 'plus'):
        assert getattr(got, k).dtype == getattr(want, k).dtype and getattr(got, k).tolist() == getattr(want, k).tolist(), k
    return got


def paf_line(q='ctgA', qs=10, qe=5010, strand='+', t='chr1', ts=100, te=5100, mapq=60, tail='', sep='\t', eol='\n'):
    return sep.join(str(x) for x in (q, 300000, qs, qe, strand, t, 90000000, ts, te, 4000, 5000, mapq)).encode() + tail.encode() + eol.encode()


def pad_to(text, size, eol='\n'):
    """text + one valid line with a tag tail, `size` bytes in all"""
    short = paf_line(q='pad', tail='\tcg:Z:', eol=eol)
    assert size - len(text) >= len(short)
    return text + paf_line(q='pad', tail='\tcg:Z:' + 'M' * (size - len(text) - len(short)), eol=eol)


@pytest.mark.parametrize('eol', ['\n', '\r\n', '\r'], ids=['lf', 'crlf', 'cr'])
def test_reader_with_every_byte_of_a_line_on_the_block_seam(eol):
    """a line shifted byte by byte across the end of the first 4096-byte block: each separator as the last byte of the block, each of the first fields
    and the line start straddling the seam, '\\r' and '\\n' on either side of it"""
    probe = paf_line(q='ctg_straddle', qs=123456, qe=654321, t='chrom_7', ts=1234567, te=7654321, mapq=17, tail='\tNM:i:3', eol=eol)
    for shift in range(0, len(probe) + 3):
        head = pad_to(paf_line(eol=eol), BLOCK - shift, eol)
        assert len(head) == BLOCK - shift and head.endswith(eol.encode())
        got = same_table(head + probe + paf_line(q='after', t='ctg_straddle', eol=eol))
        assert got.n_rec == 4 and got.names()[-2:] == ['chrom_7', 'after'] and got.mapq.tolist()[2] == 17


def test_reader_skips_a_long_tail_and_reads_what_follows(tmp_path):
    rng = np.random.default_rng(5)
    tail = '\tcg:Z:' + ''.join('%d%s' % (n, 'MID'[k % 3]) for k, n in enumerate(rng.integers(1, 999, 20000)))      # > 64 KB: many blocks without a line start
    assert len(tail) > 1 << 16
    text = paf_line() + paf_line(q='long', tail=tail) + paf_line(q='next', t='long', mapq=3) + paf_line(q='long', tail=tail + ' \t x', eol='\r\n') + paf_line(q='z')
    got = same_table(text)
    assert got.names() == ['ctgA', 'chr1', 'long', 'next', 'z'] and got.mapq.tolist() == [60, 60, 3, 60, 60]
    path = str(tmp_path / 'aln.paf')
    with open(path, 'wb') as f:
        f.write(text)
    same_table(text, path)


def test_reader_line_and_field_dialects():
    twelve = paf_line()
    assert twelve.count(b'\t') == 11 and twelve.endswith(b'60\n')                      # the break right behind field 11
    text = (twelve + b'\n \t \n\x0b\x0c\x1c\x1d\x1e\x1f\n' + paf_line(sep=' \t  ', q='  \tlead', eol=' \n') + paf_line(q='cr', eol='\r') + b'\r' + paf_line(q='crlf', eol='\r\n')
            + paf_line(q='same', t='same', mapq='00') + paf_line(q='q', strand='-') + paf_line(q='q', strand='++') + paf_line(q='q', strand='+x')
            + paf_line(q='big', qs='9' * 18, qe='0' * 17 + '7', te='000', tail='\tcg:Z:5M\x1f', eol='\x0b\n') + paf_line(q='n' * 255, t='m' * 255))
    got = same_table(text)
    assert got.plus.tolist() == [True, True, True, True, True, False, False, False, True, True] and got.mapq[4] == 0 and got.query[4] == got.target[4]
    assert got.query_start[8] == 10 ** 18 - 1 and got.query_end[8] == 7
    same_table(text[:-1])                                        # the last line without a break
    same_table(twelve[:-1])
    same_table(twelve[:-1] + b'\r')
    for empty in (b'', b'\n', b' \t\r\n\r\r\n', b'\x1c'):
        assert same_table(empty).n_rec == 0


@pytest.mark.parametrize('grid', ['1', '2'])
def test_reader_grid_stride_loops(grid, monkeypatch):
    rng = np.random.default_rng(int(grid))
    names = ['ctg%d' % k for k in range(40)] + ['chr%d' % k for k in range(5)]
    lines = [paf_line(q=names[rng.integers(45)], t=names[rng.integers(45)], qs=int(rng.integers(1 << 40)), qe=int(rng.integers(1 << 40)), mapq=int(rng.integers(61)),
                      strand='+-'[rng.integers(2)], tail='\tcg:Z:' + 'M' * int(rng.integers(0, 3000)), eol=['\n', '\r\n', '\r', '\n\n'][rng.integers(4)])
             for _ in range(700)]
    text = b''.join(lines)
    assert len(text) > 200 * BLOCK
    want = same_table(text)
    monkeypatch.setenv('HHX_PAF_GRID', grid)
    got = same_table(text)
    assert got.names() == want.names() and got.query.tolist() == want.query.tolist()


@pytest.mark.parametrize('why, text', [('19 digits', paf_line() + paf_line(qs='1' * 19)), ('a sign', paf_line(mapq='+5')), ('an underscore', paf_line(te='1_0')),
                                       ('eleven fields', paf_line() + b'\t'.join(paf_line().split(b'\t')[:11]) + b'\n' + paf_line()),
                                       ('eleven fields, then a long line', b'\t'.join(paf_line().split(b'\t')[:11]) + b'\n' + paf_line(tail='\tx' * 40)),
                                       ('a high byte', paf_line(tail='\tco:Z:caf') + b'\x80\n'), ('a name of 256 bytes', paf_line(t='m' * 256)),
                                       ('a query of 256 bytes', paf_line(q='m' * 256)), ('a letter in an integer', paf_line(qe='12a')),
                                       ('a skipped line is read too', paf_line(mapq=0, ts='x'))], ids=lambda x: x if isinstance(x, str) else None)
def test_reader_refusals_make_no_handle(why, text, tmp_path):
    with pytest.raises(rc.NumpyPaf.Unsupported):
        rc.NumpyPaf(text)
    with pytest.raises(_lib.Paf.Unsupported) as e:
        _lib.Paf(text)
    if 'fields' in why:
        assert 'line 2' in str(e.value) if why == 'eleven fields' else 'line 1' in str(e.value)
    L, h, buf = _lib.load(), _lib.C.c_void_p(), np.frombuffer(text, np.uint8)
    assert L.hhx_paf_open_bytes(_lib.ptr(buf), buf.size, _lib.C.byref(h)) == _lib.HHX_UNSUPPORTED and not h
    path = str(tmp_path / 'bad.paf')
    with open(path, 'wb') as f:
        f.write(text)
    assert L.hhx_paf_open(os.fsencode(path), _lib.C.byref(h)) == _lib.HHX_UNSUPPORTED and not h
    ctg_group = {'ctgA': [('g', 1, 300000, 1, 300000, 1)]}
    assert refsort.parse_paf(path, ctg_group, 5000, _original=lambda *a: 'theirs') == 'theirs' and refsort.STATS['parse_paf'] == 'reference'


def test_reader_paths_and_null_handles(tmp_path):
    with pytest.raises(_lib.Paf.Unsupported):
        _lib.Paf(str(tmp_path))                                  # no regular file
    with pytest.raises(RuntimeError):
        _lib.Paf(str(tmp_path / 'missing.paf'))
    L, n = _lib.load(), _lib.C.c_int64(0)
    assert L.hhx_paf_counts(None, _lib.C.byref(n), None, None) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_paf_table(None, *[None] * 10) != 0 and L.hhx_paf_close(None) == 0
    assert L.hhx_paf_open_bytes(None, 0, None) != 0


# ------------------------------------------------------------------ both LIS sums
def random_sequences(rng, lengths, span=None, wmax=5000):
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    value = np.concatenate([rng.integers(-(span or max(2 * n, 2)), (span or max(2 * n, 2)) + 1, n) for n in lengths] + [np.zeros(0, np.int64)])
    return ptr, value.astype(np.int64), rng.integers(1, wmax + 1, value.size).astype(np.int64)


def same_sums(ptr, value, weight):
    want_f, want_r = rc.lis_sums(ptr, value, weight)
    got_f, got_r = _lib.lis_sums(ptr, value, weight)
    assert got_f.dtype == np.int64 and got_f.tolist() == want_f.tolist() and got_r.tolist() == want_r.tolist()
    return got_f, got_r


def test_lis_chunk_seams_and_unequal_sequences():
    rng = np.random.default_rng(8)
    for n in (1, 2, 63, 64, 65, 129):                            # the wave takes 64 elements at a time
        same_sums(*random_sequences(rng, [n]))
        same_sums(*random_sequences(rng, [n], span=6))           # many repeats and zeros
    same_sums(*random_sequences(rng, [5, 0, 129, 1, 64, 0, 0, 200, 2, 65, 17, 63, 300]))
    same_sums(*random_sequences(rng, list(rng.integers(0, 40, 300))))
    f, r = same_sums([0, 0, 0], [], [])
    assert f.tolist() == [0, 0] and r.tolist() == [0, 0]
    assert _lib.lis_sums([0], [], [])[0].size == 0


def test_lis_classes_repeats_and_zero():
    f, r = same_sums([0, 4], [2, 6, 4, 2], [5, 1, 3, 50])       # a repeat as the last element: dropped
    assert (f.tolist(), r.tolist()) == ([8], [0])
    f, r = same_sums([0, 3, 6, 10], [1, 2, 3, -3, -2, -1, 0, 4, 0, -4], [1, 2, 3, 1, 2, 3, 7, 1, 100, 2])
    assert (f.tolist(), r.tolist()) == ([6, 0, 8], [0, 6, 7])   # all of one class; 0 stands in both, its repeat in neither
    rng = np.random.default_rng(9)
    v = np.arange(1, 101, dtype=np.int64)
    for values in (v, -v, v[::-1].copy(), -v[::-1].copy(), rng.permutation(v)):
        same_sums([0, 100], values, rng.integers(1, 9, 100))


def test_lis_wide_cells_and_both_tree_forms():
    rng = np.random.default_rng(10)
    ptr, value, weight = random_sequences(rng, [100, 7, 101, 64])
    wide = weight.copy()
    wide[:100] += 1 << 26                                        # the first sequence sums to more than 2^32: 8-byte cells for the call
    assert int(wide[:100].sum()) >= 1 << 32
    for w in (weight, wide):
        want = rc.lis_sums(ptr, value, w)
        for lds_n in (None, 4095, 101, 100, 64, 10, 0):          # LDS for all; the seam between the sequences; HBM scratch for all
            _lib.tune('sort_verdict_lds_n', lds_n)
            got = _lib.lis_sums(ptr, value, w)
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), lds_n
    big = np.array([1 << 61, 1 << 60, 5], np.int64)              # below 2^62 in all
    f, r = same_sums([0, 3], [1, 2, 3], big)
    assert f.tolist() == [int(big.sum())]


def test_lis_refusals():
    for ptr, value, weight in (([0, 2], [1, 2], [5, 0]), ([0, 2], [1, 2], [5, -1]), ([0, 2, 4], [1, 2, 1, 2], [1, 1, 1 << 61, 1 << 61])):
        with pytest.raises(_lib.LisUnsupported):
            _lib.lis_sums(ptr, value, weight)
        with pytest.raises(rc.LisUnsupported):
            rc.lis_sums(ptr, value, weight)
    n = rc.MAX_N + 1
    with pytest.raises(_lib.LisUnsupported, match='beyond'):
        _lib.lis_sums([0, n], np.arange(n), np.ones(n, np.int64))
    with pytest.raises(RuntimeError):
        _lib.lis_sums([1, 2], [1, 2], [1, 1])                    # ptr[0] != 0: a caller's mistake, not a hand-back
    with pytest.raises(ValueError):
        _lib.lis_sums([0, 3], [1, 2], [1, 1])


# ------------------------------------------------------------------ records of sub-ranges and N runs
LENS = (100, 37, 5000, 1, 16, 4200)


@pytest.fixture(scope='module')
def assembly():
    rng = np.random.default_rng(12)
    text = b''.join(b'>s%d\n' % k + bc.wrap(bc.bases(rng, n), 60) for k, n in enumerate(LENS))
    return rc.NumpyFasta(text, keep_letter_case=True), _lib.Fasta(text, keep_letter_case=True)


def same_file(assembly, tmp_path, records, width, tag=''):
    """records: [(name, [(ctg, start0, len, rev) | int Ns, ...])]"""
    theirs, ours = assembly
    names, off, ctg, start, length, rev = [], [0], [], [], [], []
    for name, parts in records:
        names.append(name)
        for p in parts:
            c, s, m, r = (-1, 0, p, 0) if isinstance(p, int) else p
            ctg.append(c), start.append(s), length.append(m), rev.append(r)
        off.append(len(ctg))
    a, b = str(tmp_path / ('theirs' + tag)), str(tmp_path / ('ours' + tag))
    n = theirs.emit_segments(a, names, off, ctg, start, length, rev, width)
    assert ours.emit_segments(b, names, off, ctg, start, length, rev, width) == n
    assert open(b, 'rb').read() == open(a, 'rb').read()
    return open(b, 'rb').read()


RECORDS = [('odd_ranges', [(2, 3, 45, 0), (2, 1001, 333, 1), (0, 7, 93, 1), (2, 17, 4099, 0), (5, 1, 4199, 1)]),             # starts and lengths off every multiple of 16
           ('down_to_byte_0', [(0, 0, 100, 1), 1, (2, 0, 17, 1), (1, 0, 37, 1), (3, 0, 1, 1), (0, 0, 1, 1), (4, 0, 16, 1)]),  # reversed ranges that end at byte 0
           ('n_runs', [0, (1, 5, 9, 0), 1, (1, 5, 9, 1), 15, (3, 0, 1, 0), 16, (4, 0, 16, 0), 17, (1, 0, 0, 1), 4097, (0, 99, 1, 0), 0]),
           ('only_n', [0, 1, 15, 16, 17, 4097]),
           ('empty', []),
           ('empty_pieces', [0, (2, 5000, 0, 0), (0, 0, 0, 1), 0]),
           ('iupac', [(2, 100, 300, 1), (5, 4000, 200, 1)]),                                                                       # bytes outside ATCGNatcgn stay
           ('last', [(3, 0, 1, 0)])]


@pytest.mark.parametrize('slab', [None, bc.SLAB_MIN], ids=['default_slab', 'min_slab'])
@pytest.mark.parametrize('width', [1, 7, 60, 4099, 1 << 40])
def test_emit_segments_equals_the_gathers(assembly, width, slab, tmp_path):
    _lib.tune('fasta_slab', slab)
    data = same_file(assembly, tmp_path, RECORDS, width)
    assert b'>empty\n>empty_pieces\n>iupac\n' in data and data.endswith(b'>last\n' + assembly[0].sequences()[sum(LENS[:3]):sum(LENS[:3]) + 1].tobytes() + b'\n')
    assert any(c in data for c in b'RYKMSWryBDHVbd')


@pytest.mark.parametrize('width', [1, 7, 60])
def test_emit_segments_piece_seams_on_and_next_to_line_ends(assembly, width, tmp_path):
    """the seam between two pieces at every column of a line, for a forward, a reversed and an N piece on either side"""
    records = []
    for a in range(0, 2 * width + 2):
        records.append(('seam%d' % a, [(2, 11, a, 0), (2, 500, width + 1, 1), a % 3, (2, 2, a, 1), (5, 1, 2 * width, 0), 2 * width - a % width]))
    same_file(assembly, tmp_path, records, width)
    _lib.tune('fasta_slab', bc.SLAB_MIN)                         # and the same records cut by slab seams
    same_file(assembly, tmp_path, records, width, '_min_slab')


def test_emit_segments_refusals_leave_no_file(assembly, tmp_path):
    _theirs, fa = assembly
    out = str(tmp_path / 'out.fa')
    for ctg, start, length, width in ((0, 0, 101, 60), (0, 100, 1, 60), (0, -1, 5, 60), (1, 30, 8, 60), (0, 0, -1, 60), (-1, 0, -1, 60), (0, 0, 5, 0), (0, 0, 5, -7),
                                      (-1, 0, (1 << 60) + 1, 60)):
        with pytest.raises(_lib.Fasta.Unsupported):
            fa.emit_segments(out, ['g'], [0, 1], [ctg], [start], [length], [0], width)
        assert not os.path.exists(out)
    with pytest.raises(RuntimeError):                            # a contig the table does not have
        fa.emit_segments(out, ['g'], [0, 1], [len(LENS)], [0], [1], [0], 60)
    with pytest.raises(RuntimeError):
        fa.emit_segments(out, ['g'], [0, 1], [-2], [0], [1], [0], 60)
    assert not os.path.exists(out)
    assert fa.emit_segments(out, ['g', 'e'], [0, 3, 3], [0, -1, 1], [96, 0, 0], [4, 2, 3], [1, 0, 0], 4) == os.path.getsize(out)
    assert fa.emit_segments(out, [], [0], [], [], [], [], 60) == 0 and open(out, 'rb').read() == b''
    L = _lib.load()
    assert L.hhx_fasta_emit_segments(None, b'x', 0, None, None, None, None, None, None, None, 60, None) != 0 and b'null' in L.hhx_last_error()
