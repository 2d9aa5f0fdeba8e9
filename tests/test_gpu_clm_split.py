"""The CLM splitter (hhx_clm_split_*, haphic_amd/csrc/hhx_clmsplit.hip) against the contract of split_clm_file
(scripts/HapHiC_reassign.py:581-622) on the corpus of tests/clm_split_cases.py: every group's file equals split_spec — and the
golden fixture the reference's own function wrote — byte for byte, for every way of cutting the text into pushes; the device's
counters equal what the host mirror of the state machine predicts; a line with fewer than two tokens raises the reference's
IndexError wherever it falls.
Run on the GPU box:  python -m pytest tests/test_gpu_clm_split.py -m gpu"""
import os

import numpy as np
import pytest

from haphic_amd import _lib
from tests import clm_split_cases as cc
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

REACHED = dict.fromkeys(cc.STATS, 0)
SMALL = cc.cases(cc.SMALL_SECTIONS)
SMALL_IDS = ['%s-%s' % (c.section, c.name) for c in SMALL]


def split(tmp, pieces, names, group_of_name, n_groups, file_chunk=None):
    """-> ([bytes per group], counters, (lines, kept, bytes per group) of finish); pieces: the pushes, or the path of a file with file_chunk"""
    paths = [os.path.join(str(tmp), 'g%d.clm' % g) for g in range(n_groups)]
    s = _lib.ClmSplit(names, group_of_name, paths)
    try:
        if file_chunk is not None:
            s.push_file(pieces, file_chunk, 2)
        else:
            for p in pieces:
                s.push(p)
        totals = s.finish()
        stats = s.stats()
    finally:
        s.close()
    for k, v in stats.items():
        REACHED[k] += v
    outs = []
    for p in paths:
        with open(p, 'rb') as f:
            outs.append(f.read())
    assert [len(o) for o in outs] == totals[2].tolist()
    return outs, stats, totals


def check(tmp, case, pieces, counters=False):
    if case.want is IndexError:
        with pytest.raises(IndexError, match='^list index out of range$'):
            split(tmp, pieces, *case.args())
        return
    outs, stats, totals = split(tmp, pieces, *case.args())
    assert outs == case.want, (case, [len(p) for p in pieces][:8])
    want_outs, want_stats = cc.simulate(pieces, *case.args())
    assert totals[0] == want_stats['lines'] and totals[1] == want_stats['kept']
    if counters:
        assert stats == want_stats, case


@pytest.mark.parametrize('case', SMALL, ids=SMALL_IDS)
def test_small_cases_one_push_and_fixed_pushes(case, tmp_path):
    check(tmp_path, case, [case.text], counters=True)
    for size in (1, 2, 3, 7, 64):
        check(tmp_path, case, cc.pushes(case.text, size), counters=True)


@pytest.mark.parametrize('case', [c for c in SMALL if c.small], ids=[i for i, c in zip(SMALL_IDS, SMALL) if c.small])
def test_small_cases_two_pushes_cut_at_every_offset(case, tmp_path):
    """inside the first token, between the tokens, around the dropped byte, inside the distances, between '\\r' and '\\n', behind a lone '\\r', on a break"""
    for cut in range(len(case.text) + 1):
        check(tmp_path, case, [case.text[:cut], case.text[cut:]], counters=True)


def test_golden_fixture_of_the_reference(tmp_path):
    cases = cc.golden_cases(load_golden('clm_split.npz'))
    assert len(cases) > 50
    for name, text, names, group, G, want in cases:
        if want is IndexError:
            with pytest.raises(IndexError, match='^list index out of range$'):
                split(tmp_path, [text], names, group, G)
        else:
            assert split(tmp_path, [text], names, group, G)[0] == want, name
            assert split(tmp_path, cc.pushes(text, 5), names, group, G)[0] == want, name


@pytest.mark.parametrize('shift', ['dst', 'src'])
@pytest.mark.parametrize('length', cc.SIZE_LENGTHS)
def test_line_lengths_at_the_block_and_the_tile_in_every_alignment_phase(length, shift, tmp_path):
    """lines of TX_BLOCK and GATHER_TILE -1 / 0 / +1 bytes, source and destination moved through the 16 phases of a 16-byte store: the
    counters say which tiles held several lines and which lines spanned tiles, as the host mirror lays them out"""
    multi = span = 0
    for phase in range(16):
        case = cc.size_case(length, phase, shift)
        outs, stats, _ = split(tmp_path, [case.text], *case.args())
        assert outs == case.want, case
        assert stats == cc.simulate([case.text], *case.args())[1], case
        multi += stats['multi_line_tiles']
        span += stats['multi_tile_lines']
        for size in (64, 1000):
            pieces = cc.pushes(case.text, size)
            outs, stats, _ = split(tmp_path, pieces, *case.args())
            assert outs == case.want and stats == cc.simulate(pieces, *case.args())[1], (case, size)
    assert multi >= 16 and (span >= 16 or length < cc.GATHER_TILE - 16)


def test_block_sized_line_in_tiny_pushes(tmp_path):
    case = cc.size_case(cc.TX_BLOCK + 1, 0, 'dst')
    for size in (1, 2, 3, 7):
        pieces = cc.pushes(case.text[:cc.TX_BLOCK + 200], size)
        want = cc.simulate(pieces, *case.args())
        outs, stats, _ = split(tmp_path, pieces, *case.args())
        assert outs == want[0] == cc.split_spec(case.text[:cc.TX_BLOCK + 200], *case.args()) and stats == want[1]
        assert stats['continuations'] > 100


def test_device_pointer_pushes_aligned_and_not(tmp_path):
    import torch
    case = cc.size_case(cc.GATHER_TILE + 1, 3, 'src')
    buf = torch.zeros(len(case.text) + 64, dtype=torch.uint8, device='cuda')
    for lead in (0, 5):
        buf[lead:lead + len(case.text)] = torch.frombuffer(bytearray(case.text), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        paths = [os.path.join(str(tmp_path), 'd%d.clm' % g) for g in range(case.n_groups)]
        s = _lib.ClmSplit(case.names, case.group_of_name, paths)
        try:
            at = 0
            for n in (7000, 1, 9000, len(case.text)):
                n = min(n, len(case.text) - at)
                s.push(device_ptr=buf.data_ptr() + lead + at, n_bytes=n)
                at += n
            s.finish()
        finally:
            s.close()
        assert [open(p, 'rb').read() for p in paths] == case.want


@pytest.mark.parametrize('kept', [True, False], ids=['kept', 'dropped'])
def test_one_300k_line_through_the_file_reader_in_4k_chunks(kept, tmp_path):
    text = cc.long_line_text(kept)
    clm = tmp_path / 'long.clm'
    clm.write_bytes(text)
    outs, stats, totals = split(tmp_path, str(clm), cc.NAMES3, cc.GROUP3, 3, file_chunk=4096)
    assert outs == cc.split_spec(text, cc.NAMES3, cc.GROUP3, 3)
    assert stats == cc.simulate(cc.pushes(text, 4096), cc.NAMES3, cc.GROUP3, 3)[1]
    assert stats['continuations'] >= 300_000 // 4096 and totals[0] == 5 and (len(outs[0]) > 300_000) == kept


def test_first_token_beyond_the_head_bound_is_refused(tmp_path):
    text = cc.head_bound_text()
    for pieces in ([text], cc.pushes(text, 4096), cc.pushes(text, 50_000)):
        with pytest.raises(RuntimeError, match='first two tokens of a line do not end within 65536 bytes'):
            split(tmp_path, pieces, cc.NAMES3, cc.GROUP3, 3)
    ok = b'ctgA+' + b' ' * (cc.HEAD_MAX - 12) + b'ctgB- 1 5\n'         # the second token ends on byte HEAD_MAX - 1
    assert split(tmp_path, cc.pushes(ok, 4096), ['ctgA', 'ctgB'], [0, 0], 1)[0] == [ok]
    assert split(tmp_path, [ok], ['ctgA', 'ctgB'], [0, 0], 1)[0] == [ok]


@pytest.fixture(scope='module')
def big_file(tmp_path_factory):
    text = cc.file_text(2 << 20, first_line_bytes=4097)               # the first line's "\r\n" lies across bytes 4095 | 4096
    d = tmp_path_factory.mktemp('clm_file')
    (d / 'paired_links.clm').write_bytes(text)
    return d, text, cc.split_spec(text, cc.NAMES3, cc.GROUP3, 3)


def test_file_in_chunks_equals_one_push(big_file):
    d, text, want = big_file
    one, stats_one, totals = split(d, [text], cc.NAMES3, cc.GROUP3, 3)
    assert one == want and stats_one == cc.simulate([text], cc.NAMES3, cc.GROUP3, 3)[1]
    assert stats_one['multi_line_tiles'] > 0 and stats_one['multi_tile_lines'] > 0 and stats_one['seams'] == 0
    for chunk in (4096, 65536):
        outs, stats, _ = split(d, str(d / 'paired_links.clm'), cc.NAMES3, cc.GROUP3, 3, file_chunk=chunk)
        assert outs == want, chunk
        assert stats == cc.simulate(cc.pushes(text, chunk), cc.NAMES3, cc.GROUP3, 3)[1], chunk
        assert stats['lines'] == totals[0] and stats['kept'] == totals[1]
    assert text[4095:4097] == b'\r\n'


def test_cr_on_the_last_byte_of_a_chunk_is_joined_with_its_lf(big_file):
    d, text, want = big_file
    outs, stats, _ = split(d, str(d / 'paired_links.clm'), cc.NAMES3, cc.GROUP3, 3, file_chunk=4096)
    assert stats['seams'] >= 1 and outs == want
    assert want[0].startswith(text[:4095] + b'\n')                   # one '\n' for the pair, not two lines


@pytest.mark.parametrize('where', ['first_push', 'later_push', 'open_at_finish'])
def test_bad_line_raises_the_reference_error(where, tmp_path):
    good = b'ctgA+ ctgB- 1 5\nctgC+ ctgD- 2 6 7\n'
    pieces = {'first_push': [good + b'ctgA+\n' + good, good], 'later_push': [good, good, good[:9], good[9:] + b' \t\r\n' + good],
              'open_at_finish': [good, good + b'ctgA+']}[where]
    s = _lib.ClmSplit(cc.NAMES3, cc.GROUP3, [str(tmp_path / ('g%d.clm' % g)) for g in range(3)])
    try:
        with pytest.raises(IndexError, match='^list index out of range$'):
            for p in pieces:
                s.push(p)
            s.finish()
        with pytest.raises(RuntimeError, match='failed'):             # the handle stays failed
            s.push(good)
    finally:
        s.close()
    with pytest.raises(IndexError):
        cc.split_spec(b''.join(pieces), cc.NAMES3, cc.GROUP3, 3)
    assert _lib.files_pending()[0] == 0


def test_null_handle_is_an_error_code():
    L = _lib.load()
    v = np.zeros(len(cc.STATS), np.int64)
    assert L.hhx_clm_split_push(None, None, 0, 0) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_clm_split_file(None, b'x', 4096, 1) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_clm_split_finish(None, None, None, None) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_clm_split_stats(None, _lib.ptr(v)) != 0 and b'null' in L.hhx_last_error()
    assert L.hhx_clm_split_destroy(None) == 0
    h = _lib.C.c_void_p()
    assert L.hhx_clm_split_create(1, None, None, None, 1, None, None, _lib.C.byref(h)) != 0
    with pytest.raises(RuntimeError, match='cannot open'):
        _lib.ClmSplit(['a'], [0], ['/nonexistent_dir/g.clm'])


def test_reassign_seam_reproduces_the_reference_tree(tmp_path, monkeypatch):
    from haphic_amd import reassign
    text, group_ctg_dict, ctg_group_dict, subdir = cc.seam_inputs()
    clm = tmp_path / 'paired_links.clm'
    clm.write_bytes(text)
    run = tmp_path / 'run'
    run.mkdir()
    monkeypatch.chdir(run)
    assert reassign.split_clm_file(str(clm), group_ctg_dict, ctg_group_dict, subdir) is None
    assert _lib.files_pending()[0] == 0
    assert cc.read_tree(str(run)) == cc.golden_tree(load_golden('clm_split.npz'))


def test_every_counter_was_reached():
    """(the last test of the file: REACHED sums hhx_clm_split_stats over the tests above)"""
    assert all(REACHED.values()), REACHED
