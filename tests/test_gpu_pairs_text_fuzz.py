"""The .pairs tokeniser (hhx_pairs_parse, haphic_amd/csrc/hhx_text.hip) against Python's own line semantics on the generated
corpus of tests/pairs_text_cases.py: ids, positions and alignments.bed bytes equal oracle.parse_pairs_text exactly, through
every way in (host bytes, a host pointer, an aligned and an unaligned device pointer, wide mode, chunks, a byte sink), the
device's own counters say that every block took the reader and the BED path the host mirror plans for it, and a malformed
line raises what the reference raises, for the line the reference would stop at.
Run on the GPU box:  python -m pytest tests/test_gpu_pairs_text_fuzz.py -m gpu"""
import re

import numpy as np
import pytest

from haphic_amd import _lib
from oracle import oracle as orc
from tests import pairs_text_cases as ptc
from tests.conftest import tick

pytestmark = pytest.mark.gpu

REACHED = dict.fromkeys(ptc.COUNTERS + ('bed_direct_text_staged',), 0)
VALID = b'#h\nr1\tA\t5\tB\t7\n\nr2 Ct 11 Atg04 12 + -\r\nr3\tnone\t1\tA\t2147483648\n'


class Parsers:
    """one parser per FASTA name table, kept over the cases: its buffers are re-used from text to text"""

    def __init__(self, wide=False):
        self.wide, self.by_names = wide, {}

    def __call__(self, names):
        key = tuple(names)
        if key not in self.by_names:
            self.by_names[key] = _lib.PairsParser(names)
            if self.wide:
                self.by_names[key].set_wide(True)
        return self.by_names[key]

    def destroy(self):
        for ps in self.by_names.values():
            ps.destroy()


@pytest.fixture
def parsers():
    p = Parsers()
    yield p
    p.destroy()


def parse_counted(ps, text, **how):
    """parse(want_bed=True) with the profile counters on: (lines, the four event counters)"""
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        n = ps.parse(text, want_bed=True, **how)
    finally:
        _lib.profile_enable(False)
    return n, {k: _lib.profile_counter(k) for k in ptc.COUNTERS}


def differences(got, want):
    """which of (id1, pos1, id2, pos2, bed) differ, dtype included"""
    out = [k for k, (a, b) in zip(('id1', 'pos1', 'id2', 'pos2'), zip(got[:4], want[:4])) if a.dtype != b.dtype or not np.array_equal(a, b)]
    return out + (['bed'] if got[4] != want[4] else [])


def check(ps, case, failures, what, aligned=True, want=None, **how):
    want = case.expected()[1] if want is None else want
    n, cnt = parse_counted(ps, None if how else case.text, **how)
    got = ps.fetch(want_bed=True)
    bad = differences(got, want)
    plan = ptc.plan(case.text, aligned=aligned)
    if n != len(want[0]) or bad:
        failures.append('%s %s: %d lines (oracle %d), differ: %s' % (what, case.name, n, len(want[0]), bad))
    if any(cnt[k] != plan[k] for k in ptc.COUNTERS):
        failures.append('%s %s: counters %r, the plan says %r' % (what, case.name, cnt, {k: plan[k] for k in ptc.COUNTERS}))
    return cnt, plan


def line_of(exc):
    m = re.search(r'line (\d+)', str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


def test_every_case_equals_the_oracle_and_takes_the_planned_paths(parsers):
    """every valid case, host bytes in: the four arrays and the BED bytes equal the oracle's, the four counters equal plan(text)"""
    failures = []
    with tick('pairs_text_fuzz: corpus'):
        cases = ptc.cases('ok')
    with tick('pairs_text_fuzz: every case'):
        for c in cases:
            cnt, plan = check(parsers(c.names), c, failures, 'bytes')
            for k in ptc.COUNTERS:
                REACHED[k] += cnt[k]
            REACHED['bed_direct_text_staged'] += plan['bed_direct_text_staged']
    assert not failures, '\n'.join(failures[:40])
    assert {c.section for c in cases} == {name for name, _ in ptc.SECTIONS if name != 'errors'}


def _subset():
    """a few cases of every section and all of the block-structure ones"""
    pick = {'shift00', 'shift05', 'shift11', 'mixed', 'mixed_last_cr', 'crcrlf_no_final', 'cr_at_16k_minus_1', 'cr_at_4096k_minus_1', 'size_1_cr', 'size_15_cr',
            'size_16_crlf', 'size_17_none', 'size_4095_cr', 'size_4096_crlf', 'size_4097_lf', 'size_8192_none', 'accepted', 'table_of_0',
            'lengths_1_to_80_and_shared_prefixes'}
    out = [c for c in ptc.cases('ok') if c.name in pick or c.section == 'blocks']
    assert len(out) == len(pick) + len(ptc.section('blocks'))
    return out


def test_host_and_device_pointers_aligned_and_not(parsers):
    """the same arrays and BED bytes from a plain and a pinned host pointer, from a 16-byte aligned device tensor (the plan of an aligned
    buffer) and from views of it 1, 7, 8 and 15 bytes in: there every block goes to the HBM reader and the byte-wise line-break scan"""
    import torch
    failures = []
    with tick('pairs_text_fuzz: pointers'):
        for c in _subset():
            ps, n = parsers(c.names), len(c.text)
            host = np.array(np.frombuffer(c.text, np.uint8))
            check(ps, c, failures, 'host_ptr', host_ptr=host.ctypes.data, n_bytes=n)
            pinned = torch.from_numpy(host).pin_memory()
            check(ps, c, failures, 'pinned host_ptr', host_ptr=pinned.data_ptr(), n_bytes=n)
            dev = torch.empty(n + 16, dtype=torch.uint8, device='cuda:0')
            assert dev.data_ptr() % 16 == 0
            for shift in (0, 1, 7, 8, 15):
                dev[shift:shift + n].copy_(pinned)
                torch.cuda.synchronize()
                cnt, plan = check(ps, c, failures, 'device_ptr + %d' % shift, aligned=shift == 0, device_ptr=dev.data_ptr() + shift, n_bytes=n)
                if shift:
                    assert plan['text_blocks_staged'] == 0 and plan['text_blocks_direct'] == -(-(len(ptc.line_bounds(c.text)) - 1) // ptc.LN_BLOCK)
    assert not failures, '\n'.join(failures[:40])


def test_wide_mode():
    """set_wide: same ids and BED bytes, int64 positions; the int32 window is refused in narrow mode only, a literal beyond 2^40 in both"""
    narrow, wide = Parsers(), Parsers(wide=True)
    failures = []
    try:
        with tick('pairs_text_fuzz: wide'):
            for c in _subset():
                want = c.expected(wide=True)[1]
                assert want[1].dtype == np.int64 and want[4] == c.expected()[1][4]
                check(wide(c.names), c, failures, 'wide', want=want)
            cases = ptc.cases('range')
            assert len(cases) > 10 and any(c.refused_wide for c in cases) and not all(c.refused_wide for c in cases)
            for c in cases:
                with pytest.raises(ValueError, match='outside the int32 range') as e:
                    narrow(c.names).parse(c.text, want_bed=True)
                assert line_of(e) == c.bad_line, c
                ps = _lib.PairsParser(c.names)                       # a parser of its own: the line count starts at this text
                ps.set_wide(True)
                kind, want = c.expected(wide=True)
                try:
                    if c.refused_wide:
                        before = ps.parse(VALID)
                        with pytest.raises(ValueError, match=re.escape('beyond 2^40')) as e:
                            ps.parse(c.text, want_bed=True)
                        assert line_of(e) == before + c.bad_line, c
                    elif kind == 'raises':                           # accepted here, a later line is malformed
                        with pytest.raises(want):
                            ps.parse(c.text, want_bed=True)
                    else:
                        check(ps, c, failures, 'wide', want=want)
                finally:
                    ps.destroy()
        assert not failures, '\n'.join(failures[:40])
    finally:
        narrow.destroy()
        wide.destroy()


def _fetch_chunks(ps, text, cuts):
    rows, beds = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ps.parse(text[a:b], want_bed=True)
        out = ps.fetch(want_bed=True)
        rows.append(out[:4])
        beds.append(out[4])
    return [np.concatenate([r[k] for r in rows]) for k in range(4)] + [b''.join(beds)]


def test_chunks_of_whole_lines_and_buffer_reuse(parsers):
    """one parser throughout: a small text cut in two at every line boundary, a large one cut at random boundaries — the concatenated
    results equal the one-shot result; a large text, a small one, the large one again: the first answer (no stale buffer contents)"""
    rng = np.random.default_rng(7)
    by_name = {c.name: c for c in ptc.cases('ok')}
    with tick('pairs_text_fuzz: chunks'):
        for name in ('size_4097_crlf', 'mixed_no_final'):
            c = by_name[name]
            ps, want, bounds = parsers(c.names), c.expected()[1], ptc.line_bounds(c.text)
            assert len(bounds) > 40
            for cut in bounds[1:-1].tolist():
                assert not differences(_fetch_chunks(ps, c.text, [0, cut, len(c.text)]), want), (name, cut)
        for name in ('shift09', 'long_read_names', 'text_span_around_in_cap'):
            c = by_name[name]
            ps, want, bounds = parsers(c.names), c.expected()[1], ptc.line_bounds(c.text)
            for n_cuts in (1, 3, 9, 40):
                cuts = [0] + sorted(set(rng.choice(bounds[1:-1], n_cuts, replace=False).tolist())) + [len(c.text)]
                assert not differences(_fetch_chunks(ps, c.text, cuts), want), (name, cuts)
        large, small = by_name['bed_span_around_out_cap'], by_name['size_17_none']
        ps = parsers(large.names)
        for c in (large, small, large, by_name['one_30k_token_col1'], small, large):
            assert ps.parse(c.text, want_bed=True) == len(c.expected()[1][0])
            assert not differences(ps.fetch(want_bed=True), c.expected()[1]), c


def test_bed_through_a_byte_sink(parsers, tmp_path):
    """set_bed_sink on the two block-structure cases with the most BED bytes: the file holds the oracle's bytes"""
    cases = sorted(ptc.section('blocks'), key=lambda c: -len(c.expected()[1][4]))[:2]
    with tick('pairs_text_fuzz: sink'):
        for k, c in enumerate(cases):
            want = c.expected()[1]
            ps = parsers(c.names)
            path = str(tmp_path / ('sink%d.bed' % k))
            sink = _lib.ByteSink(path, expected_bytes=len(want[4]))
            try:
                ps.set_bed_sink(sink)
                for _ in range(2):                                   # two chunks into one file
                    assert ps.parse(c.text, want_bed=True) == len(want[0]) and ps.bed_bytes == len(want[4])
                    got = ps.fetch()
                    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
            finally:
                ps.set_bed_sink(None)
                sink.close()
            _lib.files_join()
            with open(path, 'rb') as f:
                assert f.read() == want[4] * 2, c


def test_malformed_lines_raise_what_the_reference_raises(parsers):
    """every error case: the exception type of the oracle call on the same bytes; the line number is that of the first offending line
    in file order, counted over everything the parser has parsed before; the parser then parses a valid text correctly"""
    cases = ptc.cases('error')
    assert len(cases) > 100 and {c.expected()[1] for c in cases} == {IndexError, ValueError}
    want_valid = orc.parse_pairs_text(VALID, ptc.BASE_NAMES)
    before = {}
    failures = []
    with tick('pairs_text_fuzz: errors'):
        for c in cases:
            kind, exc = c.expected()
            assert kind == 'raises'
            ps = parsers(c.names)
            seen = before.get(id(ps), 0)
            try:
                ps.parse(c.text, want_bed=bool(seen & 1))
                failures.append('%s: no exception (the reference: %s)' % (c.name, exc.__name__))
            except (IndexError, ValueError, RuntimeError) as e:
                m = re.search(r'line (\d+)', str(e))
                if type(e) is not exc:
                    failures.append('%s: %s("%s"), the reference raises %s' % (c.name, type(e).__name__, e, exc.__name__))
                elif not m or int(m.group(1)) != seen + c.bad_line:
                    failures.append('%s: "%s", the first offending line is %d (+ %d lines of earlier chunks)' % (c.name, e, c.bad_line, seen))
            n = ps.parse(VALID, want_bed=True)
            if n != len(want_valid[0]) or differences(ps.fetch(want_bed=True), want_valid):
                failures.append('%s: the parser is not usable after the exception' % c.name)
            before[id(ps)] = seen + n
    assert not failures, '\n'.join(failures[:40])


def test_malformed_line_through_the_generator(tmp_path, monkeypatch):
    """what the caller of cluster.pairs_generator_inter_ctgs sees: the file in small chunks, the reference's exception type, the line
    number counted from the top of the file"""
    from haphic_amd import cluster
    monkeypatch.chdir(tmp_path)
    by_name = {c.name: c for c in ptc.cases('error')}
    with tick('pairs_text_fuzz: generator'):
        for name, chunk in (('4col_bad_staged', 2048), ('4col_int_unstaged', 40_000), ('5col_fifth_then_4col_int_staged_blocks_1_2', 1024)):
            c = by_name[name]
            (tmp_path / 'in.pairs').write_bytes(c.text)
            aln = cluster.pairs_generator_inter_ctgs('in.pairs', 'pairs')
            aln.chunk_bytes = chunk                                   # the reader refuses a line longer than two chunks
            lines = 0
            with pytest.raises(c.expected()[1]) as e:
                for _parser, n in aln.batches(c.names):
                    lines += n
            assert line_of(e) == c.bad_line and lines < c.bad_line, (name, str(e.value), lines)
            cluster._lib.files_join()


def test_every_path_was_reached(parsers):
    """across the corpus each of the four counters was non-zero, and some block formatted its BED straight into HBM from LDS-staged
    text: a later change of IN_CAP / OUT_CAP cannot quietly turn the boundary cases into ordinary ones"""
    if not any(REACHED.values()):                                    # run on its own: the block-structure section is what reaches them
        failures = []
        for c in ptc.section('blocks'):
            cnt, plan = check(parsers(c.names), c, failures, 'bytes')
            for k in ptc.COUNTERS:
                REACHED[k] += cnt[k]
            REACHED['bed_direct_text_staged'] += plan['bed_direct_text_staged']
        assert not failures, '\n'.join(failures)
    print('pairs_text_fuzz: blocks by path', REACHED)
    assert all(v > 0 for v in REACHED.values()), REACHED
