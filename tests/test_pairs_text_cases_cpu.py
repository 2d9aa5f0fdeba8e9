"""The corpus of tests/pairs_text_cases.py is itself checked here, without a GPU: it is deterministic and inside the tokeniser's stated
domain, the block plan agrees with hand-computed splits, and — where the reference checkout is present — the reference's own
pairs_generator / pairs_generator_inter_ctgs, run live on every case written to a file, yield the oracle's rows, write the oracle's
alignments.bed and raise the oracle's exception type.  That ties oracle.parse_pairs_text on the new inputs to the reference."""
import os

import numpy as np
import pytest

from tests import oracle_lib
from tests import pairs_text_cases as ptc
from tests.test_reference_run_integration import REF, _load_reference


def test_corpus_is_deterministic_and_in_domain():
    total = 0
    for name, build in ptc.SECTIONS:
        a, b = list(build()), list(build())
        assert [(c.name, c.kind, c.bad_line, c.names, c.text) for c in a] == [(c.name, c.kind, c.bad_line, c.names, c.text) for c in b], name
        assert [c.name for c in a] == [c.name for c in ptc.section(name)] and all(ptc.in_domain(c.text) for c in a)
        assert len({c.name for c in a}) == len(a) >= 4
        total += len(a)
    assert total == len(ptc.cases())
    # the domain check has teeth
    for bad in ('r1\tA\x855\tB\t7\n', 'r1\tA\xa0\t5\tB\t7\n', 'r\u3000A 5 B 7\n', 'r\u2028A 5 B 7\n', 'r A 5 B \u0667\n', 'r A \uff15 B 7\n'):
        assert not ptc.in_domain(bad.encode())
    with pytest.raises(UnicodeDecodeError):
        ptc.in_domain(b'r\xff A 5 B 7\n')
    assert ptc.in_domain('Ņ\tŠ\t5\tŜ\t7\n'.encode())


def test_expectations_come_from_the_oracle_and_name_the_first_bad_line():
    kinds = {}
    for c in ptc.cases():
        kind, want = c.expected()
        kinds.setdefault(c.kind, []).append(c)
        if c.kind == 'ok':
            assert kind == 'ok' and len(want[0]) == len(ptc.line_bounds(c.text)) - 1, c
            assert ptc.first_bad_line(c.text, c.names) is None if len(c.text) < 50_000 else True
        elif c.kind == 'error':
            assert kind == 'raises' and ptc.first_bad_line(c.text, c.names) == c.bad_line, c
        else:                                                        # the oracle accepts the line the device path refuses
            b = ptc.line_bounds(c.text)
            line = c.text[b[c.bad_line - 1]:b[c.bad_line]]
            pos = ptc.orc.parse_pairs_text(line, c.names, wide=True)
            assert max(abs(int(pos[1][0])), abs(int(pos[3][0]))) > 2**31 - 2, c
            assert ptc.first_bad_line(c.text[:b[c.bad_line - 1]], c.names) is None, c
    assert len(kinds['ok']) > 60 and len(kinds['error']) > 100 and len(kinds['range']) > 10
    assert {c.expected()[1] for c in kinds['error']} == {IndexError, ValueError}


def _line(read_bytes):
    return b'r' * read_bytes + b'\tA\t5\tB\t7\n'                     # read_bytes + 9 bytes of text, 2 * read_bytes + 30 of BED


def test_plan_on_hand_built_spans():
    zero = dict.fromkeys(ptc.COUNTERS + ('bed_direct_text_staged',), 0)
    assert (ptc.LN_BLOCK, ptc.IN_CAP, ptc.OUT_CAP, ptc.TX_BLOCK) == (128, 24576, 36864, 4096)
    assert ptc.plan(b'') == zero
    # 128 lines of 192 bytes: a span of exactly IN_CAP stages; BED 128 * 396 bytes > OUT_CAP leaves directly
    text = _line(183) * 128
    assert len(text) == ptc.IN_CAP
    assert ptc.plan(text) == dict(zero, text_blocks_staged=1, bed_blocks_direct=1, bed_direct_text_staged=1)
    assert ptc.plan(text, want_bed=False) == dict(zero, text_blocks_staged=1)
    assert ptc.plan(text, aligned=False) == dict(zero, text_blocks_direct=1, bed_blocks_direct=1)
    assert ptc.plan(_line(183) * 127 + _line(184)) == dict(zero, text_blocks_direct=1, bed_blocks_direct=1)          # one byte more
    assert ptc.plan(text + _line(1)) == dict(zero, text_blocks_staged=2, bed_blocks_direct=1, bed_blocks_lds=1, bed_direct_text_staged=1)   # a 129th line: a block of its own
    # the second block starts at byte 12809: its span counts from 12800
    first = _line(91) * 127 + _line(100)
    assert len(first) == 12809
    for last, staged in ((183 - 9, True), (183 - 8, False)):
        p = ptc.plan(first + _line(183) * 127 + _line(last))
        assert (p['text_blocks_staged'], p['text_blocks_direct']) == (1 + staged, 1 - staged), (last, p)
    # BED: 128 lines of 2 * 129 + 30 = 288 bytes are exactly OUT_CAP; a comment-only block writes nothing and counts in neither
    text = _line(129) * 128
    assert ptc.bed_lengths(text).tolist() == [288] * 128
    assert ptc.plan(text) == dict(zero, text_blocks_staged=1, bed_blocks_lds=1)
    assert ptc.plan(_line(129) * 127 + b'r' * 129 + b'\tuu\t5\tB\t7\n') == dict(zero, text_blocks_staged=1, bed_blocks_direct=1, bed_direct_text_staged=1)
    assert ptc.plan(b'#c\n' * 128 + text) == dict(zero, text_blocks_staged=2, bed_blocks_lds=1)
    # behind a block of 36879 BED bytes the next one starts at offset 15 mod 16: OUT_CAP - 15 bytes still fit, one more does not
    head = _line(129) * 127 + b'r' * 136 + b'\tuu\t5\tB\t7\n'
    assert int(ptc.bed_lengths(head).sum()) == ptc.OUT_CAP + 15
    for last, lds in ((129 - 8, True), (129 - 7, False)):
        p = ptc.plan(head + _line(129) * 127 + b'r' * last + b'\tuu\t5\tB\t7\n')
        assert (p['bed_blocks_lds'], p['bed_blocks_direct']) == (int(lds), 2 - int(lds)), (last, p)
    # line ends as universal newlines cut them
    assert ptc.line_bounds(b'a\r\nb\rc\n\rd\r\r\ne').tolist() == [0, 3, 5, 7, 8, 10, 12, 13]
    assert ptc.line_bounds(b'a\r').tolist() == [0, 2] and ptc.line_bounds(b'\n').tolist() == [0, 1] and ptc.line_bounds(b'a').tolist() == [0, 1]


def test_plan_of_the_boundary_cases():
    """the block-structure cases sit where they were built to sit"""
    by_name = {c.name: c for c in ptc.section('blocks')}
    p = ptc.plan(by_name['text_span_around_in_cap'].text)
    assert (p['text_blocks_staged'], p['text_blocks_direct']) == (sum(d <= 0 for d in ptc.IN_CAP_DELTAS) + 1, sum(d > 0 for d in ptc.IN_CAP_DELTAS))
    p = ptc.plan(by_name['bed_span_around_out_cap'].text)
    assert (p['bed_blocks_lds'], p['bed_blocks_direct']) == (sum(d <= 0 for d in ptc.OUT_CAP_DELTAS), sum(d > 0 for d in ptc.OUT_CAP_DELTAS))
    assert p['text_blocks_direct'] == 0 and p['bed_direct_text_staged'] == p['bed_blocks_direct']
    assert ptc.plan(by_name['long_read_names'].text)['bed_direct_text_staged'] >= 4
    for col in (0, 1, 3):
        assert ptc.plan(by_name['one_30k_token_col%d' % col].text)['text_blocks_direct'] == 1
    assert ptc.plan(by_name['last_block_of_1'].text)['text_blocks_staged'] == 2 and len(ptc.line_bounds(by_name['last_block_of_127'].text)) - 1 == 255


def _bed_tuples(bed):
    """(ref, mref, pos, mpos) of every pair of records of the oracle's BED bytes (tokens hold no whitespace)"""
    rec = [r.split('\t') for r in bed.decode('utf-8').split('\n')[:-1]]
    assert len(rec) % 2 == 0 and all(len(r) == 6 and r[1] == r[2] for r in rec)
    return [(a[0], b[0], int(a[1]), int(b[1])) for a, b in zip(rec[0::2], rec[1::2])]


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_reference_generators_agree_with_the_oracle_on_every_case(tmp_path, monkeypatch):
    H = _load_reference()
    monkeypatch.chdir(tmp_path)
    n_rows = 0
    for c in ptc.cases():
        with open('in.pairs', 'wb') as f:
            f.write(c.text)
        kind, want = c.expected(wide=True)
        for gen, inter in ((H.pairs_generator, False), (H.pairs_generator_inter_ctgs, True)):
            if kind == 'raises':
                with pytest.raises(want):
                    list(gen('in.pairs', 'pairs'))
                continue
            got = list(gen('in.pairs', 'pairs'))
            with open('alignments.bed', 'rb') as f:
                assert f.read() == want[4], c
            tuples = _bed_tuples(want[4])
            cid = {n: i for i, n in enumerate(c.names)}
            data = ptc.bed_lengths(c.text) > 0
            assert [(cid.get(a, -1), x, cid.get(b, -1), y) for a, b, x, y in tuples] == list(zip(*[want[k][data].tolist() for k in range(4)])), c
            assert got == [t for t in tuples if not inter or t[0] != t[1]], c
            n_rows += len(got)
    assert n_rows > 20_000


@pytest.fixture
def host_only(monkeypatch):
    from haphic_amd import cluster
    monkeypatch.setattr(cluster, '_lib', oracle_lib)
    return cluster


@pytest.mark.parametrize('name', ['shift03', 'mixed'])
def test_chunked_front_end_on_the_stand_in(host_only, tmp_path, monkeypatch, name):
    """cluster.pairs_generator* over small chunks with tests/oracle_lib standing in for the library: the batches, concatenated, are the
    one-shot rows and alignments.bed holds the one-shot bytes"""
    c = {c.name: c for c in ptc.cases('ok')}[name]
    monkeypatch.chdir(tmp_path)
    with open('in.pairs', 'wb') as f:
        f.write(c.text)
    want = c.expected()[1]
    for gen in (host_only.pairs_generator, host_only.pairs_generator_inter_ctgs):
        aln = gen('in.pairs', 'pairs')
        aln.chunk_bytes = 1500
        rows = [parser.fetch()[:4] for parser, _n in aln.batches(c.names)]
        assert len(rows) > 5 and aln.stats['chunks'] == len(rows)
        assert all(np.array_equal(np.concatenate([r[k] for r in rows]), want[k]) for k in range(4))
        with open('alignments.bed', 'rb') as f:
            assert f.read() == want[4]
