"""tests/clm_write_cases.py without a GPU: every case reaches the seams it is named for (asserted from the host mirror of the writer, so that
an edit of the corpus cannot quietly turn a boundary case into an ordinary one), and the contract (oracle.ingest + oracle.clm_text) gives
the bytes the reference's own update_clm_dict / output_clm wrote (tests/golden/clm_write.npz)."""
import hashlib
import os

import numpy as np
import pytest

from tests import clm_write_cases as cw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clm_write.npz')


def _blocks(p):
    return [b for c in p['chunks'] for b in c.blocks]


@pytest.mark.parametrize('name', cw.CASE_NAMES)
def test_mirror_accounts_for_every_byte_of_the_contract(name):
    c = cw.case(name)
    for chunk in (None, 8, 1024):
        p = c.plan(chunk, 4096)
        assert p['n_bytes'] == len(c.text) == sum(p['pieces']) and p['n_lines'] == c.text.count(b'\n')
        assert all(0 < n <= 4096 for n in p['pieces'])
        at = 0
        for ch in p['chunks']:                                       # every chunk is whole lines, every line starts where the mirror says
            body = c.text[at:at + ch.B]
            assert body.endswith(b'\n') and body.count(b'\n') == 4 * (ch.kr1 - ch.kr0) == len(ch.line_starts)
            assert [b[0] for b in ch.blocks][1:] == [b[1] for b in ch.blocks][:-1] and ch.blocks[-1][1] == ch.B
            at += ch.B


def test_group_sizes_case():
    c = cw.case('group_sizes')
    assert [g[2] for g in c.kept] == [s for s in cw.GROUP_SIZES if s >= 2]                       # dict order is the order of the first read pairs
    assert sorted((np.diff(c.want['clm_ptr']) // 4).tolist()) == sorted(cw.GROUP_SIZES)
    keys = [(c.table.ctg_rank[a], c.table.ctg_rank[b]) for a, b, _c, _d in c.kept]
    assert keys != sorted(keys)                                                                # ... which is not key order
    assert {1, 2, 3, 63, 64, 65, 255, 256, 257, 1000} == set(cw.GROUP_SIZES) and len(c.want['full_i']) == len(cw.GROUP_SIZES)
    assert len(c.cuts) == 2 and len({len(p[0]) for p in c.pushes()}) == 3
    ch, = c.plan()['chunks']
    starts = set(e % cw.CW_T for e in ch.line_starts[1:])
    assert 0 in starts and cw.CW_T - 1 in starts                                               # a header on the first and on the last element of a block
    assert ch.E % cw.CW_T != 0 and ch.E > 10 * cw.CW_T
    sizes = {g[2] for g in c.kept}
    assert any(np.unique(d[0]).size < d.shape[1] for _a, _b, _c, d in c.kept)                  # equal distances inside a line
    assert {255, 256, 257} <= sizes                                                            # lines that straddle blocks, by one distance more or less


def test_digits_case():
    c = cw.case('digits')
    assert sorted(g[2] for g in c.kept) == list(cw.DIGIT_COUNTS)
    assert {len(str(2 * g[2])) for g in c.kept} == {1, 2, 3, 4} and {2 * g[2] for g in c.kept} >= {4, 8, 10, 98, 100, 998, 1000}
    per_line = [np.concatenate([g[3][n] for g in c.kept]) for n in range(4)]
    targets = cw.digit_targets()
    for n in range(4):
        assert set(targets[n]) <= set(per_line[n].tolist()), (n, sorted(set(targets[n]) - set(per_line[n].tolist())))
        assert len(targets[n]) >= len(cw.DIGIT_VALUES) - 2
    assert 0 in targets[2] and {9, 10, 99, 100, 10 ** 9 - 1, 10 ** 9} <= set(targets[0]) & set(targets[1]) & set(targets[2]) & set(targets[3])
    assert set(cw.n_digits(np.concatenate(per_line)).tolist()) == set(range(1, 11))
    assert any((np.diff(g[3], axis=1) == 0).any() for g in c.kept)


@pytest.mark.parametrize('name, max_len', [('longest_2p31m1', 2 ** 31 - 1), ('longest_2p20m1', 2 ** 20 - 1), ('longest_2p20', 2 ** 20)])
def test_longest_cases(name, max_len):
    c = cw.case(name)
    a, b, cnt, d = c.kept[0]
    assert c.lengths[a] == c.lengths[b] == max_len == c.lengths.max()
    assert d[1][-1] == 2 * max_len and d[2][0] == 0                                             # len_i + len_j from position 0, and distance 0
    assert d.max() == 2 * max_len == max(g[3].max() for g in c.kept)
    if max_len == 2 ** 31 - 1:
        assert d.max() > 2 ** 32 - 8 and len(str(d.max())) == 10 and b' 4294967294 4294967294\n' in c.text
    else:
        assert (2 * max_len).bit_length() == (21 if max_len == 2 ** 20 - 1 else 22)            # the two sides of bits_for(2 * max_ctg_len)
    pos = set(c.p1.tolist()) | set(c.p2.tolist())
    assert 0 in pos and max_len - 1 in pos


def test_phase_cases_run_through_every_residue():
    seen_b0, seen_b1 = set(), set()
    for name in cw.PHASE_NAMES:
        c = cw.case(name)
        ch, = c.plan()['chunks']
        assert c.kept[0][2] == 2 and len(ch.blocks) >= 5
        seen_b0.add(ch.blocks[1][0] & 15)
        seen_b1.add(ch.blocks[1][1] & 15)
    assert seen_b0 == set(range(16))
    every_b0 = {b[0] & 15 for n in cw.PHASE_NAMES for b in _blocks(cw.case(n).plan())}
    every_b1 = {b[1] & 15 for n in cw.PHASE_NAMES for b in _blocks(cw.case(n).plan())}
    assert every_b0 == every_b1 == set(range(16))                                              # both ragged ends of the 16-byte copy-out


def test_direct_case():
    c = cw.case('direct')
    ch, = c.plan()['chunks']
    spans = [b[2] for b in ch.blocks]
    assert spans[cw.DIRECT_BLOCK_AT_CAP] == cw.CW_OUT_CAP == 24576 and spans[cw.DIRECT_BLOCK_OVER_CAP] == cw.CW_OUT_CAP + 1 == 24577
    direct = [s > cw.CW_OUT_CAP for s in spans]
    assert ch.direct == sum(direct) >= 4 and len(spans) - ch.direct >= 4
    assert any(direct[k] and direct[k + 1] and direct[k + 2] for k in range(len(direct) - 2))   # several consecutive blocks
    assert direct[0] is False and direct[-1] is False and True in direct                        # staged, direct and staged again in one chunk
    long_names = [len(n) for n in c.names if len(n) >= 100]
    assert long_names and min(long_names) >= 100 and max(long_names) <= 300 and max(long_names) > 250
    assert {g[2] for g in c.kept} == {2, 3} and sum(g[2] == 2 for g in c.kept) > 0.9 * len(c.kept)


def test_short_names_and_nothing_kept_cases():
    c = cw.case('short_names_E40')
    assert all(len(n) == 1 for n in c.names) and c.plan()['chunks'][0].E == 40 < cw.CW_T
    assert c.text.startswith(b'%s+ %s+\t' % tuple(c.names[k].encode() for k in c.kept[0][:2]))
    assert len(c.text.split(b'\t')[0]) == 5
    c = cw.case('short_names_E256')
    ch, = c.plan()['chunks']
    assert ch.E == cw.CW_T and len(ch.blocks) == 1 and len(c.want['full_i']) == len(c.kept) + 1
    c = cw.case('nothing_kept')
    assert c.text == b'' and c.kept == [] and len(c.want['full_i']) == 50 and cw.counters(c.plan()) == dict.fromkeys(cw.COUNTERS, 0)
    c = cw.case('one_kept_among_thousands')
    assert len(c.kept) == 1 and c.kept[0][2] == 2 and len(c.want['full_i']) == 3000 and c.text.count(b'\n') == 4
    k = [int(x) for x in np.flatnonzero(np.diff(c.want['clm_ptr']) >= 8)]
    assert k == [1500]


def test_random_case():
    c = cw.case('random')
    assert len(c.id1) == 20_000 and len(c.names) == 40 and len({len(n) for n in c.names}) >= 5
    sizes = [g[2] for g in c.kept]
    assert min(np.diff(c.want['clm_ptr'])) == 4 and min(sizes) == 2 and max(sizes) > 200         # skipped, smallest kept, heavy groups
    assert c.plan()['chunks'][0].E % cw.CW_T != 0


@pytest.mark.parametrize('name', cw.CHUNK_SWEEP_CASES)
def test_chunk_settings_reach_the_cut_rules(name):
    """over the "clm_chunk" settings of the GPU sweep: three chunks or more at every setting but the default, at the proven value a cut on
    upper_bound's equality behind several contig pairs, and somewhere a contig pair larger than the chunk (the at-least-one rule)"""
    c = cw.case(name)
    settings = cw.chunk_settings(name)
    assert settings[:3] == (4, 8, 1024) and settings[4] is None and settings[3] not in (4, 8, 1024, None)
    plans = {v: c.plan(v) for v in settings}
    assert plans[None]['n_chunks'] == 1
    for v in settings[:4]:
        assert plans[v]['n_chunks'] >= 3, (v, plans[v]['n_chunks'])
        assert sum(ch.kr1 - ch.kr0 for ch in plans[v]['chunks']) == len(c.kept)
        for ch in plans[v]['chunks']:                                # the rule itself
            n = sum(g[2] for g in c.kept[ch.kr0:ch.kr1])
            assert (ch.oversize and ch.kr1 == ch.kr0 + 1 and n > v // 4) or (not ch.oversize and n <= v // 4)
            assert ch.equality == (n == v // 4)
            if not ch.oversize and ch.kr1 < len(c.kept):
                assert n + c.kept[ch.kr1][2] > v // 4                # as many whole pairs as fit
    eq = plans[settings[3]]
    assert any(ch.equality and ch.kr1 - ch.kr0 >= 2 for ch in eq['chunks'])
    assert any(ch.oversize for v in settings[:4] for ch in plans[v]['chunks'])
    assert all(ch.oversize for ch in plans[4]['chunks'])            # one read pair per chunk: every kept contig pair is larger
    assert any(ch.equality for ch in plans[8]['chunks'])            # a contig pair of exactly two read pairs
    if name != 'direct':                                             # (its contig pairs have two or three read pairs)
        assert any(ch.oversize for ch in eq['chunks']) and any(ch.oversize for ch in plans[1024]['chunks'])
    # the number of line bits differs between the chunks of one file
    assert len({(4 * (ch.kr1 - ch.kr0)).bit_length() for ch in plans[1024]['chunks']}) >= 2 or name == 'direct'


@pytest.mark.parametrize('name', cw.PIECE_SWEEP_CASES)
def test_piece_settings_reach_the_sink_seams(name):
    c = cw.case(name)
    settings = cw.piece_settings(name)
    n = len(c.text)
    assert settings == (4096, 12288, n, None) and 4096 * 20 < n < cw.PIECE
    p = c.plan(None, 4096)
    assert len(p['pieces']) > 20 > cw.NBUF and p['pieces'][-1] == n % 4096 != 0
    cut = np.cumsum(p['pieces'])[:-1]
    assert any(c.text[k - 1:k] != b'\n' for k in cut.tolist())      # a piece boundary inside a line
    assert c.plan(None, n)['pieces'] == [n]                          # n == piece exactly
    assert c.plan(None, n - 1)['pieces'] == [n - 1, 1]
    assert c.plan()['pieces'] == [n]
    both = [ch.B for ch in c.plan(1024)['chunks']]
    assert max(both) > 12288                                         # with "clm_chunk" 1024 a chunk's text is longer than a piece
    if name == 'random':                                             # ... and shorter (every chunk of 'direct' is longer)
        assert min(both) < 12288 and min(both) % 4096 != 0


def test_refused_cases():
    for name in cw.REFUSED_NAMES:
        c = cw.case(name)
        beyond = (c.p1 >= c.lengths[c.id1]).sum() + (c.p2 >= c.lengths[c.id2]).sum()
        assert beyond == (2 if name == 'beyond_negative' else 1)
        assert ((c.p1 == c.lengths[c.id1]) | (c.p2 == c.lengths[c.id2])).sum() == 1
        assert (b' -898 -898 ' in c.text or b'\t-898 -898 ' in c.text) == (name == 'beyond_negative')
        assert (min(g[3].min() for g in c.kept) < 0) == (name == 'beyond_negative')


def test_contract_equals_the_reference_files():
    """oracle.clm_text on oracle.ingest's arrays == paired_links.clm as the reference's update_clm_dict + output_clm wrote it, and the fixture
    was made from the inputs the corpus generates today"""
    z = np.load(GOLDEN)
    gold = cw.golden_outputs(z)
    assert tuple(gold) == cw.GOLDEN_CASES
    for k, name in enumerate(cw.GOLDEN_CASES):
        c = cw.case(name)
        lo, hi = int(z['name_off'][k]), int(z['name_off'][k + 1])
        assert [str(n) for n in z['names'][lo:hi]] == c.names and np.array_equal(z['lengths'][lo:hi], c.lengths), name
        lo, hi = int(z['pair_off'][k]), int(z['pair_off'][k + 1])
        assert np.array_equal(z['pairs'][lo:hi], np.stack([c.id1, c.p1, c.id2, c.p2], axis=1)), name
        assert tuple(z['cuts'][int(z['cut_off'][k]):int(z['cut_off'][k + 1])].tolist()) == c.cuts, name
        n, sha, text = gold[name]
        assert (text is None) == (n > cw.GOLDEN_TEXT_MAX)
        assert len(c.text) == n and hashlib.sha256(c.text).hexdigest() == sha, name
        if text is not None:
            assert c.text == text, name
    assert sum(1 for v in gold.values() if v[2] is not None) >= 20
    assert os.path.getsize(GOLDEN) < 1_000_000
