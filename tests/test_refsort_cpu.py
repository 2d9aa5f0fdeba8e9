"""`haphic refsort` without a GPU: the mirrors of haphic_amd/refsort.py over the numpy engine of tests/refsort_cases.py against what the reference's
own functions gave (tests/golden/refsort.npz), every hand-back condition, the interval stand-in and the command line."""
import io
import os
import types

import numpy as np
import pytest

from haphic_amd import containers, intervals, refsort, scaffolds
from tests import refsort_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/scripts'
Z = np.load(os.path.join(HERE, 'golden', 'refsort.npz'))
GOLDEN = rc.golden(Z)
CASES = rc.cases()
SERVED = [c for c in CASES if c.served]
ENGINE = rc.NumpyEngine


def test_the_fixture_was_made_from_these_cases():
    inputs = rc.golden_inputs(Z)
    assert list(inputs) == [c.name for c in CASES] == list(GOLDEN)
    for c in CASES:
        assert inputs[c.name] == [c.agp.decode(), c.paf.decode(), None if c.fasta is None else c.fasta.decode()], c.name
    want = {'both orientations': 'both_orientations', 'tie': 'sum_tie', 'empty class': 'empty_forward_class', 'failure': 'alignment_check_fails'}
    assert GOLDEN[want['tie']]['log'][1] == 'group: g\tforward LIS: 101\treverse LIS: 101' and GOLDEN[want['tie']]['log'][2] == 'chr1: g -'
    assert 'forward LIS: 0\t' in GOLDEN[want['empty class']]['log'][1] and GOLDEN[want['failure']]['raises'] == 'Exception'
    assert '>hole\n>c8\n' in GOLDEN['empty_record']['fa']


@pytest.mark.parametrize('source', ['path', 'bytes'])
@pytest.mark.parametrize('case', SERVED, ids=repr)
def test_mirrors_give_the_reference_results(case, source, tmp_path):
    refsort.STATS.clear()
    rec = rc.run_mirrors(case, str(tmp_path), ENGINE, refsort, scaffolds, paf_source=source)
    assert rec == GOLDEN[case.name]
    assert refsort.STATS['parse_paf'] == 'device'                # none of these may be handed back (no original is bound: it would raise, too)
    if not rec['raises']:
        assert refsort.STATS['order_and_orient_groups'] == 'device'


def test_python_types_and_container_of_parse_paf(tmp_path):
    case = next(c for c in CASES if c.name == 'contig_in_two_groups')
    args = case.write(str(tmp_path))
    ctg_group = rc.parse_agp(args.agp, args.min_ctg_len)[0]
    d = refsort.parse_paf(args.paf, ctg_group, args.aln_len_cutoff, _engine=ENGINE, _logger=rc.ListLogger())
    assert isinstance(d, refsort.PafGroups) and d.default_factory is dict and 'nowhere' not in d
    alns, total = d['group2']['chr1']
    assert type(total) is int and all(type(a) is tuple and [type(x) for x in a] == [str, int, float, float, int] for a in alns)
    assert d == {g: {r: [[tuple(a) for a in alns], total] for r, alns, total in refs} for g, refs in GOLDEN[case.name]['paf']}
    log = rc.ListLogger()
    refsort.parse_paf(args.paf, ctg_group, args.aln_len_cutoff, _engine=ENGINE, _logger=log)
    assert log.lines == ['Parsing input PAF file...']


# ------------------------------------------------------------------ what is handed back
def _job(tmp_path, name='both_orientations'):
    case = next(c for c in CASES if c.name == name)
    args = case.write(str(tmp_path))
    ctg_group, group_lines, group_len, solo = rc.parse_agp(args.agp, args.min_ctg_len)
    group_ref = refsort.parse_paf(args.paf, ctg_group, args.aln_len_cutoff, _engine=ENGINE, _logger=rc.ListLogger())
    fa_dict = scaffolds.parse_fasta(args.fasta, _engine=ENGINE.Fasta, logger=rc.ListLogger())
    return args, [ctg_group, group_ref, group_lines, group_len, solo, args], fa_dict


def _handed_back(positional, fa_dict, fout, engine=ENGINE, capsys=None):
    """-> True when the call reached `_original` whole: with the same arguments, nothing logged, nothing printed"""
    seen, log = [], rc.ListLogger()

    def original(*a):
        seen.append(a)
        return 'theirs'
    refsort.STATS.clear()
    got = refsort.order_and_orient_groups(*positional, fa_dict, fout, _original=original, _engine=engine, _logger=log)
    if got != 'theirs':
        return False
    assert len(seen) == 1 and all(x is y for x, y in zip(seen[0], list(positional) + [fa_dict, fout])) and not log.lines
    assert refsort.STATS['order_and_orient_groups'] == 'reference'
    if capsys is not None:
        assert capsys.readouterr().out == ''
    return True


def test_order_and_orient_hands_back_whole(tmp_path, capsys):
    args, pos, fa_dict = _job(tmp_path)
    out = str(tmp_path / 'out.fa')
    with open(out, 'w') as fout:
        assert not _handed_back(pos, fa_dict, fout)              # the job itself is served ...
    assert open(out).read() == GOLDEN['both_orientations']['fa'] and capsys.readouterr().out == GOLDEN['both_orientations']['stdout']
    with open(out, 'w') as fout:
        assert _handed_back(pos, {'c0': ['ACGT', 4, 1]}, fout, capsys=capsys)          # no FastaTable
        thawed = scaffolds.parse_fasta(args.fasta, _engine=ENGINE.Fasta, logger=rc.ListLogger())
        thawed['c0']
        assert not thawed.frozen and _handed_back(pos, thawed, fout, capsys=capsys)    # a thawed one
        assert _handed_back(pos, fa_dict, io.StringIO(), capsys=capsys)                # fout without a name
        assert _handed_back(pos, fa_dict, types.SimpleNamespace(name=3, write=None, flush=None), capsys=capsys)
        for width in (0, -2):
            pos[5] = types.SimpleNamespace(**dict(vars(args), max_width=width))
            assert _handed_back(pos, fa_dict, fout, capsys=capsys)
        pos[5] = args
        small = types.SimpleNamespace(**dict(vars(ENGINE), lis_sums=lambda p, v, w: rc.lis_sums(p, v, w, max_n=2)))       # a sequence beyond the LIS limit
        assert _handed_back(pos, fa_dict, fout, engine=small, capsys=capsys)
        for bad in ({'group1': {'chr1': [[('c0', 101.0, 60.0, 1050.0, 1)], 101]}},                          # a length that is no int
                    {'group1': {'chr1': [[('c0', 101, 60.0, 1050.0)], 101]}},                               # a short tuple
                    {'group1': {'chr1': [[('c0', 101, 60.25, 1050.0, 1)], 101]}},                           # a mid that is no multiple of 0.5
                    {'group1': {'chr1': [[('c0', 0, 60.0, 1050.0, 1)], 0]}},                                # a weight of 0
                    {'group1': {'chr1': [[('c0', 101, 60.0, 1050.0, 2)], 101]}},                            # the reference's assertion :234
                    {'group1': {'chr1': 7}}):
            pos[1] = bad
            assert _handed_back(pos, fa_dict, fout, capsys=capsys), bad
    assert open(out).read() == ''                                # none of them touched the file


@pytest.mark.parametrize('line, why', [('g\t1\t51\t1\tW\tc0\t250\t400\t+\n', 'end beyond the contig'), ('g\t1\t51\t1\tW\tc0\t0\t50\t+\n', 'start 0'),
                                       ('g\t1\t51\t1\tW\tc0\t60\t50\t+\n', 'start beyond end'), ('g\t1\t51\t1\tW\tnope\t1\t50\t+\n', 'no such contig'),
                                       ('g\t1\t51\t1\tW\tc0\t1\t50\t?\n', 'no orientation'), ('g\t1\t51\t1\tW\tc0\t1\t50\n', 'eight fields'),
                                       ('g\t1\t0\t1\tU\t-5\tscaffold\tyes\tproximity_ligation\n', 'negative N count'),
                                       ('g\t1\t0\t1\tU\tmany\tscaffold\tyes\tproximity_ligation\n', 'no N count')])
def test_agp_lines_python_decides_are_handed_back(line, why, tmp_path, capsys):
    args, pos, fa_dict = _job(tmp_path)
    for group in ('group1', 'group2', 'c8'):                     # a forward group, a reversed one, an unanchored one
        lines = dict(pos[2])
        lines[group] = lines[group] + [line.replace('g\t', group + '\t', 1)]
        with open(str(tmp_path / 'out.fa'), 'w') as fout:
            assert _handed_back(pos[:2] + [lines] + pos[3:], fa_dict, fout, capsys=capsys), (why, group)
    if why not in ('eight fields', 'no orientation', 'no N count'):                      # without --fasta nothing is sliced: served
        lines = dict(pos[2])
        lines['c8'] = lines['c8'] + [line.replace('g\t', 'c8\t', 1)]
        assert not _handed_back(pos[:2] + [lines] + pos[3:], None, None)
        assert capsys.readouterr().out.endswith(line.replace('g\t', 'c8\t', 1))


def test_parse_paf_hands_back_what_the_reader_refuses(tmp_path):
    args, pos, _fa = _job(tmp_path)
    good = next(c for c in CASES if c.name == 'both_orientations').paf
    line = good.split(b'\n')[0]
    refused = {'eleven fields': good + b'\t'.join(line.split(b'\t')[:11]) + b'\n', 'a sign': good.replace(b'\t10\t', b'\t+10\t', 1),
               'an underscore': good.replace(b'\t110\t', b'\t1_10\t', 1), '19 digits': good.replace(b'\t1000\t', b'\t' + b'1' * 19 + b'\t', 1),
               'a high byte': good + b'# caf\xc3\xa9\n', 'a long name': good.replace(b'chr1', b'c' * 256, 1),
               '2^52': good.replace(b'\t1000\t', b'\t%d\t' % (1 << 52), 1)}
    for why, text in refused.items():
        seen, log = [], rc.ListLogger()
        refsort.STATS.clear()
        got = refsort.parse_paf(text, pos[0], args.aln_len_cutoff, _original=lambda *a: seen.append(a) or 'theirs', _engine=ENGINE, _logger=log)
        assert got == 'theirs' and seen == [(text, pos[0], args.aln_len_cutoff)] and not log.lines and refsort.STATS['parse_paf'] == 'reference', why
        with pytest.raises((ENGINE.Paf.Unsupported, refsort._HandBack)):
            refsort.parse_paf(text, pos[0], args.aln_len_cutoff, _engine=ENGINE, _logger=log)
    with pytest.raises(ENGINE.Paf.Unsupported):
        ENGINE.Paf(str(tmp_path))                                # no regular file

    def raising(*a):
        raise IndexError('list index out of range')
    with pytest.raises(IndexError):                              # the reference's exception is the caller's
        refsort.parse_paf(refused['eleven fields'], pos[0], args.aln_len_cutoff, _original=raising, _engine=ENGINE)
    accepted = good.replace(b'\t1000\t', b'\t' + b'9' * 18 + b'\t', 1) + b'c0\t1\t1\t1\t+\tc0\t1\t1\t1\t1\t1\t00 \n'       # 18 digits; one name on both sides
    tab = ENGINE.Paf(accepted)
    assert tab.target_start[0] == 10 ** 18 - 1 and tab.query[-1] == tab.target[-1] == 0 and tab.mapq[-1] == 0


@pytest.mark.parametrize('case', [c for c in CASES if not c.served], ids=repr)
def test_handed_back_cases_give_the_reference_results(case, tmp_path):
    """with the reference's functions behind the mirrors (restated here where the checkout is absent: parse_paf :81-134 per line)"""
    def their_paf(paf, ctg_group_dict, cutoff):
        out = {}
        with open(paf) as f:
            for line in f:
                if not line.strip():
                    continue
                cols = line.split()
                if int(cols[11]) < 1 or int(cols[3]) - int(cols[2]) < cutoff or not ctg_group_dict.get(cols[0]):
                    continue
                s, e, rs, re_ = int(cols[2]), int(cols[3]), int(cols[7]), int(cols[8])
                groups = ctg_group_dict[cols[0]]
                group = groups[0][0] if len(groups) == 1 else refsort._max_ovl_group(groups, s, e)
                slot = out.setdefault(group, {}).setdefault(cols[5], [[], 0])
                slot[0].append((cols[0], e - s + 1, (e - s) / 2 + s, (re_ - rs) / 2 + rs, 1 if cols[4] == '+' else -1))
                slot[1] += e - s + 1
        return out

    calls = []

    def their_order(*a):                                         # (the reference's own runs behind the seams: the test below, where the checkout is)
        calls.append(a)
    refsort.STATS.clear()
    rec = rc.run_mirrors(case, str(tmp_path), ENGINE, refsort, scaffolds, originals={'parse_paf': their_paf, 'order_and_orient_groups': their_order})
    want = GOLDEN[case.name]
    assert rec['raises'] == want['raises'] and rec['paf'] == want['paf']
    if case.name == 'handback/slice_beyond_the_contig':          # parse_paf is served, the slice is Python's to cut
        assert refsort.STATS == {'parse_paf': 'device', 'order_and_orient_groups': 'reference'} and len(calls) == 1
        assert (rec['stdout'], rec['log'], rec['fa']) == ('', [], '')
    else:                                                        # parse_paf is the reference's, what follows is served on its dict
        assert refsort.STATS['parse_paf'] == 'reference' and not calls
        if not want['raises']:
            assert (rec['stdout'], rec['log'], rec['fa']) == (want['stdout'], want['log'], want['fa'])
            assert refsort.STATS['order_and_orient_groups'] == 'device'


# ------------------------------------------------------------------ the engine's two restatements against each other
def test_lis_restatement_on_small_sequences():
    rng = np.random.default_rng(3)
    assert rc.lis_sums([0, 0], [], []) == ([0], [0])
    f, r = rc.lis_sums([0, 3, 3, 7], [2, 4, 6, -6, -4, 0, 2], [5, 6, 7, 1, 2, 3, 4])
    assert f.tolist() == [18, 0, 7] and r.tolist() == [0, 0, 6]              # 0 belongs to both classes
    f, r = rc.lis_sums([0, 4], [2, 6, 2, 4], [5, 1, 50, 3])                    # a repeat is dropped, the first keeps its weight
    assert f.tolist() == [8]
    for _ in range(20):
        n = int(rng.integers(1, 12))
        v, w = rng.integers(-4, 5, n), rng.integers(1, 9, n)
        best = {True: 0, False: 0}
        for fwd in (True, False):                                # every subset, the slow way
            seen, keep = set(), []
            for x, y in zip(v.tolist(), w.tolist()):
                if (x < 0 if fwd else x > 0) or x in seen:
                    continue
                seen.add(x)
                keep.append((x, y))
            for mask in range(1 << len(keep)):
                sub = [keep[k] for k in range(len(keep)) if mask >> k & 1]
                if all(a[0] < b[0] for a, b in zip(sub, sub[1:])):
                    best[fwd] = max(best[fwd], sum(y for _x, y in sub))
        f, r = rc.lis_sums([0, n], v, w)
        assert (int(f[0]), int(r[0])) == (best[True], best[False])
    with pytest.raises(rc.LisUnsupported):
        rc.lis_sums([0, 1], [1], [0])


def test_interval_stand_in():
    closed = intervals.closed
    a = closed(10, 20) & closed(15, 30)
    assert (a.lower, a.upper, a.empty) == (15, 20, False) and 15 in a and 20.0 in a and 20.5 not in a
    assert (closed(1, 5) & closed(6, 9)).empty and (closed(5, 1) & closed(0, 9)).empty and 3 not in closed(5, 1)
    assert (closed(1, 5) & closed(5, 9)).upper - (closed(1, 5) & closed(5, 9)).lower + 1 == 1
    for s, e in ((1, 150), (151, 300), (40, 30)):                # get_max_ovl_group :67-78 through it == the integer form of the mirror
        groups = [('a', 1, 150, 0, 0, 1), ('b', 151, 300, 0, 0, 1)]
        best, best_len = None, -1
        for g, c0, c1, *_ in groups:
            ovl = closed(c0, c1) & closed(s, e)
            n = 0 if ovl.empty else ovl.upper - ovl.lower + 1
            if n > best_len:
                best, best_len = g, n
        assert best == refsort._max_ovl_group(groups, s, e)


# ------------------------------------------------------------------ the reference's run() around the mirrors
@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
def test_reference_functions_with_and_without_the_seams(tmp_path):
    from haphic_amd import patch
    from tests.golden.make_golden_refsort import load_reference_refsort
    F = load_reference_refsort(REF, '_haphic_refsort_reference_for_test')
    theirs = {c.name: rc.run_reference(F, c, str(tmp_path / 'theirs' / str(k))) for k, c in enumerate(CASES)}
    saved = patch.patch_refsort(F, engine=ENGINE)
    try:
        assert set(saved) == set(patch.REFSORT_SEAMS)
        for k, c in enumerate(CASES):
            refsort.STATS.clear()
            ours = rc.run_reference(F, c, str(tmp_path / 'ours' / str(k)))
            assert ours == theirs[c.name] == GOLDEN[c.name], c.name
            if c.served:
                assert 'reference' not in refsort.STATS.values() and refsort.STATS['parse_paf'] == 'device', c.name
            else:
                assert 'reference' in refsort.STATS.values(), c.name
    finally:
        for name, fn in saved.items():
            setattr(F, name, fn)
    saved = patch.patch_refsort(F, engine=ENGINE, paf=False)      # the wrapper's default: parse_paf stays the reference's, its dict is flattened all the same
    try:
        assert F.parse_paf is saved['parse_paf'] and F.order_and_orient_groups is not saved['order_and_orient_groups']
        for k, c in enumerate(SERVED):
            refsort.STATS.clear()
            assert rc.run_reference(F, c, str(tmp_path / 'mixed' / str(k))) == GOLDEN[c.name], c.name
            assert 'parse_paf' not in refsort.STATS and refsort.STATS.get('order_and_orient_groups', 'device') == 'device', c.name
    finally:
        for name, fn in saved.items():
            setattr(F, name, fn)
    assert not isinstance(F.parse_fasta(str(tmp_path / 'theirs' / '0' / 'in.fasta')), containers.FastaTable)      # the seams are gone again


# ------------------------------------------------------------------ the command line
def run_main(argv):
    from haphic_amd import __main__ as cli
    with pytest.raises(SystemExit) as e:
        cli.main(list(argv))
    return str(e.value)


def test_refsort_is_a_command_now(monkeypatch):
    monkeypatch.delenv('HAPHIC_REFERENCE', raising=False)
    assert 'HapHiC checkout not found' in run_main(['refsort', '--reference', '/nonexistent'])
    assert '--gpus is a flag of the "cluster" step only' in run_main(['refsort', '--gpus', '2'])
    msg = run_main(['pipeline'])
    assert 'steps only' in msg and all('"%s"' % s in msg for s in ('cluster', 'plot', 'reassign', 'sort', 'build', 'refsort'))
    from haphic_amd import __main__ as cli
    assert 'python -m haphic_amd refsort' in cli.__doc__ and '--keep-reference-refsort' in cli.__doc__ and '--device-paf' in cli.__doc__ and 'intervals.py' in cli.__doc__


def test_library_side_is_declared():
    from haphic_amd import _lib, patch
    for name in ('hhx_paf_open', 'hhx_paf_open_bytes', 'hhx_paf_counts', 'hhx_paf_table', 'hhx_paf_close', 'hhx_lis_sums', 'hhx_fasta_emit_segments'):
        assert name in _lib.SIGNATURES
    assert not hasattr(_lib.Paf, '_release') and _lib.Paf.close(None) is None       # as Gfa: the constructor releases the handle, the object owns nothing
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'haphic_hip.h')).read()
    for cite in ('HapHiC_refsort.py:81-134', 'HapHiC_refsort.py:175-214', 'HapHiC_refsort.py:269-342'):
        assert cite in header, cite
    assert set(patch.REFSORT_SEAMS) == {'parse_fasta', 'parse_paf', 'order_and_orient_groups'}
