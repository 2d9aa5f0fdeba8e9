"""Cases and a numpy engine for `haphic refsort` on the device (haphic_amd/refsort.py, csrc/hhx_paf.hip, hhx_lis_sums, hhx_fasta_emit_segments).

NumpyEngine has the interface of the haphic_amd._lib module as far as the mirrors use it — Paf (the reader restated over Python's own text-mode lines
and str.split()), lis_sums (find_lis, HapHiC_refsort.py:175-214, restated as the O(n^2) recurrence on integers), Fasta (tests/build_cases.py's, with
emit_segments restated as array gathers) — so the mirrors run without a GPU and the device has a second statement to agree with.
tests/golden/refsort.npz (make_golden_refsort.py) pins both to what the reference's own functions and run() gave on cases()."""
import io
import json
import logging
import os
import re
import types
from collections import defaultdict

import numpy as np

from tests import build_cases as bc

MAX_N = 1 << 18                # HHX_SORT_VERDICT_MAX_N
_INT = re.compile(r'[0-9]{1,18}\Z')


# ------------------------------------------------------------------ the engine
class NumpyPaf:
    class Unsupported(RuntimeError):
        pass

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            if not os.path.isfile(source):
                if os.path.exists(source):
                    raise NumpyPaf.Unsupported('no regular file')
                raise RuntimeError('cannot open {}'.format(source))
            with open(source, 'rb') as f:
                source = f.read()
        data = bytes(source)
        if any(b >= 0x80 for b in data):
            raise NumpyPaf.Unsupported('a byte >= 0x80')
        ids, names, rows = {}, [], []

        def name_id(s):
            if len(s) > 255:
                raise NumpyPaf.Unsupported('a name beyond 255 bytes')
            if s not in ids:
                ids[s] = len(names)
                names.append(s)
            return ids[s]
        for n, line in enumerate(io.TextIOWrapper(io.BytesIO(data), encoding='ascii', newline=None), 1):
            if not line.strip():
                continue
            cols = line.split()
            if len(cols) < 12:
                raise NumpyPaf.Unsupported('line {}: fewer than 12 fields'.format(n))
            for k in (2, 3, 7, 8, 11):
                if not _INT.match(cols[k]):
                    raise NumpyPaf.Unsupported('line {}: field {}'.format(n, k))
            q = name_id(cols[0])
            rows.append((q, name_id(cols[5]), int(cols[2]), int(cols[3]), int(cols[7]), int(cols[8]), int(cols[11]), cols[4] == '+'))
        t = np.array(rows, np.int64).reshape(-1, 8)
        self._names, self.n_rec, self.n_names = names, len(rows), len(names)
        self.query, self.target = t[:, 0].astype(np.int32), t[:, 1].astype(np.int32)
        self.query_start, self.query_end, self.target_start, self.target_end, self.mapq = (np.ascontiguousarray(t[:, k]) for k in range(2, 7))
        self.plus = t[:, 7].astype(bool)

    def names(self):
        return list(self._names)

    def close(self):
        pass


class LisUnsupported(RuntimeError):
    pass


def lis_class_sum(values, weights, forward):
    """find_lis :175-214 of one class on integer keys: the O(n^2) recurrence, the sum only"""
    seen, vs, ws = set(), [], []
    for v, w in zip(values, weights):
        if (forward and v < 0) or (not forward and v > 0) or v in seen:
            continue
        seen.add(v)
        vs.append(v)
        ws.append(w)
    dp = []
    for i, (v, w) in enumerate(zip(vs, ws)):
        dp.append(w + max([dp[j] for j in range(i) if vs[j] < v] or [0]))
    return max(dp) if dp else 0


def lis_sums(ptr, value, weight, max_n=MAX_N):
    ptr, value, weight = np.asarray(ptr, np.int64).tolist(), np.asarray(value, np.int64).tolist(), np.asarray(weight, np.int64).tolist()
    sf, sr = [], []
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b - a > max_n or any(w <= 0 for w in weight[a:b]) or sum(weight[a:b]) >= 1 << 62:
            raise LisUnsupported('sequence [{}, {})'.format(a, b))
        sf.append(lis_class_sum(value[a:b], weight[a:b], True))
        sr.append(lis_class_sum(value[a:b], weight[a:b], False))
    return np.array(sf, np.int64), np.array(sr, np.int64)


class NumpyFasta(bc.NumpyFasta):
    Unsupported = bc.NumpyFasta.Unsupported

    def emit_segments(self, path, rec_names, piece_off, piece_ctg, piece_start, piece_len, piece_rev, max_width):
        if max_width < 1:
            raise self.Unsupported('max_width {}'.format(max_width))
        for c, s, m in zip(piece_ctg, piece_start, piece_len):
            if m < 0 or (c >= 0 and not 0 <= s <= s + m <= self.seq_len[c]):
                raise self.Unsupported('a piece outside its contig')
        out = []
        for r, name in enumerate(rec_names):
            parts = [np.zeros(0, np.uint8)]
            for k in range(piece_off[r], piece_off[r + 1]):
                c, s, m = int(piece_ctg[k]), int(piece_start[k]), int(piece_len[k])
                if c < 0:
                    parts.append(np.full(m, ord('N'), np.uint8))
                else:
                    x = self._seq[self.seq_off[c] + s:self.seq_off[c] + s + m]
                    parts.append(bc._COMP[x][::-1] if piece_rev[k] else x)
            seq = np.concatenate(parts)
            n_lines = -(-seq.size // max_width)
            body = np.full(seq.size + n_lines, ord('\n'), np.uint8)
            at = np.arange(seq.size, dtype=np.int64)
            body[at + at // max_width] = seq
            out.append(b'>' + name.encode() + b'\n' + body.tobytes())
        data = b''.join(out)
        with open(path, 'wb') as f:
            f.write(data)
        return len(data)


NumpyEngine = types.SimpleNamespace(Paf=NumpyPaf, Fasta=NumpyFasta, lis_sums=lis_sums, LisUnsupported=LisUnsupported)


# ------------------------------------------------------------------ cases
class Case:
    """agp, paf: the texts of the two files (bytes); fasta: bytes of the draft assembly or None (no --fasta); the arguments of haphic refsort.
    served: the mirrors take it on the device (False: some call is handed back, the result is still the reference's)"""

    def __init__(self, name, agp, paf, fasta=None, min_ctg_len=0, aln_len_cutoff=20, skip_aln_check=False, keep_original_ids=False, max_width=60,
                 ref_order=None, served=True):
        self.name, self.agp, self.paf, self.fasta = name, agp, paf, fasta
        self.min_ctg_len, self.aln_len_cutoff, self.skip_aln_check, self.keep_original_ids = min_ctg_len, aln_len_cutoff, skip_aln_check, keep_original_ids
        self.max_width, self.ref_order, self.served = max_width, ref_order, served

    def __repr__(self):
        return self.name

    def write(self, directory):
        """the input files in `directory` -> the args namespace of HapHiC_refsort.run (fout relative to the working directory)"""
        paths = {}
        for key, data in (('agp', self.agp), ('paf', self.paf), ('fasta', self.fasta)):
            paths[key] = None
            if data is not None:
                paths[key] = os.path.join(directory, 'in.' + key)
                with open(paths[key], 'wb') as f:
                    f.write(data)
        return types.SimpleNamespace(agp=paths['agp'], paf=paths['paf'], fasta=paths['fasta'], min_ctg_len=self.min_ctg_len, aln_len_cutoff=self.aln_len_cutoff,
                                     skip_aln_check=self.skip_aln_check, keep_original_ids=self.keep_original_ids, max_width=self.max_width,
                                     fout='scaffolds.refsort.fa', ref_order=self.ref_order)


LENGTHS = {'c0': 300, 'c1': 217, 'c2': 260, 'c3': 333, 'c4': 300, 'c5': 240, 'c6': 199, 'c7': 120, 'c8': 75, 'c9': 150, 'c10': 64}


def fasta_text(seed=11):
    rng = np.random.default_rng(seed)
    return b''.join(b'>' + n.encode() + b' len=%d\n' % m + bc.wrap(bc.bases(rng, m), 60) for n, m in LENGTHS.items())


def agp_text(groups):
    """groups: [(name, [(ctg, start, end, orient) | int Ns, ...])] -> AGP lines as `haphic build` writes them"""
    out = []
    for group, parts in groups:
        acc = 0
        for n, part in enumerate(parts, 1):
            if isinstance(part, int):
                out.append('{}\t{}\t{}\t{}\tU\t{}\tscaffold\tyes\tproximity_ligation\n'.format(group, acc + 1, acc + part, n, part))
                acc += part
            else:
                ctg, start, end, orient = part
                out.append('{}\t{}\t{}\t{}\tW\t{}\t{}\t{}\t{}\n'.format(group, acc + 1, acc + end - start + 1, n, ctg, start, end, orient))
                acc += end - start + 1
    return ''.join(out).encode()


def paf_text(alns, eol='\n', tag=''):
    """alns: [(ctg, qs, qe, strand, ref, rs, re, mapq)] -> PAF lines (12 fields, then `tag`)"""
    return ''.join('{0}\t{8}\t{1}\t{2}\t{3}\t{4}\t100000\t{5}\t{6}\t{9}\t{9}\t{7}{10}{11}'.format(
        c, qs, qe, strand, ref, rs, re, mapq, LENGTHS.get(c, 1000), qe - qs, tag, eol) for c, qs, qe, strand, ref, rs, re, mapq in alns).encode()


def whole(ctg, orient='+'):
    return (ctg, 1, LENGTHS[ctg], orient)


BASE_GROUPS = [('group1', [whole('c0'), 100, whole('c1', '-'), 100, whole('c2')]),
               ('group2', [whole('c3', '-'), 0, whole('c4')]),
               ('group3', [whole('c5'), 100, whole('c6', '-')]),
               ('c7', [whole('c7')]),
               ('c8', [whole('c8')])]
# group1 lies forward on chr1, group2 reversed on chr2, group3 forward on chr1 with a smaller sum; c7 / c8 have no alignment at all
BASE_ALNS = [('c0', 10, 110, '+', 'chr1', 1000, 1100, 60), ('c0', 150, 290, '+', 'chr1', 1200, 1340, 60),
             ('c1', 20, 200, '-', 'chr1', 2000, 2180, 60), ('c2', 5, 255, '+', 'chr1', 3000, 3250, 30),
             ('c3', 30, 300, '+', 'chr2', 9000, 9270, 60), ('c4', 10, 280, '-', 'chr2', 5000, 5270, 60),
             ('c5', 40, 200, '+', 'chr1', 20000, 20160, 60), ('c6', 10, 100, '-', 'chr1', 21000, 21090, 1),
             ('c9', 1, 140, '+', 'chr1', 500, 640, 60)]                               # c9: not in the AGP file


def cases():
    fa = fasta_text()
    base_agp, base_paf = agp_text(BASE_GROUPS), paf_text(BASE_ALNS)
    out = [Case('both_orientations', base_agp, base_paf, fa, skip_aln_check=True),
           Case('no_fasta', base_agp, base_paf, None, skip_aln_check=True),
           Case('keep_original_ids', base_agp, base_paf, fa, skip_aln_check=True, keep_original_ids=True),
           Case('ref_order', base_agp, base_paf, fa, skip_aln_check=True, ref_order='chr2,chr1'),
           Case('ref_order_leaves_one_out', base_agp, base_paf, fa, skip_aln_check=True, ref_order='chr2,chrX'),
           Case('solo_under_min_ctg_len', base_agp, base_paf, fa, min_ctg_len=10),           # c7 / c8 are one_ctg_groups: the check passes
           Case('alignment_check_fails', base_agp, base_paf, fa),                            # min_ctg_len 0: c7 / c8 must have alignments
           Case('crlf_tags_blank_lines', base_agp, b'\r\n \t\r\n' + paf_text(BASE_ALNS, '\r\n', '\ttp:A:P\tcg:Z:' + '10M2D' * 40) + b'\n\n', fa,
                skip_aln_check=True)]
    for w in (1, 7):
        out.append(Case('max_width_%d' % w, base_agp, base_paf, fa, skip_aln_check=True, max_width=w))
    # a tie of the two sums goes to the reverse orientation; an empty class counts 0
    out.append(Case('sum_tie', agp_text([('g', [whole('c0'), 100, whole('c1')])]),
                    paf_text([('c0', 10, 110, '+', 'chr1', 100, 200, 60), ('c1', 10, 110, '-', 'chr1', 300, 400, 60)]), fa))
    out.append(Case('empty_forward_class', agp_text([('g', [whole('c0'), 100, whole('c1')])]),
                    paf_text([('c0', 10, 110, '-', 'chr1', 300, 400, 60), ('c1', 10, 150, '-', 'chr1', 100, 240, 60)]), fa))
    # the same order value twice (one query range on two places of the reference): the first in ref_mid order keeps its length
    out.append(Case('repeated_orders', agp_text([('g', [whole('c0'), 100, whole('c1'), 100, whole('c2')])]),
                    paf_text([('c0', 10, 110, '+', 'chr1', 5000, 5100, 60), ('c1', 10, 60, '+', 'chr1', 700, 750, 60), ('c1', 10, 60, '+', 'chr1', 100, 150, 60),
                              ('c1', 9, 61, '+', 'chr1', 6000, 6052, 60), ('c2', 100, 200, '-', 'chr1', 900, 1000, 60), ('c2', 100, 200, '-', 'chr1', 10, 110, 60),
                              ('c0', 10, 110, '+', 'chr1', 50, 150, 60)]), fa))
    # alignments to several references: the largest sum names the reference, the first of equal sums wins; groups of one reference by falling sum
    out.append(Case('several_references', agp_text(BASE_GROUPS[:3]),
                    paf_text([('c0', 10, 110, '+', 'chrA', 100, 200, 60), ('c1', 10, 210, '+', 'chrB', 100, 300, 60), ('c2', 10, 110, '+', 'chrA', 400, 500, 60),
                              ('c3', 10, 110, '+', 'chrB', 900, 1000, 60), ('c4', 10, 110, '+', 'chrA', 900, 1000, 60),
                              ('c5', 10, 230, '-', 'chrB', 2000, 2220, 60), ('c6', 10, 20, '+', 'chrA', 1, 11, 60)]), fa, aln_len_cutoff=5))
    # mapq 0 and 00, alignments below the cutoff, and what is left
    out.append(Case('filters', agp_text(BASE_GROUPS[:1]),
                    paf_text([('c0', 10, 110, '+', 'chr1', 100, 200, 0), ('c0', 10, 110, '+', 'chr2', 100, 200, '00'), ('c0', 10, 29, '+', 'chr3', 100, 119, 60),
                              ('c0', 10, 30, '+', 'chr4', 100, 120, 60), ('c1', 1, 217, '+', 'chr4', 300, 516, '01'), ('c2', 5, 255, 'x', 'chr4', 3000, 3250, 7)]), fa))
    # scaffolds.raw.agp after assembly correction: c4 broken into two groups; an alignment goes to the group it overlaps most (a tie and no overlap:
    # the first), and :228 walks both entries of c4 whatever the group
    split = [('group2', [whole('c3', '-'), 100, ('c4', 1, 150, '+')]), ('group3', [('c4', 151, 300, '-'), 100, whole('c5')])]
    out.append(Case('contig_in_two_groups', agp_text(split),
                    paf_text([('c4', 10, 140, '+', 'chr1', 1000, 1130, 60), ('c4', 160, 290, '+', 'chr2', 4000, 4130, 60), ('c4', 100, 201, '+', 'chr1', 1100, 1201, 60),
                              ('c4', 120, 200, '-', 'chr2', 4300, 4380, 60), ('c3', 10, 300, '-', 'chr1', 500, 790, 60), ('c5', 10, 200, '+', 'chr2', 4500, 4690, 60),
                              ('c4', 140, 165, '+', 'chr2', 4200, 4225, 60), ('c4', 305, 330, '+', 'chr1', 1300, 1325, 60)]), fa))
    # a group that is one gap of 0 N: a header line and nothing else; gap lines of 0 and 100 N beside it
    out.append(Case('empty_record', agp_text([('group1', [whole('c0'), 0, whole('c1'), 100, whole('c2')]), ('hole', [0]), ('c8', [whole('c8')])]),
                    paf_text(BASE_ALNS[:4]), fa, skip_aln_check=True, max_width=7))
    # handed back, whole: the results are the reference's
    out.append(Case('handback/int_with_sign', base_agp, base_paf.replace(b'\t10\t110\t', b'\t+10\t1_10\t', 1), fa, skip_aln_check=True, served=False))
    out.append(Case('handback/eleven_fields', base_agp, base_paf + b'c0\t300\t10\t110\t+\tchr1\t100000\t1000\t1100\t100\t100\n', fa, skip_aln_check=True,
                    served=False))
    out.append(Case('handback/slice_beyond_the_contig', agp_text([('g', [('c0', 250, 400, '+'), -3, whole('c1')])]), paf_text(BASE_ALNS[:3]), fa, served=False))
    return out


SERVED = ('parse_fasta', 'parse_paf', 'order_and_orient_groups')


# ------------------------------------------------------------------ what run() does around the three functions, restated (the tests run where the reference is absent)
def parse_agp(agp, min_ctg_len):
    """parse_agp :28-64 restated, its pop() quirk included: while it walks the REVERSED entries of a solo contig it pops the FORWARD index"""
    ctg_group, group_ctg, group_len, group_lines = defaultdict(list), defaultdict(list), defaultdict(int), defaultdict(list)
    with open(agp) as f:
        for line in f:
            if not line.strip() or line.startswith('#'):
                continue
            cols = line.split()
            group, g0, g1 = cols[0], int(cols[1]), int(cols[2])
            group_len[group] = max(group_len[group], g1)
            group_lines[group].append(line)
            if cols[4] == 'W':
                c0, c1 = int(cols[6]), int(cols[7])
                ctg_group[cols[5]].append((group, c0, c1, g0, g1, 1 if cols[8] == '+' else -1))
                group_ctg[group].append((cols[5], c1 - c0 + 1))
    solo = set()
    for group, members in group_ctg.items():
        if len(members) == 1 and members[0][1] < min_ctg_len * 1000000:
            solo.add(group)
            entries = ctg_group[members[0][0]]
            for i, info in enumerate(entries[::-1]):
                if info[0] == group:
                    entries.pop(i)
    return ctg_group, group_lines, group_len, solo


def alignment_check(group_len, group_ref, solo, cutoff):
    missing = [g for g in group_len if g not in group_ref and g not in solo]
    if missing:
        raise Exception('Alignment check failed. Cannot find any alignment >= {} bp in the following group(s): {}'.format(cutoff, ','.join(missing)))


class ListLogger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)

    error = info


def plain(group_ref_dict):
    """the nested dict as JSON holds it: lists in insertion order, so that the orders are compared too"""
    return [[group, [[ref, [list(a) for a in alns], total] for ref, (alns, total) in refs.items()]] for group, refs in group_ref_dict.items()]


def run_mirrors(case, directory, engine, refsort, scaffolds, originals=None, paf_source='path'):
    """run() :398-409 with the three mirrors and `engine` in a fresh directory -> the record golden() holds for the case.  originals: {name: function}
    the handed-back calls go to"""
    import contextlib
    originals = originals or {}
    os.makedirs(directory, exist_ok=True)
    args = case.write(directory)
    work = os.path.join(directory, 'run')
    os.mkdir(work)
    rec = {'raises': '', 'paf': None, 'stdout': '', 'log': [], 'fa': None}
    log, stdout = ListLogger(), io.StringIO()

    def body():
        ctg_group, group_lines, group_len, solo = parse_agp(args.agp, args.min_ctg_len)
        group_ref = refsort.parse_paf(args.paf if paf_source == 'path' else case.paf, ctg_group, args.aln_len_cutoff, _original=originals.get('parse_paf'),
                                      _engine=engine, _logger=ListLogger())
        rec['paf'] = plain(group_ref)
        if not args.skip_aln_check:
            alignment_check(group_len, group_ref, solo, args.aln_len_cutoff)
        extra = dict(_original=originals.get('order_and_orient_groups'), _engine=engine, _logger=log)
        with contextlib.redirect_stdout(stdout):
            if args.fasta:
                fa_dict = scaffolds.parse_fasta(args.fasta, _original=originals.get('parse_fasta'), _engine=engine.Fasta, logger=ListLogger())
                with open(args.fout, 'w') as fout:
                    refsort.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args, fa_dict, fout, **extra)
            else:
                refsort.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args, **extra)
    try:
        bc.run_in(work, body)
    except Exception as e:
        rec['raises'] = type(e).__name__
        return rec
    rec['stdout'], rec['log'] = stdout.getvalue(), log.lines
    if args.fasta:
        rec['fa'] = open(os.path.join(work, args.fout), 'rb').read().decode('ascii')
    return rec


class _Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def run_reference(F, case, directory):
    """the same record from the functions of the module F (HapHiC_refsort, with or without the seams) as run() :398-409 calls them"""
    import contextlib
    os.makedirs(directory, exist_ok=True)
    args = case.write(directory)
    work = os.path.join(directory, 'run')
    os.mkdir(work)
    rec = {'raises': '', 'paf': None, 'stdout': '', 'log': [], 'fa': None}
    cap, stdout = _Capture(), io.StringIO()

    def body():
        ctg_group, group_lines, group_len, solo = F.parse_agp(args.agp, args.min_ctg_len)
        group_ref = F.parse_paf(args.paf, ctg_group, args.aln_len_cutoff)
        rec['paf'] = plain(group_ref)
        if not args.skip_aln_check:
            F.alignment_check(group_len, group_ref, solo, args.aln_len_cutoff)
        F.logger.addHandler(cap)
        try:
            with contextlib.redirect_stdout(stdout):
                if args.fasta:
                    fa_dict = F.parse_fasta(args.fasta)
                    cap.lines.clear()                            # (the line of parse_fasta)
                    with open(args.fout, 'w') as fout:
                        F.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args, fa_dict, fout)
                else:
                    F.order_and_orient_groups(ctg_group, group_ref, group_lines, group_len, solo, args)
        finally:
            F.logger.removeHandler(cap)
    try:
        bc.run_in(work, body)
    except Exception as e:
        rec['raises'] = type(e).__name__
        return rec
    rec['stdout'], rec['log'] = stdout.getvalue(), cap.lines
    if args.fasta:
        rec['fa'] = open(os.path.join(work, args.fout), 'rb').read().decode('ascii')
    return rec


def golden(z):
    """{case name: record} of tests/golden/refsort.npz"""
    return json.loads(z['records'].tobytes().decode('ascii'))


def golden_inputs(z):
    """{case name: [agp, paf, fasta or None]} as the fixture recorded them: what cases() must still generate"""
    return json.loads(z['inputs'].tobytes().decode('ascii'))
