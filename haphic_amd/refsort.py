"""`haphic refsort` on the device: the mirrors of the three functions of scripts/HapHiC_refsort.py that walk the PAF file, the alignments and the genome.

    parse_fasta              HapHiC_cluster.py:87-113 (imported by HapHiC_refsort.py:16)  -> scaffolds.parse_fasta: containers.FastaTable over _lib.Fasta
    parse_paf                HapHiC_refsort.py:81-134    -> the table of _lib.Paf (csrc/hhx_paf.hip), filtered and grouped with numpy
    order_and_orient_groups  HapHiC_refsort.py:151-342   -> both find_lis sums of all groups by one _lib.lis_sums call (csrc/hhx_sortverdict.hip), the AGP
                                                            lines from host code, the FASTA records by one Fasta.emit_segments call (csrc/hhx_fasta.hip)

parse_agp, get_max_ovl_group, alignment_check, the argument parser and run() :383-412 stay the reference's.  What the device does not serve goes to the
reference's own function (`_original`, bound by patch.patch_refsort) WHOLE, before a line is logged or printed: a PAF file the reader refuses
(include/haphic_hip.h lists the cases) or whose coordinates reach 2^52 (the mids are float64); a fa_dict that is no frozen FastaTable; an fout without
a usable `name`; max_width < 1; an AGP line whose slice is not 1 <= start <= end <= len(contig), whose N count is negative, whose contig is not in
the FASTA file or whose orientation is neither '+' nor '-' (Python's slicing, KeyError and the reference's assertions decide those); a group beyond
the LIS limit or with a weight <= 0; a group_ref_dict that does not flatten into arrays.
STATS says which engine ran each of the three pieces in the last run: 'device' or 'reference'.
`engine`: a stand-in for the _lib module with Paf, lis_sums, LisUnsupported (and Fasta for parse_fasta); tests/refsort_cases.py has a numpy one."""
import logging
import os
from collections import defaultdict

import numpy as np

from .containers import FastaTable

logger = logging.getLogger(__name__)

STATS = {}     # 'parse_fasta' / 'parse_paf' / 'order_and_orient_groups' -> 'device' | 'reference', of the last call of each

EXACT = 1 << 52            # below it the mids and 2 * order are exact in float64


class _HandBack(Exception):
    """the call goes to the reference's function"""


def _engine_of(engine):
    if engine is None:
        from . import _lib
        return _lib
    return engine


class PafGroups(defaultdict):
    """group_ref_dict as parse_paf :85 builds it — a defaultdict(dict) — that remembers it came from the mirror"""

    def __init__(self):
        defaultdict.__init__(self, dict)


def _max_ovl_group(groups, ctg_aln_start, ctg_aln_end):
    """get_max_ovl_group :67-78 on plain integers: the first strictly larger overlap wins, an empty overlap counts 0"""
    max_ovl_group, max_ovl = None, -1
    for group, ctg_start, ctg_end, _, __, ___ in groups:
        empty = ctg_start > ctg_end or ctg_aln_start > ctg_aln_end
        lo, hi = max(ctg_start, ctg_aln_start), min(ctg_end, ctg_aln_end)
        ovl_len = 0 if empty or lo > hi else hi - lo + 1
        if ovl_len > max_ovl:
            max_ovl, max_ovl_group = ovl_len, group
    return max_ovl_group


def _group_ref_dict(tab, ctg_group_dict, aln_len_cutoff):
    """:87-132 over the table of the reader"""
    out = PafGroups()
    names = tab.names()
    n_entries = np.full(max(len(names), 1), -1, np.int64)       # ctg in ctg_group_dict :101 -> len(ctg_group_dict[ctg])
    for k, name in enumerate(names):
        if name in ctg_group_dict:
            n_entries[k] = len(ctg_group_dict[name])
    keep = (tab.mapq >= 1) & (tab.query_end - tab.query_start >= aln_len_cutoff)       # :91, :98
    keep &= n_entries[tab.query] >= 1                                                  # :101-105
    idx = np.flatnonzero(keep)
    if idx.size == 0:
        return out
    q, t = tab.query[idx].astype(np.int64), tab.target[idx].astype(np.int64)
    qs, qe, ts, te = tab.query_start[idx], tab.query_end[idx], tab.target_start[idx], tab.target_end[idx]
    if max(int(qs.max()), int(qe.max()), int(ts.max()), int(te.max())) >= EXACT:
        raise _HandBack('a coordinate of 2^52 or more')
    group_ids, group_names = {}, []

    def gid_of(group):
        k = group_ids.get(group)
        if k is None:
            k = group_ids[group] = len(group_names)
            group_names.append(group)
        return k
    single = np.full(len(names), -1, np.int64)                  # :109-110
    for k in np.flatnonzero(n_entries == 1).tolist():
        single[k] = gid_of(ctg_group_dict[names[k]][0][0])
    gid = single[q]
    for j in np.flatnonzero(n_entries[q] > 1).tolist():         # :112-113, scaffolds.raw.agp after assembly correction
        gid[j] = gid_of(_max_ovl_group(ctg_group_dict[names[q[j]]], int(qs[j]), int(qe[j])))
    aln_len = qe - qs + 1
    rows = list(zip([names[k] for k in q.tolist()], aln_len.tolist(), ((qe - qs) / 2 + qs).tolist(), ((te - ts) / 2 + ts).tolist(),
                    np.where(tab.plus[idx], 1, -1).tolist()))
    key = gid * len(names) + t
    order = np.argsort(key, kind='stable')
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    begin = np.cumsum(count) - count
    for p in np.argsort(first, kind='stable').tolist():         # (group, ref) pairs as the file meets them: the insertion orders of both dicts
        lines = order[begin[p]:begin[p] + count[p]]
        group, ref = group_names[int(uniq[p]) // len(names)], names[int(uniq[p]) % len(names)]
        out[group][ref] = [[rows[k] for k in lines.tolist()], int(aln_len[lines].sum())]
    return out


def parse_paf(paf, ctg_group_dict, aln_len_cutoff, _original=None, _engine=None, _logger=logger):
    """parse_paf() :81-134 -> the reference's nested dict; what the reader refuses -> _original(...)"""
    eng = _engine_of(_engine)
    try:
        tab = eng.Paf(paf)
        out = _group_ref_dict(tab, ctg_group_dict, aln_len_cutoff)
    except (eng.Paf.Unsupported, _HandBack):
        if _original is None:
            raise
        STATS['parse_paf'] = 'reference'
        return _original(paf, ctg_group_dict, aln_len_cutoff)
    _logger.info('Parsing input PAF file...')
    STATS['parse_paf'] = 'device'
    return out


# ------------------------------------------------------------------ order_and_orient_groups
def _sequences(ctg_group_dict, group_ref_dict):
    """:217-244 of every group -> (groups, their max_ref, ptr, value = 2 * order as int64, weight) in the order find_lis sees them"""
    groups, refs, ptr, values, weights = [], [], [0], [], []
    entries = {}                                                # ctg -> (ctg_start, ctg_end, group_start, ctg_orient) arrays of ALL its entries :228
    for group, ref_aln_dict in group_ref_dict.items():
        max_ref = max(ref_aln_dict, key=lambda x: ref_aln_dict[x][1])
        ctgs, lens, mids, rmids, orients = zip(*ref_aln_dict[max_ref][0])
        lens, orients = np.asarray(lens), np.asarray(orients)
        mids, rmids = np.asarray(mids, np.float64), np.asarray(rmids, np.float64)
        if lens.dtype.kind != 'i' or orients.dtype.kind != 'i' or lens.ndim != 1:
            raise _HandBack('alignment lengths or orientations that are no integers')
        local, cidx = {}, np.zeros(len(ctgs), np.int64)
        for k, ctg in enumerate(ctgs):
            c = local.get(ctg)
            if c is None:
                c = local[ctg] = len(local)
                if ctg not in entries:
                    e = np.array([(x[1], x[2], x[3], x[5]) for x in ctg_group_dict[ctg]], np.float64).reshape(-1, 4)
                    entries[ctg] = e
            cidx[k] = c
        ent = [entries[ctg] for ctg in local]
        ent_cnt = np.array([len(e) for e in ent], np.int64)
        ent_ptr = np.concatenate([[0], np.cumsum(ent_cnt)])
        ent = np.concatenate(ent) if ent else np.zeros((0, 4))
        rep = ent_cnt[cidx]
        ai = np.repeat(np.arange(len(ctgs)), rep)               # alignment, then its contig's entries in their order :226-228
        ei = ent_ptr[cidx[ai]] + (np.arange(ai.size) - np.repeat(np.cumsum(rep) - rep, rep))
        ok = (ent[ei, 0] <= mids[ai]) & (mids[ai] <= ent[ei, 1])            # aln_mid in closed(ctg_start, ctg_end) :229
        ai, ei = ai[ok], ei[ok]
        sign = orients[ai] * ent[ei, 3]
        if not np.isin(sign, (1, -1)).all():                    # the reference's assertion :234
            raise _HandBack('an orientation product that is neither 1 nor -1')
        order = ent[ei, 2] + mids[ai]
        order = np.where(sign == 1, order, -order)
        by_ref = np.argsort(rmids[ai], kind='stable')           # :240
        twice = 2 * order[by_ref]
        if twice.size and not (np.abs(twice).max() < EXACT and (twice == np.rint(twice)).all()):
            raise _HandBack('an order that is no multiple of 0.5 below 2^51')
        groups.append(group)
        refs.append(max_ref)
        values.append(twice.astype(np.int64))
        weights.append(lens[ai][by_ref].astype(np.int64))
        ptr.append(ptr[-1] + twice.size)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)      # noqa: E731
    return groups, refs, np.asarray(ptr, np.int64), cat(values), cat(weights)


_FLIP = {'+': '-', '-': '+'}


class _Pieces:
    """the pieces of the records of scaffolds.refsort.fa, checked as Python's slicing and the reference's assertions would decide"""

    def __init__(self, fa_dict):
        self.fa = fa_dict
        self.rec_names, self.off, self.ctg, self.start, self.len, self.rev = [], [0], [], [], [], []

    def contig(self, ctg, start, end, orient):
        start, end = int(start), int(end)
        k = self.fa.index_of(ctg)
        if k < 0 or not 1 <= start <= end <= int(self.fa.lengths[k]) or orient not in _FLIP:
            raise _HandBack('an AGP slice the device does not take')
        self.ctg.append(k)
        self.start.append(start - 1)
        self.len.append(end - start + 1)
        self.rev.append(orient == '-')

    def gap(self, Ns):
        Ns = int(Ns)
        if Ns < 0:
            raise _HandBack('a negative N count')
        self.ctg.append(-1)
        self.start.append(0)
        self.len.append(Ns)
        self.rev.append(False)

    def line(self, cols, orient=None):
        if cols[4] == 'W':
            ctg, start, end, own = cols[5:9]
            self.contig(ctg, start, end, own if orient is None else orient)
        else:
            self.gap(cols[5])

    def end_record(self, name):
        if not name.isascii():
            raise _HandBack('a record name beyond ASCII')
        self.rec_names.append(name)
        self.off.append(len(self.ctg))


def _plan(ctg_group_dict, group_ref_dict, group_agp_lines, group_len_dict, one_ctg_groups, args, fa_dict, fout, eng):
    """everything :217-342 decides -> (LIS log lines, per-record log lines, the text of stdout, _Pieces or None)"""
    pieces = None
    if fout:
        if not (isinstance(fa_dict, FastaTable) and fa_dict.frozen):
            raise _HandBack('fa_dict is no frozen FastaTable')
        if not isinstance(getattr(fout, 'name', None), (str, os.PathLike)) or args.max_width < 1:
            raise _HandBack('fout without a path, or max_width < 1')
        pieces = _Pieces(fa_dict)
    try:
        groups, refs, ptr, value, weight = _sequences(ctg_group_dict, group_ref_dict)
    except (TypeError, ValueError, KeyError, IndexError, AttributeError) as e:
        raise _HandBack('group_ref_dict does not flatten: {!r}'.format(e))
    try:
        sums_f, sums_r = eng.lis_sums(ptr, value, weight)
    except eng.LisUnsupported as e:
        raise _HandBack(str(e))
    lis_log, ref_groups_dict = [], defaultdict(list)
    for group, max_ref, f, r in zip(groups, refs, sums_f.tolist(), sums_r.tolist()):
        lis_log.append('group: {}\tforward LIS: {}\treverse LIS: {}'.format(group, f, r))
        ref_groups_dict[max_ref].append((group, 1, f) if f > r else (group, -1, r))       # :251-254: a tie goes to the reverse orientation
    order_list = sorted(ref_groups_dict.keys()) if not args.ref_order else args.ref_order.split(',')

    rec_log, text, output_groups = [], [], set()
    keep_ids = args.keep_original_ids
    try:
        for ref in order_list:
            ref_groups_dict[ref].sort(key=lambda x: x[-1], reverse=True)
            for group, max_orient, _ in ref_groups_dict[ref]:
                if group in one_ctg_groups or group is None:
                    continue
                output_groups.add(group)
                sign = '+' if max_orient == 1 else '-'
                new_id = group if keep_ids else '{}:{}:{}'.format(group, ref, sign)
                rec_log.append('{}: {} {}'.format(ref, group, sign))
                if max_orient == 1:
                    for line in group_agp_lines[group]:
                        text.append(line if keep_ids else '{}\t{}'.format(new_id, line.split(maxsplit=1)[-1]))
                        if pieces:
                            pieces.line(line.split())
                else:
                    for n, line in enumerate(group_agp_lines[group][::-1], 1):
                        cols = line.split()
                        grp, start, end = cols[0], int(cols[1]), int(cols[2])
                        group_len = group_len_dict[grp]
                        if cols[4] == 'W':
                            if cols[-1] not in _FLIP:
                                raise _HandBack('an orientation that is neither + nor -')
                            last_col = _FLIP[cols[-1]]
                            if pieces:
                                pieces.contig(cols[5], cols[6], cols[7], last_col)
                        else:
                            last_col = cols[-1]
                            if pieces:
                                pieces.gap(cols[5])
                        text.append('{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\n'.format(grp if keep_ids else '{}:{}:-'.format(grp, ref), group_len - end + 1,
                                                                                  group_len - start + 1, n, cols[4], cols[5], cols[6], cols[7], last_col))
                if pieces:
                    pieces.end_record(str(new_id))
        for group, lines in group_agp_lines.items():            # :323-342: the remaining groups (mostly unanchored contigs)
            if group in output_groups:
                continue
            for line in lines:
                text.append(line)
                if pieces:
                    pieces.line(line.split())
            if pieces:
                pieces.end_record(str(group))
    except (ValueError, IndexError, KeyError, TypeError) as e:  # the reference's own statement raises it: let it
        raise _HandBack('an AGP line the mirror does not read: {!r}'.format(e))
    return lis_log, rec_log, ''.join(text), pieces


def order_and_orient_groups(ctg_group_dict, group_ref_dict, group_agp_lines, group_len_dict, one_ctg_groups, args, fa_dict=None, fout=None,
                            _original=None, _engine=None, _logger=logger):
    """order_and_orient_groups() :151-342: the same stdout text, INFO lines and file bytes; the records go to the PATH fout.name, nothing is written
    through fout itself"""
    eng = _engine_of(_engine)
    try:
        lis_log, rec_log, text, pieces = _plan(ctg_group_dict, group_ref_dict, group_agp_lines, group_len_dict, one_ctg_groups, args, fa_dict, fout, eng)
        if pieces:
            fout.flush()
            try:
                fa_dict.engine.emit_segments(fout.name, pieces.rec_names, pieces.off, pieces.ctg, pieces.start, pieces.len, pieces.rev, args.max_width)
            except fa_dict.engine.Unsupported as e:
                raise _HandBack(str(e))
    except _HandBack:
        if _original is None:
            raise
        STATS['order_and_orient_groups'] = 'reference'
        return _original(ctg_group_dict, group_ref_dict, group_agp_lines, group_len_dict, one_ctg_groups, args, fa_dict, fout)
    _logger.info('Ordering and orienting scaffolds based on alignments...')
    for line in lis_log + rec_log:
        _logger.info(line)
    print(text, end='')
    STATS['order_and_orient_groups'] = 'device'
