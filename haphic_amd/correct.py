"""Assembly correction (`haphic cluster --correct_nrounds N`) on the device: mirrors of the reference functions that
correct_assembly() :1200-1297 and run() :2798-2851 resolve through the module globals.

    parse_pairs_for_correction :1300-1344, parse_bam_for_correction :1362-1398
        the alignment file through the device front ends (cluster.PairsText / cluster.BamRecords) into a _lib.CorrectTable:
        coverage bins and (lo, hi) position lists stay in HBM.  They return a CovDict / LinkPosDict pair — dict-shaped, frozen
        like containers.LinkTable: anything but the mirrors below that touches one of them thaws BOTH into the reference's
        `dict` of int32 arrays / `defaultdict` of array('i'), and from then on the mirrors hand over to the original functions.
    detect_break_points :943-1014        one launch over the contigs still in the table
    break_and_update_ctgs :1017-1197     the per-pair loops and the coverage slices on the device, the O(broken contigs)
                                         bookkeeping (fa_dict, child names, the final_break_* dicts, ...) here
    pairs_generator_for_correction(_ctg) :1401-1440 :1473-1509, bam_generator_for_correction(_ctg) :1443-1470 :1512-1536
        the front ends of cluster.py carrying a contig remap (convert_ctg :1405-1411) that cluster._ingest_handle applies on
        the device between the tokeniser / BAM decoder and the ingest; alignments.bed keeps the original names (:1429).

correct_assembly itself — the round loop, corrected_asm.fa, corrected_ctgs.txt, the GFA links — stays the reference's code.
Positions are int32 as in the reference (array('i')); contigs of 2^31 bp and more are refused by _lib.CorrectTable.
After a round of breaking the table holds the children of the broken contigs alone (the reference keeps the dead entries of
ctg_link_pos_dict :1190 and never reads them again); a thaw after that round gives those live entries."""
from array import array
from collections import defaultdict

import numpy as np

from . import _lib, cluster

logger = cluster.logger


# ------------------------------------------------------------------ the two containers
class CorrectionSession:
    """The device table of one correction (a _lib.CorrectTable) and the names of its segments, in ctg_cov_dict order."""

    def __init__(self, table, names):
        self.table, self.names = table, list(names)
        self.cov = self.pos = None
        self.frozen = True

    def cov_items(self):
        off, nb, _len, _po = self.table.segments()
        flat = self.table.coverage()
        return [(n, flat[o:o + k]) for n, o, k in zip(self.names, off.tolist(), nb.tolist())]

    def pos_items(self):
        po = self.table.segments()[3]
        flat = self.table.pairs()
        view = memoryview(flat).cast('B')
        out = []
        for n, a, b in zip(self.names, po[:-1].tolist(), po[1:].tolist()):
            if b > a:                                            # a defaultdict holds the contigs that received a pair (:1342)
                out.append((n, array('i', bytes(view[8 * a:8 * b]))))
        return out

    def thaw(self):
        """both containers become the reference's objects; the device table is released"""
        if not self.frozen:
            return
        cov_items, pos_items = self.cov_items(), self.pos_items()
        self.frozen = False
        for box, items, kind in ((self.cov, cov_items, ThawedCov), (self.pos, pos_items, ThawedPos)):
            if box is not None:
                dict.update(box, items)
                box.__dict__.clear()
                box.__class__ = kind
        self.table.destroy()


class ThawedCov(dict):
    """ctg_cov_dict after a thaw: a dict {contig: ndarray(int32)} in all but the class name"""
    frozen = False


class ThawedPos(defaultdict):
    """ctg_link_pos_dict after a thaw: defaultdict(lambda: array('i')) {contig: array('i', [lo, hi, lo, hi, ...])}"""
    frozen = False


def _thawing(name):
    def method(self, *args, **kwargs):
        self._session.thaw()
        return getattr(self, name)(*args, **kwargs)
    method.__name__ = name
    return method


_DICT_METHODS = ('__getitem__', '__setitem__', '__delitem__', '__contains__', '__iter__', '__reversed__', '__len__', 'keys', 'values', 'items',
                 'get', 'pop', 'popitem', 'setdefault', 'update', 'clear', 'copy', '__eq__', '__ne__', '__repr__', '__or__', '__ror__', '__ior__')


class CovDict(dict):
    """ctg_cov_dict (:1307-1311) while it lives in HBM"""
    frozen = True

    def __init__(self, session):
        dict.__init__(self)
        self._session = session
        session.cov = self

    def __bool__(self):
        return len(self._session.names) > 0


class LinkPosDict(defaultdict):
    """ctg_link_pos_dict (:1308) while it lives in HBM"""
    frozen = True

    def __init__(self, session):
        defaultdict.__init__(self, lambda: array('i'))
        self._session = session
        session.pos = self

    def __bool__(self):
        return self._session.table.shape()[2] > 0


for _name in _DICT_METHODS:
    setattr(CovDict, _name, _thawing(_name))
    setattr(LinkPosDict, _name, _thawing(_name))
setattr(LinkPosDict, '__missing__', _thawing('__missing__'))


def _frozen_session(*containers):
    """the session behind containers that are all still frozen, else None (after thawing whatever is half-way)"""
    sessions = [getattr(c, '_session', None) if getattr(c, 'frozen', False) else None for c in containers]
    if all(s is not None for s in sessions) and all(s is sessions[0] for s in sessions):
        return sessions[0]
    for c in containers:
        if getattr(c, 'frozen', False):
            c._session.thaw()
    return None


# ------------------------------------------------------------------ pass one
def _new_table(fa_dict, args):
    names = list(fa_dict)
    return names, _lib.CorrectTable([fa_dict[c][1] for c in names], args.correct_resolution)


def parse_pairs_for_correction(fa_dict, args):
    """parse_pairs_for_correction() :1300-1344.  In a --gpus N job over a plain or BGZF file every rank fills a table from the lines of its
    own byte range (ranks.py, phase `correct_pass1`); this rank absorbs them in rank order — file order — before it finalizes.  A plain gzip
    stream is read whole by this rank, as for the ingest."""
    import time
    logger.info('Parsing input pairs file for contig correction...')
    assert args.aln_format in ('pairs', 'bgzipped_pairs')
    names, table = _new_table(fa_dict, args)
    try:
        text = cluster.PairsText(args.alignments, args.aln_format, inter_only=False, bed_path=None)
        ranked = text.multi_rank()
        if ranked:
            from . import ranks
            ranks.announce('correct_pass1', ranks.correct_spec(text, names, [fa_dict[c][1] for c in names], args.correct_resolution))
            t0 = time.perf_counter()
            lines = ranks.fill_table(table, text, names)
            kept = table.export_shape()[2]
            ranks.gather_tables(table)
            ranks.record('correct_pass1', lines, kept, time.perf_counter() - t0)
        else:
            for parser, k in text.batches(names):
                if k:
                    table.push_device(k, *parser.device_arrays()[:4])
        table.finalize()
    except BaseException:
        table.destroy()
        raise
    session = CorrectionSession(table, names)
    return CovDict(session), LinkPosDict(session)


def parse_bam_for_correction(fa_dict, args):
    """parse_bam_for_correction() :1362-1398: `flag.read1 && refid == mrefid` :1376 — the decoder marks records that fail flag.read1,
    the table keeps a record iff both ends name the same contig of fa_dict"""
    logger.info('Parsing input BAM file for contig correction...')
    names, table = _new_table(fa_dict, args)
    try:
        records = cluster.BamRecords(args.alignments, args.threads, [b'filter=flag.read1'])
        for _reader, k, ptrs in records.batches(names):
            table.push_device(k, *ptrs)
        table.finalize()
    except BaseException:
        table.destroy()
        raise
    session = CorrectionSession(table, names)
    return CovDict(session), LinkPosDict(session)


# ------------------------------------------------------------------ the rounds
def detect_break_points(ctg_cov_dict, fa_dict, args, _original=None):
    """detect_break_points() :943-1014 -> {contig: [(position, coverage), ...]} in ctg_cov_dict order"""
    session = _frozen_session(ctg_cov_dict)
    if session is None:
        if _original is None:
            raise TypeError('detect_break_points: a plain ctg_cov_dict needs the reference function (patch_reference passes it)')
        return _original(ctg_cov_dict, fa_dict, args)
    res = int(args.correct_resolution)
    n_bp, cov, bins = session.table.detect(args.median_cov_ratio, args.region_len_ratio, args.min_region_cutoff)
    out = {}
    at = 0
    for s in np.flatnonzero(n_bp).tolist():
        k = int(n_bp[s])
        out[session.names[s]] = [(int(b) * res, int(cov[s])) for b in bins[at:at + k]]
        at += k
    return out


def _child_bounds(points, length):
    bounds = [0] + list(points) + [length]
    return list(zip(bounds[:-1], bounds[1:]))


def update_bookkeeping(ctg_break_point_dict, frag_source_dict, final_break_pos_dict, final_break_frag_dict, fa_dict, read_depth_dict, unbroken_ctgs,
                       args, count_re=None):
    """The dict half of break_and_update_ctgs (:1028-1034 :1115-1187): every broken contig leaves fa_dict / read_depth_dict, its children
    `raw:start-end` (1-based, closed, on the ORIGINAL contig) enter them in order, and take the parent's place — in descending order of
    position, which is what convert_ctg :1405-1411 walks — in the two final_break_* lists of their source contig.
    A parent whose row has a view of sequences on the device (haphic_amd/assembly.py) gets children that are views of its view, and the RE sites
    :1031 of all such children of the call come from one re_counts_device call; a parent without a view is sliced and counted as a string.
    -> {contig: [child names]} in ctg_break_point_dict order."""
    from . import assembly
    count_re = count_re or cluster.count_RE_sites
    children, resident = {}, []
    for ctg, break_points in ctg_break_point_dict.items():
        parent = fa_dict[ctg]
        length = parent[1]
        on_device = getattr(parent, 'view', None) is not None
        seq = None if on_device else parent[0]
        if ctg in unbroken_ctgs:
            raw, shift = ctg, 0
        else:
            assert ':' in ctg
            raw, span = ctg.rsplit(':', 1)
            shift = int(span.split('-')[0]) - 1
        source = frag_source_dict[ctg]
        frags, starts = final_break_frag_dict[source], final_break_pos_dict[source]
        at = frags.index(ctg)
        father_pos = starts[at]
        bounds = _child_bounds([p for p, _cov in break_points], length)
        names = ['{}:{}-{}'.format(raw, s + 1 + shift, e + shift) for s, e in bounds]
        frags[at:at + 1] = names[::-1]
        starts[at:at + 1] = [father_pos + s for s, _e in bounds][::-1]
        for name, (s, e) in zip(names, bounds):
            frag_source_dict[name] = source
            if read_depth_dict:
                read_depth_dict[name] = read_depth_dict[ctg]
            if on_device:
                fa_dict[name] = assembly.child_row(parent, s, e)
                resident.append(fa_dict[name])
            else:
                piece = seq[s:e]
                fa_dict[name] = [piece, e - s, count_re(piece, args.RE)]
        del fa_dict[ctg]
        if read_depth_dict:
            del read_depth_dict[ctg]
        children[ctg] = names
    if resident:
        assembly.count_children(resident, args.RE)
    return children


def break_and_update_ctgs(ctg_break_point_dict, ctg_link_pos_dict, ctg_cov_dict, frag_source_dict, final_break_pos_dict, final_break_frag_dict,
                          fa_dict, read_depth_dict, unbroken_ctgs, args, last_round=False, _original=None):
    """break_and_update_ctgs() :1017-1197"""
    session = _frozen_session(ctg_cov_dict, ctg_link_pos_dict)
    if session is None:
        if _original is None:
            raise TypeError('break_and_update_ctgs: plain containers need the reference function (patch_reference passes it)')
        return _original(ctg_break_point_dict, ctg_link_pos_dict, ctg_cov_dict, frag_source_dict, final_break_pos_dict, final_break_frag_dict,
                         fa_dict, read_depth_dict, unbroken_ctgs, args, last_round)
    logger.info('Breaking contigs and updating data...')
    seg_of = {n: s for s, n in enumerate(session.names)}
    if not last_round:                                           # checked before any dict is touched
        missing = [c for c in ctg_break_point_dict if c not in seg_of]
        if missing:
            raise ValueError('break_and_update_ctgs: {} is not in ctg_cov_dict'.format(missing[0]))
        if sorted(ctg_break_point_dict, key=seg_of.__getitem__) != list(ctg_break_point_dict):
            raise ValueError('break_and_update_ctgs: the break points do not follow the order of ctg_cov_dict')
    unbroken_before = set(unbroken_ctgs)
    children = update_bookkeeping(ctg_break_point_dict, frag_source_dict, final_break_pos_dict, final_break_frag_dict, fa_dict, read_depth_dict,
                                  unbroken_ctgs, args)
    if last_round:                                               # only fa_dict and the final dicts are needed (:1232)
        return
    order = list(ctg_break_point_dict)
    seg, bp_off, bp_pos, zero, names = [], [0], [], [], []
    for ctg in order:
        points = ctg_break_point_dict[ctg]
        seg.append(seg_of[ctg])
        bp_pos.extend(p for p, _cov in points)
        bp_off.append(len(bp_pos))
        flag = 1 if points[0][1] == 0 else 0                     # :1068: one zero-coverage break point means all are
        if ctg not in unbroken_before and int(ctg.rsplit(':', 1)[1].split('-')[0]) != 1:
            flag |= 2                                            # pos_shift :1050 misnames the inner children of such a piece: their pairs are lost
        zero.append(flag)
        names.extend(children[ctg])
    session.table.break_(seg, bp_off, bp_pos, zero)
    session.names = names


# ------------------------------------------------------------------ pass two
def _remap_tables(corrected_names, final_break_pos_dict, final_break_frag_dict):
    """-> (source names, off, break_pos, new_id): the names the front end tokenises — the unbroken contigs and the broken ORIGINAL contigs —
    and per source the (break position ascending, id in the corrected FASTA) entries of hhx_remap_create"""
    cid = {n: i for i, n in enumerate(corrected_names)}
    pieces = set()
    for frags in final_break_frag_dict.values():
        pieces.update(frags)
    sources = [n for n in corrected_names if n not in pieces] + list(final_break_frag_dict)
    off, pos, new = [0], [], []
    for n in sources:
        if n in final_break_frag_dict:
            for p, frag in sorted(zip(final_break_pos_dict[n], final_break_frag_dict[n])):
                pos.append(p)
                new.append(cid[frag])
        else:
            pos.append(0)
            new.append(cid[n])
        off.append(len(pos))
    return sources, np.asarray(off, np.int32), np.asarray(pos, np.int32), np.asarray(new, np.int32)


class _Remapped:
    """mixin of the correction-aware front ends: cluster._ingest_handle asks remap_for(names of the corrected FASTA) and gets the names to
    tokenise and the device remap to apply to both (id, position) column pairs of every batch"""

    def _set_remap(self, final_break_pos_dict, final_break_frag_dict):
        self._break_pos, self._break_frag = final_break_pos_dict, final_break_frag_dict

    def remap_for(self, corrected_names):
        sources, off, pos, new = _remap_tables(corrected_names, self._break_pos, self._break_frag)
        self.remap_tables = (off, pos, new)                      # what a multi-rank ingest broadcasts (ranks.ingest_spec)
        return sources, _lib.ContigRemap(off, pos, new)


class CorrectedPairsText(_Remapped, cluster.PairsText):
    """multi_rank() is PairsText's: in a --gpus N job every rank tokenises the ORIGINAL names of its byte range, converts on its own device and
    sends its pairs in rank order; each writes its share of alignments.bed with the original names"""

    def __init__(self, pairs, aln_format, inter_only, final_break_pos_dict, final_break_frag_dict):
        cluster.PairsText.__init__(self, pairs, aln_format, inter_only)
        self._set_remap(final_break_pos_dict, final_break_frag_dict)


class CorrectedBamRecords(_Remapped, cluster.BamRecords):
    def __init__(self, bam, threads, format_options, inter_only, final_break_pos_dict, final_break_frag_dict):
        cluster.BamRecords.__init__(self, bam, threads, format_options)
        if self.drop_same_ref:
            raise NotImplementedError('refid != mrefid is tested after the contig conversion (:1467), not by the BAM filter')
        self.inter_only = inter_only
        self._set_remap(final_break_pos_dict, final_break_frag_dict)

    def multi_rank(self):
        return False                                             # BAM input is read by rank 0 alone


def pairs_generator_for_correction(pairs, aln_format, final_break_pos_dict, final_break_frag_dict):
    """pairs_generator_for_correction() :1473-1509"""
    return CorrectedPairsText(pairs, aln_format, False, final_break_pos_dict, final_break_frag_dict)


def pairs_generator_for_correction_ctg(pairs, aln_format, final_break_pos_dict, final_break_frag_dict):
    """pairs_generator_for_correction_ctg() :1401-1440: ref == mref is dropped AFTER the conversion :1437 (Ingest(skip_intra))"""
    return CorrectedPairsText(pairs, aln_format, True, final_break_pos_dict, final_break_frag_dict)


def bam_generator_for_correction(bam, threads, format_options, final_break_pos_dict, final_break_frag_dict):
    """bam_generator_for_correction() :1512-1536"""
    return CorrectedBamRecords(bam, threads, format_options, False, final_break_pos_dict, final_break_frag_dict)


def bam_generator_for_correction_ctg(bam, threads, format_options, final_break_pos_dict, final_break_frag_dict):
    """bam_generator_for_correction_ctg() :1443-1470"""
    return CorrectedBamRecords(bam, threads, format_options, True, final_break_pos_dict, final_break_frag_dict)
