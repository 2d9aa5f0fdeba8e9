"""The front of HapHiC_cluster.run() :2785-2831 on the device: from parse_fasta to stat_fragments no sequence byte crosses the bus.

    parse_fasta     :87-113    bind_fasta()   the reader and the RE-site count of `haphic reassign` (reassign.bind_fasta, csrc/hhx_fasta.hip); the
                                              rows of fa_dict are ViewRow: FastaRow + a view (engine, offset, length) of the resident sequences
    parse_gfa       :150-185   bind_gfa()     every file through _lib.Gfa (csrc/hhx_gfa.hip); only the tables of the S records come to the host
    stat_fragments  :188-296   cluster.stat_fragments: while every row still has a view on one engine, the bins and flanks of all contigs are
                                              segments of the resident sequences, counted in one re_counts_device call
    --correct_nrounds          correct.update_bookkeeping: the children of a contig with a view are views (child_row), the RE sites of all
                                              children of a round come from one re_counts_device call (count_children)

The sequences leave HBM when the last row lets go of them: stat_fragments :267 assigns None to element 0 of every row, a row that is deleted
(a broken contig) goes the same way, and the handle's finaliser frees the memory once no row refers to it.  correct_assembly :1267-1269, which stays
the reference's code, reads element 0 of every row to write corrected_asm.fa: a row then fetches its bytes and keeps its view, so stat_fragments
afterwards still counts on the device.

Handed back to the original functions — parse_fasta: what the reader refuses (a byte >= 0x80, a sequence line before the first header, a text
beyond half of the device's memory), repeated contig names, a path that is no file.  parse_gfa: any file the reader refuses (include/haphic_hip.h
lists the cases: too few fields, an integer that is not 1..18 digits, a name beyond 255 bytes, a byte >= 0x80, half of the memory) or that is no
regular file; the original function then takes the whole call before anything is logged, so the result or the exception is Python's own.
stat_fragments and the bookkeeping: a row without a view sends the call (the parent) to the string code."""
import os

import numpy as np

from . import _lib, cluster, containers, reassign

# how a row that is read gets its sequence: every row alone (hhx_fasta_fetch, one copy of its bytes), or the first read brings all sequences over in
# one copy that the rows slice.  The only reader of the default job is correct_assembly :1267-1269, which reads every row
BULK_FETCH = True


class Resident:
    """The sequences of one _lib.Fasta handle as the rows of a fa_dict see them: the rows share it, the handle goes with the last of them."""

    __slots__ = ('engine', '_all')

    def __init__(self, engine):
        self.engine, self._all = engine, None

    def fetch(self, key):
        off, length = key
        if not BULK_FETCH:
            return self.engine.fetch(off, length).decode('ascii')
        if self._all is None:
            self._all = np.ascontiguousarray(self.engine.sequences())
        return str(memoryview(self._all[off:off + length]), 'ascii')


class ViewRow(containers.FastaRow):
    """FastaRow whose sequence is bytes [offset, offset + length) of a Resident.  `view` -> (engine, offset, length) in the handle's sequence
    coordinates; it survives a load of element 0 and dies (None) when element 0 is assigned, as with row[0] = None :267, or the list changes shape."""

    __slots__ = ('_view',)

    def __init__(self, source, off, length, re_sites):
        containers.FastaRow.__init__(self, source.fetch, (off, length), length, re_sites)
        self._view = (source, off, length)

    @property
    def view(self):
        v = self._view
        return None if v is None else (v[0].engine, v[1], v[2])

    @property
    def source(self):
        v = self._view
        return None if v is None else v[0]

    def __setitem__(self, index, value):
        if isinstance(index, slice) or index in (0, -3):
            self._view = None
        containers.FastaRow.__setitem__(self, index, value)


def _dropping(name):
    def method(self, *args, **kwargs):
        self._view = None
        return getattr(containers.FastaRow, name)(self, *args, **kwargs)
    method.__name__ = name
    return method


for _name in ('__delitem__', '__iadd__', '__imul__', 'sort', 'reverse', 'append', 'extend', 'insert', 'pop', 'remove', 'clear'):
    setattr(ViewRow, _name, _dropping(_name))


def view_rows(fa, off, lengths, re_sites):
    """the rows of one handle, for reassign.bind_fasta"""
    source = Resident(fa)
    return map(ViewRow, [source] * len(off), off, lengths, re_sites)


def bind_fasta(H, engine=None, original=None):
    """-> the mirror of parse_fasta :87-113 for the module H: reassign.bind_fasta with rows that carry a view"""
    return reassign.bind_fasta(H, engine, original, rows=view_rows)


# ------------------------------------------------------------------ the children of --correct_nrounds (correct.update_bookkeeping)
def child_row(parent, start, end):
    """the row of parent[start:end] :1030-1032 for a parent with a view, RE sites still to be counted (count_children)"""
    source, off, _length = parent._view
    return ViewRow(source, off + start, end - start, 0)


def count_children(rows, RE):
    """element 2 of every row: count_RE_sites :1031 on its view, all rows of one engine in one re_counts_device call (no pseudo-count here)"""
    by_engine = {}
    for row in rows:
        by_engine.setdefault(id(row._view[0]), []).append(row)
    for group in by_engine.values():
        engine = group[0]._view[0].engine
        counts = engine.re_counts_device(cluster._sites_of(RE), np.fromiter((r._view[1] for r in group), np.int64, len(group)),
                                         np.fromiter((r._view[2] for r in group), np.int64, len(group)))
        for row, c in zip(group, counts.tolist()):
            row[2] = c


# ------------------------------------------------------------------ parse_gfa
def bind_gfa(M, engine=None, original=None):
    """-> the mirror of parse_gfa :150-185 for the module M (HapHiC_cluster, or HapHiC_reassign which imports the function :23).  The files are
    opened one after the other and only their tables are kept.  engine: a stand-in for _lib.Gfa (the tests' host reader)."""
    Engine = engine if engine is not None else _lib.Gfa
    if original is None:
        original = M.parse_gfa
    try:
        import inspect
        default_logger = inspect.signature(original).parameters['logger'].default
    except (KeyError, TypeError, ValueError):
        default_logger = M.logger

    def parse_gfa(gfa_list, fa_dict, logger=default_logger):
        tables = []
        for gfa in gfa_list:
            if not (isinstance(gfa, (str, os.PathLike)) and os.path.isfile(gfa)):
                return original(gfa_list, fa_dict, logger)
            try:
                g = Engine(gfa)
            except Engine.Unsupported:
                return original(gfa_list, fa_dict, logger)
            try:
                tables.append((g.names(), np.asarray(g.lengths, np.int64).tolist(), np.asarray(g.depths, np.int64).tolist()))
            finally:
                g.close()
        logger.info('Parsing input gfa file(s)...')
        read_depth_dict = dict()
        for n, (gfa, (names, lengths, depths)) in enumerate(zip(gfa_list, tables)):
            for ctg, ctg_len in zip(names, lengths):                 # contig length check :166, in file order
                if ctg in fa_dict and ctg_len != fa_dict[ctg][1]:
                    logger.error('The contig {} in gfa file {} has a different length than the one in the fasta file. '
                                 'Maybe the gfa file does not match the fasta file.'.format(ctg, gfa))
                    raise RuntimeError('The contig {} in gfa file {} has a different length than the one in the fasta file. '
                                       'Maybe the gfa file(s) does not match the fasta file.'.format(ctg, gfa))
            read_depth_dict.update(zip(names, zip([n] * len(names), depths)))      # :171: the first position, the last value
        for ctg in fa_dict:                                          # :174
            if ctg not in read_depth_dict:
                logger.error('Can not find contig {} in the gfa file(s). Maybe the gfa file(s) does not match the fasta file.'.format(ctg))
                raise RuntimeError('Can not find contig {} in the gfa file(s). Maybe the gfa file(s) does not match the fasta file.'.format(ctg))
        gfa_seq_num, fa_seq_num = len(read_depth_dict), len(fa_dict)
        if gfa_seq_num > fa_seq_num:
            logger.warning('The number of contigs in the gfa file(s) ({}) is greater than that in the fasta file ({}). '
                           'Maybe some contigs were removed in the fasta file?'.format(gfa_seq_num, fa_seq_num))
        return read_depth_dict

    return parse_gfa
